// Gradient guard (include/maestro_hip.h): global L2 norm of the flat gradient buffer, clipping coefficient and the
// non-finite skip, as the five device scalars of mh_adamw_dev.  Two launches: mh_grad_sumsq_partial streams the gradient once
// (one f32 partial and one inf / NaN count per MH_GUARD_CHUNK elements, plain stores), mh_grad_guard_finish -- one workgroup --
// sums the partials in double and writes hyper[5] + the MhGuardState.  No atomics, every order of additions is fixed by
// (n, lane, wave): the same gradient gives the same bits on every run.
#include "common.hpp"
#include "../../include/maestro_hip.h"
#include <limits.h>

// Loads of the streaming phase: 0 = plain (default), 1 = nontemporal.  Alone, over the 705 MB gradient of C3, the nontemporal form
// is the faster one (110 against 121 us); inside the step it is the slower one (+0.131 against +0.110 ms per step over the
// unguarded step, 15 alternating rounds): AdamW reads the same buffer right after, and what plain loads leave in the caches is
// worth more than the 10 us.  What counts is the step, so plain loads stay (profiles/grad_guard.md); -DMH_GUARD_NT_LOADS=1
// rebuilds the other form.
#ifndef MH_GUARD_NT_LOADS
#define MH_GUARD_NT_LOADS 0
#endif

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int QUADS = MH_GUARD_CHUNK / (4 * THREADS);       // float4 loads per lane and chunk
constexpr int BATCH = 8;                                     // of them in flight before the first is consumed
static_assert(MH_GUARD_CHUNK % (4 * THREADS * BATCH) == 0, "a chunk is a whole number of load batches");

__device__ __forceinline__ f32x4 load4(const float* p) {
#if MH_GUARD_NT_LOADS
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#else
    return *reinterpret_cast<const f32x4*>(p);
#endif
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

__global__ __launch_bounds__(THREADS) void grad_sumsq_partial_kernel(const float* __restrict__ g, long n, float* __restrict__ partial,
                                                                     unsigned* __restrict__ bad) {
    __shared__ float red_s[WAVES];
    __shared__ unsigned red_b[WAVES];
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.x * MH_GUARD_CHUNK;
    const bool whole = base + MH_GUARD_CHUNK <= n;              // uniform: every chunk but the last
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    unsigned nb = 0;
#pragma unroll
    for (int k0 = 0; k0 < QUADS; k0 += BATCH) {
        f32x4 v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const long i = base + 4L * ((k0 + k) * THREADS + tid);
            // the ragged chunk: a quad past n reads nothing and adds +0 (fma(0, 0, acc) == acc: the order is that of the whole chunk)
            v[k] = (whole || i < n) ? load4(g + i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] = __builtin_fmaf(v[k][c], v[k][c], acc[c]);
                nb += (__float_as_uint(v[k][c]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
            }
    }
    float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    nb = wave_sum_u32(nb);
    if ((tid & 63) == 0) { red_s[tid >> 6] = s; red_b[tid >> 6] = nb; }
    __syncthreads();
    if (tid == 0) {
        partial[blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        bad[blockIdx.x] = red_b[0] + red_b[1] + red_b[2] + red_b[3];      // <= MH_GUARD_CHUNK: no overflow
    }
}

// b^t for an integer t >= 0 by repeated squaring: at most 126 double multiplications, relative error <= 126 * 2^-53 -- nothing
// of it survives the rounding to float (t = 1 gives b itself).
__device__ __forceinline__ double pow_int(double b, long long t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(THREADS) void grad_guard_finish_kernel(const float* __restrict__ partial, const unsigned* __restrict__ bad,
                                                                    long rows, float grad_scale, float max_norm, int skip_nonfinite,
                                                                    float lr, float b1, float b2, float* __restrict__ hyper,
                                                                    MhGuardState* __restrict__ state) {
    __shared__ double red_s[THREADS];
    __shared__ unsigned long long red_b[THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    unsigned long long nb = 0;
    for (long r = tid; r < rows; r += THREADS) {
        s += (double)partial[r];
        nb += bad[r];
    }
    red_s[tid] = s;
    red_b[tid] = nb;
    __syncthreads();
#pragma unroll
    for (int o = THREADS / 2; o > 0; o >>= 1) {                 // the fixed tree: slot l += slot l + o
        if (tid < o) { red_s[tid] += red_s[tid + o]; red_b[tid] += red_b[tid + o]; }
        __syncthreads();
    }
    if (tid != 0) return;
    const float norm = (float)((double)fabsf(grad_scale) * sqrt(red_s[0]));
    const unsigned nbad = red_b[0] > (unsigned long long)UINT_MAX ? UINT_MAX : (unsigned)red_b[0];
    const bool finite = isfinite(norm) && nbad == 0;
    const float coef = (max_norm > 0.f && finite) ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
    const bool apply = finite || !skip_nonfinite;
    long long t = state->t;
    if (apply) {
        t += 1;
        state->t = t;
    } else {
        state->skipped += 1;
    }
    state->norm = norm;
    state->coef = coef;
    state->finite = finite ? 1 : 0;
    state->bad = nbad;
    hyper[0] = lr;
    hyper[1] = (float)(1.0 - pow_int((double)b1, t));
    hyper[2] = (float)sqrt(1.0 - pow_int((double)b2, t));
    hyper[3] = grad_scale * coef;
    hyper[4] = apply ? 1.f : 0.f;
}

}  // namespace

static bool finite_f(float x) { return x - x == 0.f; }      // host side: neither inf nor NaN

extern "C" long mh_grad_sumsq_partial_rows(long n) { return n <= 0 ? 0 : (n + MH_GUARD_CHUNK - 1) / MH_GUARD_CHUNK; }

extern "C" int mh_grad_sumsq_partial(const float* g, long n, float* partial, unsigned* bad, void* stream) {
    MH_CHECK_ARG(g && partial && bad, "mh_grad_sumsq_partial: null pointer (g, partial, bad)");
    MH_CHECK_ARG(n > 0 && n % 4 == 0, "mh_grad_sumsq_partial: n %ld must be positive and a multiple of 4", n);
    MH_CHECK_ARG(((uintptr_t)g % 16) == 0, "mh_grad_sumsq_partial: g must be 16-byte aligned");
    const long rows = mh_grad_sumsq_partial_rows(n);
    MH_CHECK_ARG(rows <= 0x7fffffffL, "mh_grad_sumsq_partial: n %ld gives more workgroups than a grid holds", n);
    hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3((unsigned)rows), dim3(THREADS), 0, (hipStream_t)stream, g, n, partial, bad);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_grad_guard_finish(const float* partial, const unsigned* bad, long rows, float grad_scale, float max_norm,
                                    int skip_nonfinite, float lr, float b1, float b2, float* hyper, MhGuardState* state, void* stream) {
    MH_CHECK_ARG(partial && bad && hyper && state, "mh_grad_guard_finish: null pointer (partial, bad, hyper, state)");
    MH_CHECK_ARG(rows >= 1 && rows <= (1L << 24), "mh_grad_guard_finish: rows %ld must be 1 ... 2^24 (mh_grad_sumsq_partial_rows)", rows);
    MH_CHECK_ARG(finite_f(grad_scale) && finite_f(lr) && finite_f(max_norm), "mh_grad_guard_finish: grad_scale, max_norm and lr must be finite");
    MH_CHECK_ARG(b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f, "mh_grad_guard_finish: b1 %g, b2 %g must be in [0, 1)", (double)b1, (double)b2);
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, partial, bad, rows, grad_scale, max_norm,
                       skip_nonfinite, lr, b1, b2, hyper, state);
    MH_LAUNCH_CHECK();
    return 0;
}
