// Scene prediction around the resident prediction path (predict.hip): the window cut in front of it, the weighted accumulation of
// overlapping windows into a scene canvas behind it, and the canvas finish.  C declarations and the full contract: include/maestro_hip.h.
//
// Nothing here is atomic.  The blend is a gather through an inverted index: a canvas pixel is owned by the thread of the LOWEST
// slot whose window covers it, and that thread walks the covering slots in ascending order, so every pixel has one writer and
// one sum order.  The inverted index is the window table itself (B rows in LDS) and, per workgroup, the short list of the slots
// whose windows overlap the workgroup's own window: the O(B) test is paid once per workgroup, not per pixel.
#include "common.hpp"
#include "logits_walk.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_PASSES = 4;               // pixels of a window per blend workgroup: SC_PASSES * SC_THREADS
constexpr int SC_MAX_CHUNKS = 64;          // workgroups along one plane of the gather (they stride over the plane)

// Rounded one by one: a * b and a + b as separate fp32 operations, never contracted into an FMA (the build's default contracts
// a + b * c, and under it __fmul_rn / __fadd_rn are the plain operators), so that the canvas holds the sums include/maestro_hip.h states.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// Row b of the table in pixels of a raster with q pixels per unit and S-pixel windows: false for a row that names no scene or
// leaves the [H, W] raster (such a row is skipped, never followed).
__device__ __forceinline__ bool window_of(const int32_t* __restrict__ table, int b, int N, int q, int S, int H, int W, int& n,
                                          int& py, int& px) {
    n = table[4 * b];
    const long y = (long)table[4 * b + 1] * q, x = (long)table[4 * b + 2] * q;
    py = (int)y;
    px = (int)x;
    return n >= 0 && n < N && y >= 0 && x >= 0 && y + S <= H && x + S <= W;
}

// One plane (b, p) per blockIdx.x; VEC: four pixels per thread, S % 4 == 0, Ws % 4 == 0 and both bases 16-byte aligned (the
// store is always 16 bytes; the load is, too, where the window's first column is a multiple of 4).
template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void window_gather_kernel(const float* __restrict__ scene, float* __restrict__ out,
                                                                   const int32_t* __restrict__ table, int N, int planes, int Hs,
                                                                   int Ws, int S, int q) {
    const int b = blockIdx.x / planes, p = blockIdx.x - b * planes;
    int n, py, px;
    if (!window_of(table, b, N, q, S, Hs, Ws, n, py, px)) return;
    const int per = VEC ? S / 4 : S, items = S * per;
    const float* src = scene + (((size_t)n * planes + p) * Hs + py) * Ws + px;
    float* dst = out + (size_t)blockIdx.x * S * S;
    for (int i = blockIdx.y * SC_THREADS + threadIdx.x; i < items; i += gridDim.y * SC_THREADS) {
        const int y = i / per, x = i - y * per;
        if (VEC) {
            const float* s = src + (size_t)y * Ws + 4 * x;
            f32x4 v;
            if ((px & 3) == 0) v = *reinterpret_cast<const f32x4*>(s);
            else v = (f32x4){s[0], s[1], s[2], s[3]};
            *reinterpret_cast<f32x4*>(dst + (size_t)y * S + 4 * x) = v;
        } else {
            dst[(size_t)y * S + x] = src[(size_t)y * Ws + x];
        }
    }
}

// blockIdx.y = the slot, blockIdx.x = a chunk of SC_PASSES * SC_THREADS pixels of its window in row-major order: consecutive
// threads are consecutive x of one window row, for the canvas and for every slot's prob plane alike.
// LDS: int tab[B][4] = (n, first canvas row, first canvas column, on) | int list[B] | float prof[S].
__global__ __launch_bounds__(SC_THREADS) void predict_blend_kernel(const float* __restrict__ prob, float scale,
                                                                   const float* __restrict__ profile,
                                                                   const int32_t* __restrict__ table, float* __restrict__ acc,
                                                                   float* __restrict__ wsum, int B, int N, int C, int S, int q, int Hc,
                                                                   int Wc) {
    extern __shared__ __attribute__((aligned(16))) int sc_lds[];
    int* tab = sc_lds;
    int* list = sc_lds + 4 * B;
    float* prof = reinterpret_cast<float*>(sc_lds + 5 * B);
    __shared__ int counts[2];                         // entries of `list`; how many of them are slots below this one
    const int tid = threadIdx.x, b = blockIdx.y;
    for (int i = tid; i < B; i += SC_THREADS) {
        int n, py, px;
        const bool ok = window_of(table, i, N, q, S, Hc, Wc, n, py, px) && table[4 * i + 3] != 0;
        tab[4 * i] = n;
        tab[4 * i + 1] = py;
        tab[4 * i + 2] = px;
        tab[4 * i + 3] = ok ? 1 : 0;
    }
    for (int i = tid; i < S; i += SC_THREADS) prof[i] = profile[i];
    __syncthreads();
    if (!tab[4 * b + 3]) return;                      // a pad slot (the whole workgroup leaves)
    const int n = tab[4 * b], py = tab[4 * b + 1], px = tab[4 * b + 2];
    if (tid < 64) {                                   // wave 0: the slots whose windows overlap this one, in ascending order
        int cnt = 0, lo = 0;
        for (int base = 0; base < B; base += 64) {
            const int s = base + tid;
            const bool hit = s < B && s != b && tab[4 * s + 3] && tab[4 * s] == n && abs(tab[4 * s + 1] - py) < S &&
                             abs(tab[4 * s + 2] - px) < S;
            const unsigned long long m = __ballot(hit);
            if (hit) list[cnt + __popcll(m & ((1ull << tid) - 1ull))] = s;
            cnt += __popcll(m);
            lo += __popcll(__ballot(hit && s < b));
        }
        if (tid == 0) { counts[0] = cnt; counts[1] = lo; }
    }
    __syncthreads();
    const int n_list = counts[0], n_lo = counts[1];
    const int n_win = S * S;
    const size_t plane = (size_t)n_win, cplane = (size_t)Hc * Wc;
    const int p_end = min(n_win, (int)(blockIdx.x + 1) * SC_PASSES * SC_THREADS);
    for (int p = blockIdx.x * SC_PASSES * SC_THREADS + tid; p < p_end; p += SC_THREADS) {
        const int y = p / S, x = p - y * S, Y = py + y, X = px + x;
        bool owner = true;
        for (int j = 0; j < n_lo && owner; ++j) {
            const int s = list[j];
            owner = (unsigned)(Y - tab[4 * s + 1]) >= (unsigned)S || (unsigned)(X - tab[4 * s + 2]) >= (unsigned)S;
        }
        if (!owner) continue;                         // a lower slot's thread sums this pixel
        const size_t pix = (size_t)Y * Wc + X;
        const float w0 = mul_rn(prof[y], prof[x]);
        float ws = add_rn(wsum[n * cplane + pix], w0);
        for (int j = n_lo; j < n_list; ++j) {
            const int s = list[j], dy = Y - tab[4 * s + 1], dx = X - tab[4 * s + 2];
            if ((unsigned)dy < (unsigned)S && (unsigned)dx < (unsigned)S) ws = add_rn(ws, mul_rn(prof[dy], prof[dx]));
        }
        wsum[n * cplane + pix] = ws;
        for (int c = 0; c < C; ++c) {
            float* a = acc + ((size_t)n * C + c) * cplane + pix;
            float v = add_rn(*a, mul_rn(mul_rn(prob[((size_t)b * C + c) * plane + p], scale), w0));
            for (int j = n_lo; j < n_list; ++j) {
                const int s = list[j], dy = Y - tab[4 * s + 1], dx = X - tab[4 * s + 2];
                if ((unsigned)dy < (unsigned)S && (unsigned)dx < (unsigned)S)
                    v = add_rn(v, mul_rn(mul_rn(prob[((size_t)s * C + c) * plane + (size_t)dy * S + dx], scale),
                                               mul_rn(prof[dy], prof[dx])));
            }
            *a = v;
        }
    }
}

// One canvas pixel per thread, coalesced over the pixels of a plane.  `mean` may be `acc`: a thread reads element c of its own
// pixel before it writes it, and nobody else touches that pixel.
__global__ __launch_bounds__(SC_THREADS) void predict_blend_finish_kernel(const float* acc, const float* __restrict__ wsum,
                                                                          uint8_t* __restrict__ cls, float* __restrict__ conf,
                                                                          float* mean, long n_items, int C, long n_pix) {
    for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < n_items; i += (long)gridDim.x * SC_THREADS) {
        const long n = i / n_pix, pix = i - n * n_pix;
        const size_t o = (size_t)n * C * n_pix + pix;
        const float w = wsum[i];
        if (w == 0.f) {                               // no window reached the pixel
            if (cls) cls[i] = MH_SCENE_UNCOVERED;
            if (conf) conf[i] = 0.f;
            if (mean)
                for (int c = 0; c < C; ++c) mean[o + (size_t)c * n_pix] = 0.f;
            continue;
        }
        float best;
        const int arg = argmax_torch(acc + o, C, (size_t)n_pix, best);
        if (cls) cls[i] = (uint8_t)arg;
        if (conf) conf[i] = __fdiv_rn(best, w);
        if (mean)
            for (int c = 0; c < C; ++c) mean[o + (size_t)c * n_pix] = __fdiv_rn(acc[o + (size_t)c * n_pix], w);
    }
}

// The host copy of the table, before any launch: 0, or the index of the first row that names no scene or leaves the raster + 1.
int bad_row(const int32_t* t, int B, int N, int q, int S, int H, int W) {
    for (int b = 0; b < B; ++b) {
        const long n = t[4 * b], y = (long)t[4 * b + 1] * q, x = (long)t[4 * b + 2] * q;
        if (n < 0 || n >= N || y < 0 || x < 0 || y + S > H || x + S > W) return b + 1;
    }
    return 0;
}

}  // namespace

extern "C" int mh_window_gather(const float* scene, float* out, const int32_t* table_dev, const int32_t* table_host, int B, int N,
                                int planes, int Hs, int Ws, int S, int q, void* stream) {
    MH_CHECK_ARG(scene && out, "mh_window_gather: null scene or out");
    MH_CHECK_ARG(table_dev && table_host, "mh_window_gather: null window table (device and host copies are both needed)");
    MH_CHECK_ARG(B > 0 && N > 0 && planes > 0, "mh_window_gather: B, N, planes must be positive (got %d, %d, %d)", B, N, planes);
    MH_CHECK_ARG(S > 0 && q > 0 && Hs > 0 && Ws > 0, "mh_window_gather: S, q, Hs, Ws must be positive (got %d, %d, %d, %d)", S, q, Hs, Ws);
    MH_CHECK_ARG(B <= MH_SCENE_MAX_SLOTS, "mh_window_gather: %d slots (at most %d)", B, MH_SCENE_MAX_SLOTS);
    MH_CHECK_ARG(S <= 46340 && (long)B * planes <= 0x7fffffffL, "mh_window_gather: S = %d or B * planes = %ld too large", S,
                 (long)B * planes);
    const int bad = bad_row(table_host, B, N, q, S, Hs, Ws);
    MH_CHECK_ARG(!bad, "mh_window_gather: slot %d = (scene %d, y0 %d, x0 %d) names no scene of %d or leaves the %d x %d raster "
                 "(q = %d, S = %d)", bad - 1, table_host[4 * (bad - 1)], table_host[4 * (bad - 1) + 1], table_host[4 * (bad - 1) + 2], N,
                 Hs, Ws, q, S);
    const bool vec = S % 4 == 0 && Ws % 4 == 0 && (uintptr_t)scene % 16 == 0 && (uintptr_t)out % 16 == 0;
    const long items = (long)S * (vec ? S / 4 : S);
    const dim3 grid((unsigned)(B * planes), (unsigned)min((items + SC_THREADS - 1) / SC_THREADS, (long)SC_MAX_CHUNKS));
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(window_gather_kernel<true>, grid, dim3(SC_THREADS), 0, s, scene, out, table_dev, N, planes, Hs, Ws, S, q);
    else
        hipLaunchKernelGGL(window_gather_kernel<false>, grid, dim3(SC_THREADS), 0, s, scene, out, table_dev, N, planes, Hs, Ws, S, q);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_predict_blend(const float* prob, float scale, const float* profile, const int32_t* table_dev,
                                const int32_t* table_host, float* acc, float* wsum, int B, int N, int C, int S, int q, int Hc, int Wc,
                                void* stream) {
    MH_CHECK_ARG(prob && profile && acc && wsum, "mh_predict_blend: null prob, profile, acc or wsum");
    MH_CHECK_ARG(table_dev && table_host, "mh_predict_blend: null window table (device and host copies are both needed)");
    MH_CHECK_ARG(B > 0 && N > 0, "mh_predict_blend: B, N must be positive (got %d, %d)", B, N);
    MH_CHECK_ARG(S > 0 && q > 0 && Hc > 0 && Wc > 0, "mh_predict_blend: S, q, Hc, Wc must be positive (got %d, %d, %d, %d)", S, q, Hc, Wc);
    MH_CHECK_ARG(C >= 2 && C <= 128, "mh_predict_blend: %d classes (2 ... 128 are supported)", C);
    MH_CHECK_ARG(B <= MH_SCENE_MAX_SLOTS && S <= MH_SCENE_MAX_S, "mh_predict_blend: B = %d (at most %d), S = %d (at most %d)", B,
                 MH_SCENE_MAX_SLOTS, S, MH_SCENE_MAX_S);
    MH_CHECK_ARG((long)Hc * Wc <= 46340L * 46340L, "mh_predict_blend: canvas %d x %d too large", Hc, Wc);
    MH_CHECK_ARG(scale > 0.f && scale <= 1.f, "mh_predict_blend: scale = %g (1 / the number of views)", (double)scale);
    const int bad = bad_row(table_host, B, N, q, S, Hc, Wc);
    MH_CHECK_ARG(!bad, "mh_predict_blend: slot %d = (scene %d, y0 %d, x0 %d) names no scene of %d or leaves the %d x %d canvas "
                 "(q = %d, S = %d)", bad - 1, table_host[4 * (bad - 1)], table_host[4 * (bad - 1) + 1], table_host[4 * (bad - 1) + 2], N,
                 Hc, Wc, q, S);
    const int per = SC_PASSES * SC_THREADS;
    const dim3 grid((unsigned)(((long)S * S + per - 1) / per), (unsigned)B);
    const size_t lds = (size_t)(5 * B + S) * 4;       // at most 36 KiB
    hipLaunchKernelGGL(predict_blend_kernel, grid, dim3(SC_THREADS), lds, (hipStream_t)stream, prob, scale, profile, table_dev, acc,
                       wsum, B, N, C, S, q, Hc, Wc);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_predict_blend_finish(const float* acc, const float* wsum, uint8_t* cls, float* conf, float* mean, int N, int C,
                                       long n_pix, void* stream) {
    MH_CHECK_ARG(acc && wsum, "mh_predict_blend_finish: null acc or wsum");
    MH_CHECK_ARG(cls || conf || mean, "mh_predict_blend_finish: no output (cls, conf and mean are all null)");
    MH_CHECK_ARG(N > 0 && n_pix > 0 && n_pix <= 46340L * 46340L, "mh_predict_blend_finish: N = %d, n_pix = %ld", N, n_pix);
    MH_CHECK_ARG(C >= 2 && C <= 128, "mh_predict_blend_finish: %d classes (2 ... 128 are supported)", C);
    const long n = (long)N * n_pix;
    hipLaunchKernelGGL(predict_blend_finish_kernel, dim3((unsigned)min((n + SC_THREADS - 1) / SC_THREADS, 4096L)), dim3(SC_THREADS), 0,
                       (hipStream_t)stream, acc, wsum, cls, conf, mean, n, C, n_pix);
    MH_LAUNCH_CHECK();
    return 0;
}
