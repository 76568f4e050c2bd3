// Masked reconstruction loss at patch layout + its gradient, bias-gradient column sums, casts.
#include "gemm_common.hpp"

namespace {

// rec/target f32 [T, PPC] (token rows of ONE modality: T = B * Lm); mask_group u8 [B, Lgroup]; token (b, t) of the
// modality sits at group position tok_off + t.  acc[0] += sum(e over masked), loss partial; drec (bf16) =
// coef * de/drec for masked tokens, 0 elsewhere, with coef = weight / (n_masked_tokens * PPC).
// One WAVE per token (4 tokens per block), 16-byte accesses; the block reduces its partial loss through LDS and issues one
// atomic (32768 -> 8192 atomics for the aerial modality; blocks whose 4 tokens are all visible issue none).
// DET (deterministic mode, mh_masked_loss_det): the same arithmetic, but the block's partial loss goes to acc[blockIdx.x]
// with a plain store instead of being added to the loss word.
// CS (step ends, mh_masked_loss_cs): the block also stores the column sums of the bf16 values it writes to drec -- the pixelify bias
// gradient -- to cs_partial[blockIdx.x, 0 .. PPC) (plain stores, zeros included), PPC <= 256 * LOSS_CS_NV.  A lane owns the same
// columns in every row, so the sums stay in registers until the block's four waves meet in LDS.
constexpr int LOSS_CS_NV = 4;
template <bool DET, bool CS = false>
__global__ __launch_bounds__(256) void masked_loss_kernel(const float* __restrict__ rec, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask_group, const int* __restrict__ n_masked,
                                                          float weight, float* __restrict__ acc, bf16_t* __restrict__ drec,
                                                          int B, int Lm, int Lgroup, int tok_off, int PPC, int p, int tgt_C,
                                                          int tgt_c0, int n_g, int denom_is_elems, int rows_per_wave,
                                                          float* __restrict__ cs_partial = nullptr) {
    // band window (several band-groups per modality): rec column k = pixel * n_g + c pairs with target column
    // pixel * tgt_C + tgt_c0 + c of the MODALITY's target rows (tgt_C channels); n_g == tgt_C: the plain case
    __shared__ float red[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float coef = weight / (denom_is_elems ? (float)(*n_masked) : (float)(*n_masked) * (float)PPC);
    const bool window = n_g != tgt_C;
    const int tgt_ld = window ? PPC / n_g * tgt_C : PPC;
    float s = 0.f;
    f32x4 cs[CS ? LOSS_CS_NV : 1];
#pragma unroll
    for (int j = 0; j < (CS ? LOSS_CS_NV : 1); ++j) cs[j] = (f32x4){0, 0, 0, 0};
    // several rows per wave: the block's ONE atomic into the loss word costs ~10 ns of serialised time (same-line atomics,
    // scripts/micro_amax.hip) -- 8192 blocks of 4 rows made the aerial modality's launch 80 us of atomics
    for (int rr = 0; rr < rows_per_wave; ++rr) {
        const int row = (blockIdx.x * 4 + w) * rows_per_wave + rr;
        if (row >= B * Lm) break;
        const int b = row / Lm, t = row - b * Lm;
        const bool masked = mask_group[(size_t)b * Lgroup + tok_off + t] != 0;
        const float* r = rec + (size_t)row * PPC;
        const float* g = target + (size_t)row * tgt_ld;
        bf16_t* d = drec ? drec + (size_t)row * PPC : nullptr;
        auto chunk = [&](int c, f32x4* colsum) {
            float dd[4] = {0.f, 0.f, 0.f, 0.f};
            if (masked) {
                const f32x4 rv = *reinterpret_cast<const f32x4*>(r + c);
                f32x4 tv;
                if (!window) {
                    tv = *reinterpret_cast<const f32x4*>(g + c);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const int pix = (c + e) / n_g; tv[e] = g[pix * tgt_C + tgt_c0 + (c + e) - pix * n_g]; }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float diff = rv[e] - tv[e];
                    if (p == 2) { s += diff * diff; dd[e] = 2.f * diff * coef; }
                    else { s += fabsf(diff); dd[e] = (diff > 0.f ? coef : (diff < 0.f ? -coef : 0.f)); }
                }
            }
            u32x2 pk = {pack_bf2(dd[0], dd[1]), pack_bf2(dd[2], dd[3])};
            if (d) *reinterpret_cast<u32x2*>(d + c) = pk;
            if (CS && masked) *colsum += bf2x2_to_f32x4(pk[0], pk[1]);
        };
        if constexpr (CS) {
#pragma unroll
            for (int j = 0; j < LOSS_CS_NV; ++j)
                if (lane * 4 + 256 * j < PPC) chunk(lane * 4 + 256 * j, &cs[j]);
        } else {
            for (int c = lane * 4; c < PPC; c += 256) chunk(c, nullptr);
        }
    }
    if constexpr (CS) {     // (the tail of mask.hip's gather_rows_bf16_cs_kernel: see the note there)
        __shared__ f32x4 csred[4][64 * LOSS_CS_NV];
#pragma unroll
        for (int j = 0; j < LOSS_CS_NV; ++j) csred[w][lane + 64 * j] = cs[j];
        __syncthreads();
        const float* cr = reinterpret_cast<const float*>(csred);
        for (int c = threadIdx.x; c < PPC; c += 256)
            cs_partial[(size_t)blockIdx.x * PPC + c] = (cr[c] + cr[256 * LOSS_CS_NV + c]) + (cr[512 * LOSS_CS_NV + c] + cr[768 * LOSS_CS_NV + c]);
    }
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = (red[0] + red[1]) + (red[2] + red[3]);
        if constexpr (DET) {     // zero is written too: every slot of the partial row is owned by one block
            acc[blockIdx.x] = (blockIdx.x == 0 && *n_masked == 0) ? __builtin_nanf("") : t * coef;
        } else {
        if (t != 0.f) atomicAdd(acc, t * coef);  // coef = weight / n_elems -> acc accumulates the weighted loss
        // a modality without a single masked token in the batch: the reference takes the mean of an empty selection
        // (maestro/train/model.py:241-243) -> NaN loss, zero gradient for this modality; reproduced, not guarded
        if (blockIdx.x == 0 && *n_masked == 0) atomicAdd(acc, __builtin_nanf(""));
        }
    }
}

// 1024 threads: 16 waves walk the block's rows side by side, 64 lanes x 4 columns each, eight row loads in flight per lane.  The
// launch is bound by two things that pull in opposite directions -- memory-level parallelism (wants many resident waves) and the
// same-address atomics of the final add (M / rows_per_block per column: wants few, fat blocks) -- so a block is 16 waves on up to
// 1024 rows: 32768 x 768 bf16 31.7 -> see scripts/bench_small_reductions.py.
// DET (mh_colsum_partial): row block blockIdx.y stores its sums to out[blockIdx.y, :] instead of adding them to out[:].
template <bool DET>
__global__ __launch_bounds__(1024) void colsum_kernel(const void* __restrict__ x, int is_f32, float* __restrict__ out, int M,
                                                      int N, int ld, int rows_per_block) {
    __shared__ f32x4 red[16][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    f32x4 acc = {0, 0, 0, 0};
    if (c < N) {
        // independent row loads, eight in flight per lane.  The element type is tested OUTSIDE the loops: with the test inside,
        // the two cases met in one accumulator after every load and the ISA waited `vmcnt(0)` per row (one round trip each).
        if (is_f32) {
#pragma unroll 8
            for (int r = r0 + w; r < r1; r += nw)
                acc += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x) + (size_t)r * ld + c);
        } else {
#pragma unroll 8
            for (int r = r0 + w; r < r1; r += nw) {
                const u32x2 pk = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(x) + (size_t)r * ld + c);
                acc += bf2x2_to_f32x4(pk[0], pk[1]);
            }
        }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < N) {
        f32x4 t = red[0][lane];
        for (int i = 1; i < nw; ++i) t += red[i][lane];
        if constexpr (DET) {
            *reinterpret_cast<f32x4*>(out + (size_t)blockIdx.y * N + c) = t;
        } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(out + c + e, t[e]);
        }
    }
}

// zero a list of (offset, length) float spans of one buffer: blockIdx.y = span, blockIdx.x walks it in 1024-float pieces
__global__ __launch_bounds__(256) void zero_spans_kernel(float* __restrict__ base, const long* __restrict__ spans) {
    const long off = spans[2 * blockIdx.y], len = spans[2 * blockIdx.y + 1];
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < len; i += (long)gridDim.x * 1024) {
        float* p = base + off + i;
        if (i + 3 < len && (reinterpret_cast<uintptr_t>(p) & 15) == 0) *reinterpret_cast<f32x4*>(p) = (f32x4){0, 0, 0, 0};
        else for (long e = i; e < min(len, i + 4); ++e) base[off + e] = 0.f;
    }
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        u32x2 pk = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *reinterpret_cast<u32x2*>(dst + i) = pk;
    } else {
        for (long j = i; j < n; ++j) dst[j] = f2bf(src[j]);
    }
}

__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int E, int K, int Kpad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)E * Kpad) return;
    const int e = i / Kpad, k = i - (long)e * Kpad;
    dst[i] = k < K ? f2bf(w[(size_t)e * K + k]) : (bf16_t)0;
}

__global__ __launch_bounds__(256) void unpack_rows_add_kernel(const float* __restrict__ src, float* __restrict__ dst, int E, int K, int Kpad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)E * K) return;
    const int e = i / K, k = i - (long)e * K;
    atomicAdd(dst + i, src[(size_t)e * Kpad + k]);  // shared patch-embed weights may be updated from parallel streams
}

// x *= *scale, skipped when the device scalar is exactly 1 (loss.backward() with autograd's default ones gradient): the
// Lightning bridge scales the flat gradient buffer by d loss without reading the scalar on the host.
__global__ __launch_bounds__(256) void scale_dev_kernel(float* __restrict__ x, long n, const float* __restrict__ scale) {
    const float s = *scale;
    if (s == 1.f) return;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 4 <= n) {
        *reinterpret_cast<f32x4*>(x + i) = *reinterpret_cast<const f32x4*>(x + i) * s;
    } else {
        for (long j = i; j < n; ++j) x[j] *= s;
    }
}

}  // namespace

// rows per wave of masked_loss_kernel: about 1024 workgroups (= same-word atomics) per launch, at most 16 rows per wave
static int loss_rows_per_wave(long rows) { return (int)std::min(16L, std::max(1L, rows / 4096)); }

extern "C" int mh_scale_dev(float* x, long n, const float* scale, void* stream) {
    MH_CHECK_ARG(x && scale && n > 0 && ((uintptr_t)x % 16) == 0, "mh_scale_dev: bad arguments (x 16-byte aligned)");
    hipLaunchKernelGGL(scale_dev_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, x, n, scale);
    MH_LAUNCH_CHECK();
    return 0;
}

// Host side of the six masked-loss entries over masked_loss_kernel<DET, CS>: the shared checks, rows per wave, grid and launch.
// ``name``: the entry's own name, for its messages.  ``pointers``: the entry's required pointers are all there.  ``ppc_cap``: > 0 in
// the CS entries (a lane keeps its columns' sums in registers).  ``window`` = {tgt_C, tgt_c0, n_g}: the band window of the *_bands
// entries, whose denominator counts elements; nullptr: the plain case.  The entries younger than the first two also refuse B, Lm <= 0.
template <bool DET, bool CS>
static int launch_masked_loss(const char* name, bool pointers, int ppc_cap, const int* window, const float* rec, const float* target,
                              const uint8_t* mask_group, const int* n_masked, float weight, float* acc, void* drec, float* cs_partial,
                              int B, int Lm, int Lgroup, int tok_off, int PPC, int p, void* stream) {
    MH_CHECK_ARG(pointers, "%s: null pointer", name);
    const bool ok = ((!DET && !CS) || (B > 0 && Lm > 0)) && (p == 1 || p == 2) && PPC % 4 == 0 && tok_off + Lm <= Lgroup;
    if (ppc_cap > 0)
        MH_CHECK_ARG(ok && PPC > 0 && PPC <= ppc_cap && tok_off >= 0, "%s: bad arguments (PPC %% 4 == 0, PPC <= %d)", name, ppc_cap);
    MH_CHECK_ARG(ok, "%s: bad arguments", name);
    const int tgt_C = window ? window[0] : 1, tgt_c0 = window ? window[1] : 0, n_g = window ? window[2] : 1;
    MH_CHECK_ARG(n_g > 0 && PPC % n_g == 0 && tgt_c0 >= 0 && tgt_c0 + n_g <= tgt_C, "%s: band window [%d, %d) of %d", name, tgt_c0,
                 tgt_c0 + n_g, tgt_C);
    const int rpw = loss_rows_per_wave((long)B * Lm);
    hipLaunchKernelGGL((masked_loss_kernel<DET, CS>), dim3(ceil_div((long)B * Lm, 4 * rpw)), dim3(256), 0, (hipStream_t)stream, rec, target,
                       mask_group, n_masked, weight, acc, (bf16_t*)drec, B, Lm, Lgroup, tok_off, PPC, p, tgt_C, tgt_c0, n_g, window ? 1 : 0,
                       rpw, cs_partial);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_masked_loss(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked,
                              float weight, float* acc, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                              void* stream) {
    return launch_masked_loss<false, false>("mh_masked_loss", rec && target && mask_group && n_masked && acc, 0, nullptr, rec, target,
                                            mask_group, n_masked, weight, acc, drec, nullptr, B, Lm, Lgroup, tok_off, PPC, p, stream);
}

extern "C" int mh_masked_loss_bands(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems,
                                    float weight, float* acc, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                                    int tgt_C, int tgt_c0, int n_g, void* stream) {
    const int window[3] = {tgt_C, tgt_c0, n_g};
    return launch_masked_loss<false, false>("mh_masked_loss_bands", rec && target && mask_group && n_elems && acc, 0, window, rec, target,
                                            mask_group, n_elems, weight, acc, drec, nullptr, B, Lm, Lgroup, tok_off, PPC, p, stream);
}

extern "C" int mh_masked_loss_partial_size(int B, int Lm) {
    const long rows = (long)B * Lm;
    return rows > 0 ? ceil_div(rows, 4 * loss_rows_per_wave(rows)) : 0;
}

extern "C" int mh_masked_loss_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked,
                                  float weight, float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC,
                                  int p, void* stream) {
    return launch_masked_loss<true, false>("mh_masked_loss_det", rec && target && mask_group && n_masked && loss_partial, 0, nullptr, rec,
                                           target, mask_group, n_masked, weight, loss_partial, drec, nullptr, B, Lm, Lgroup, tok_off, PPC,
                                           p, stream);
}

extern "C" int mh_masked_loss_bands_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems,
                                        float weight, float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off,
                                        int PPC, int p, int tgt_C, int tgt_c0, int n_g, void* stream) {
    const int window[3] = {tgt_C, tgt_c0, n_g};
    return launch_masked_loss<true, false>("mh_masked_loss_bands_det", rec && target && mask_group && n_elems && loss_partial, 0, window,
                                           rec, target, mask_group, n_elems, weight, loss_partial, drec, nullptr, B, Lm, Lgroup, tok_off,
                                           PPC, p, stream);
}

extern "C" int mh_masked_loss_cs_rows(int B, int Lm) { return mh_masked_loss_partial_size(B, Lm); }

extern "C" int mh_masked_loss_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                                 float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                                 void* stream) {
    return launch_masked_loss<false, true>("mh_masked_loss_cs", rec && target && mask_group && n_masked && acc && drec && cs_partial,
                                           256 * LOSS_CS_NV, nullptr, rec, target, mask_group, n_masked, weight, acc, drec, cs_partial, B,
                                           Lm, Lgroup, tok_off, PPC, p, stream);
}

extern "C" int mh_masked_loss_bands_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems,
                                       float weight, float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off,
                                       int PPC, int p, int tgt_C, int tgt_c0, int n_g, void* stream) {
    const int window[3] = {tgt_C, tgt_c0, n_g};
    return launch_masked_loss<false, true>("mh_masked_loss_bands_cs", rec && target && mask_group && n_elems && acc && drec && cs_partial,
                                           256 * LOSS_CS_NV, window, rec, target, mask_group, n_elems, weight, acc, drec, cs_partial, B,
                                           Lm, Lgroup, tok_off, PPC, p, stream);
}

extern "C" int mh_colsum_partial_rows(int M) { return M > 0 ? ceil_div(M, MH_COLSUM_PARTIAL_ROWS) : 0; }

extern "C" int mh_colsum_partial(const void* x, int x_is_f32, float* partial, int M, int N, int ld, void* stream) {
    MH_CHECK_ARG(x && partial && ((uintptr_t)partial % 16) == 0, "mh_colsum_partial: null pointer / partial not 16-byte aligned");
    MH_CHECK_ARG(M > 0 && N > 0 && N % 4 == 0 && ld % 4 == 0 && N <= ld, "mh_colsum_partial: bad sizes M=%d N=%d ld=%d", M, N, ld);
    hipLaunchKernelGGL(colsum_kernel<true>, dim3(ceil_div(N, 256), ceil_div(M, MH_COLSUM_PARTIAL_ROWS)), dim3(1024), 0,
                       (hipStream_t)stream, x, x_is_f32, partial, M, N, ld, MH_COLSUM_PARTIAL_ROWS);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_colsum(const void* x, int x_is_f32, float* out, int M, int N, int ld, void* stream) {
    MH_CHECK_ARG(x && out && N % 4 == 0 && ld % 4 == 0, "mh_colsum: bad arguments");
    // up to 1024 rows per 16-wave block; fewer when that would leave most CUs without a block
    const int col_blocks = ceil_div(N, 256);
    int rows_per_block = 1024;
    while (rows_per_block > 128 && (long)col_blocks * ceil_div(M, rows_per_block) < 128) rows_per_block >>= 1;
    hipLaunchKernelGGL(colsum_kernel<false>, dim3(col_blocks, ceil_div(M, rows_per_block)), dim3(1024), 0, (hipStream_t)stream, x,
                       x_is_f32, out, M, N, ld, rows_per_block);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_zero_spans(float* base, const long* spans_device, int n_spans, long max_len, void* stream) {
    MH_CHECK_ARG(base && spans_device && n_spans > 0 && max_len > 0, "mh_zero_spans: bad arguments");
    dim3 grid((unsigned)min(64L, (max_len + 1023) / 1024), n_spans);
    hipLaunchKernelGGL(zero_spans_kernel, grid, dim3(256), 0, (hipStream_t)stream, base, spans_device);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_cast_bf16(const float* src, void* dst, long n, void* stream) {
    MH_CHECK_ARG(src && dst && n > 0, "mh_cast_bf16: bad arguments");
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_pack_rows_bf16(const float* w, void* dst, int E, int K, int Kpad, void* stream) {
    MH_CHECK_ARG(w && dst && Kpad >= K, "mh_pack_rows_bf16: bad arguments");
    hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div((long)E * Kpad, 256)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)dst, E, K, Kpad);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_unpack_rows_add(const float* src, float* dst, int E, int K, int Kpad, void* stream) {
    MH_CHECK_ARG(src && dst && Kpad >= K, "mh_unpack_rows_add: bad arguments");
    hipLaunchKernelGGL(unpack_rows_add_kernel, dim3(ceil_div((long)E * K, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, E, K, Kpad);
    MH_LAUNCH_CHECK();
    return 0;
}
