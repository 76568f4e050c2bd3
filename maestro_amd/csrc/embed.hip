// Patch extraction, target normalisation, patch-embed GroupNorm (+ encodings) forward/backward.
// See include/maestro_hip.h for the reference lines each entry point replaces.  All HBM-bound: coalesced row reads,
// LDS transposes where the output order differs from the input order, wavefront reductions for statistics.
#include "common.hpp"
#include "reduce_det.hpp"
#include "../../include/maestro_hip.h"

namespace {

// Generic block reduction for blockDim.x in {64, 128, 256}.
__device__ __forceinline__ float block_sum_any(float v, float* red) {
    v = wave_sum(v);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// One block per patch (token).  LDS holds the patch in TARGET order [(p1*P+p2)*Ctot + c].
// Band windows (several band-groups per modality, maestro/layers/embed.py:18-34): the image has Csrc channels, the patch takes
// channels c0 .. c0 + Ctot - 1 of it; the elevation rescale always refers to channel 0 of the IMAGE.
__global__ void patchify_kernel(const float* __restrict__ img, bf16_t* __restrict__ cols, float* __restrict__ target,
                                int Csrc, int c0, int Ctot, int S, int P, int Kpad, const int* __restrict__ norm_bands,
                                int n_groups, int normalise, int rescale_elev) {
    extern __shared__ __attribute__((aligned(16))) float patch[];  // P*P*Ctot floats + 8 reduction slots
    const int g = S / P;
    const int tok = blockIdx.x;  // (bd, ph, pw)
    const int bd = tok / (g * g), pp = tok - bd * g * g, ph = pp / g, pw = pp - ph * g;
    const int PP = P * P, K = Ctot * PP;
    float* red = patch + K;
    const float* base0 = img + ((size_t)bd * Csrc) * S * S + (size_t)(ph * P) * S + pw * P;   // channel 0 of the image
    const float* base = base0 + (size_t)c0 * S * S;
    if ((P & 3) == 0 && (Kpad & 3) == 0) {
        // four consecutive pixels of one patch row per thread: 16-byte image loads, 8-byte bf16 stores
        for (int k = threadIdx.x * 4; k < Kpad; k += blockDim.x * 4) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < K) {
                const int c = k / PP, r = k - c * PP, p1 = r / P, p2 = r - p1 * P;
                v = *reinterpret_cast<const f32x4*>(base + (size_t)c * S * S + p1 * S + p2);
                if (rescale_elev && c0 + c >= 1) v = 30.f * (*reinterpret_cast<const f32x4*>(base0 + p1 * S + p2) - v);
#pragma unroll
                for (int e = 0; e < 4; ++e) patch[(r + e) * Ctot + c] = v[e];
            }
            if (cols) {
                u32x2 pk = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
                *reinterpret_cast<u32x2*>(cols + (size_t)tok * Kpad + k) = pk;
            }
        }
    } else {
        for (int k = threadIdx.x; k < Kpad; k += blockDim.x) {
            float v = 0.f;
            if (k < K) {
                const int c = k / PP, r = k - c * PP, p1 = r / P, p2 = r - p1 * P;
                v = base[(size_t)c * S * S + p1 * S + p2];
                if (rescale_elev && c0 + c >= 1) v = 30.f * (base0[p1 * S + p2] - v);
                patch[r * Ctot + c] = v;
            }
            if (cols) cols[(size_t)tok * Kpad + k] = f2bf(v);
        }
    }
    if (!target) return;
    __syncthreads();
    float* out = target + (size_t)tok * K;
    if (!normalise) {
        for (int e = threadIdx.x; e < K; e += blockDim.x) out[e] = patch[e];
        return;
    }
    // patch-group-wise statistics: unbiased variance, eps 1e-6 (reference model.py:226-229), two-pass; a thread owns whole
    // pixels of the group (no per-element div / mod)
    int c_lo = 0;
    for (int gi = 0; gi < n_groups; ++gi) {
        const int cg = norm_bands[gi], n = cg * PP;
        float s = 0.f;
        for (int pix = threadIdx.x; pix < PP; pix += blockDim.x)
            for (int cc = 0; cc < cg; ++cc) s += patch[pix * Ctot + c_lo + cc];
        const float mu = block_sum_any(s, red) / n;
        float q = 0.f;
        for (int pix = threadIdx.x; pix < PP; pix += blockDim.x)
            for (int cc = 0; cc < cg; ++cc) {
                const float d = patch[pix * Ctot + c_lo + cc] - mu;
                q += d * d;
            }
        const float var = block_sum_any(q, red) / (n - 1);
        const float inv = 1.f / sqrtf(var + 1.0e-6f);
        for (int pix = threadIdx.x; pix < PP; pix += blockDim.x)
            for (int cc = 0; cc < cg; ++cc) {
                const int idx = pix * Ctot + c_lo + cc;
                out[idx] = (patch[idx] - mu) * inv;
            }
        c_lo += cg;
    }
}

// P = 16 patches (aerial / spot rasters: 1024 x C elements per token), ONE WAVE per patch, no LDS, no barriers: lane l owns the four
// consecutive pixels (row l >> 2, columns 4 (l & 3) ..) of the patch in every channel, i.e. one 16-byte image load per channel,
// one 8-byte store per channel into the K-ordered bf16 columns (a wave writes 512 contiguous bytes) and -- because a lane holds
// ALL channels of its pixels -- 16 CT contiguous bytes of the pixel-major fp32 target (a wave writes the patch's 4 CT KiB in one
// run).  The patch-group statistics are two wave reductions per group.  The block-per-patch kernel above (LDS transpose, four
// block reductions = eight barriers per 4 KiB patch) ran at 2.0 TB/s on the C3 aerial launch (335 MB in 165 us).
template <int CT>
__global__ __launch_bounds__(256) void patchify_wave16_kernel(const float* __restrict__ img, bf16_t* __restrict__ cols,
                                                              float* __restrict__ target, int Csrc, int c0, int S, int Kpad,
                                                              const int* __restrict__ norm_bands, int n_groups, int normalise,
                                                              int rescale_elev, int n_tok) {
    constexpr int P = 16, PP = 256, K = CT * PP;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (tok >= n_tok) return;
    const int g = S / P;
    const int bd = tok / (g * g), pp = tok - bd * g * g, ph = pp / g, pw = pp - ph * g;
    const int p1 = l >> 2, p2 = (l & 3) * 4;
    const size_t plane = (size_t)S * S;
    const float* base0 = img + (size_t)bd * Csrc * plane + (size_t)(ph * P + p1) * S + pw * P + p2;   // channel 0 of the image
    f32x4 v[CT];
    f32x4 elev = {0.f, 0.f, 0.f, 0.f};
    if (rescale_elev) elev = *reinterpret_cast<const f32x4*>(base0);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        v[c] = *reinterpret_cast<const f32x4*>(base0 + (size_t)(c0 + c) * plane);
        if (rescale_elev && c0 + c >= 1) v[c] = 30.f * (elev - v[c]);
    }
    if (cols) {
        bf16_t* crow = cols + (size_t)tok * Kpad;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const u32x2 pk = {pack_bf2(v[c][0], v[c][1]), pack_bf2(v[c][2], v[c][3])};
            *reinterpret_cast<u32x2*>(crow + c * PP + 4 * l) = pk;
        }
        for (int k = K + 4 * l; k < Kpad; k += 256) *reinterpret_cast<u32x2*>(crow + k) = (u32x2){0u, 0u};   // K padding
    }
    if (!target) return;
    if (normalise) {   // patch-group-wise statistics: unbiased variance, eps 1e-6 (reference model.py:226-229), two-pass
        int c_lo = 0;
        for (int gi = 0; gi < n_groups; ++gi) {
            const int cg = norm_bands[gi], n = cg * PP;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c >= c_lo && c < c_lo + cg) s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
            const float mu = wave_sum(s) / n;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c >= c_lo && c < c_lo + cg) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float d = v[c][e] - mu; q += d * d; }
                }
            const float inv = 1.f / sqrtf(wave_sum(q) / (n - 1) + 1.0e-6f);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c >= c_lo && c < c_lo + cg) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[c][e] = (v[c][e] - mu) * inv;
                }
            c_lo += cg;
        }
    }
    float t[4 * CT];   // the lane's four pixels, channel-minor: element (4 l + e) * CT + c of the patch
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < CT; ++c) t[e * CT + c] = v[c][e];
    float* out = target + (size_t)tok * K + (size_t)l * 4 * CT;
#pragma unroll
    for (int i = 0; i < CT; ++i) *reinterpret_cast<f32x4*>(out + 4 * i) = (f32x4){t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]};
}

// ---- GroupNorm(1, E) statistics over a whole (L x E) image: per-chunk (sum, centred sum of squares), then a finalize.
// A chunk is 32 values per thread and stays in registers, so it is reduced in two passes: its fp32 sum s first, then the sum q of
// (x - m)^2 around m = s / n_c.  The finalize merges the chunks in fp64 with the exact expansion
//   sum (x - mu)^2 = sum_c [ q_c + 2 (m_c - mu) (s_c - n_c m_c) + n_c (m_c - mu)^2 ],   mu = sum_c s_c / n,
// recomputing m_c = s_c / n_c with the same fp32 division, so the centre it assumes is bit for bit the one the chunk used.
// The earlier form kept fp32 sums of x and x^2 per chunk: E[x^2] - E[x]^2 cancels, and the variance of an image whose mean is
// 100 sigma was off by 3e-4 relative, at 1000 sigma by 5e-2.  (Sums shifted by a per-image pivot cure that too, but their mean is
// only as good as the pivot is close to it: on zero-mean images they are worse than plain sums.  A chunk centred on its own mean
// has no such case, and the mean itself is the same sum of chunk sums as before.)
constexpr int GN_CHUNK = 8192;

__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ y, float* __restrict__ partial,
                                                         long per_image, int nchunk) {
    __shared__ float red[8];
    constexpr int NV = GN_CHUNK / (256 * 4);
    const int bd = blockIdx.y, ch = blockIdx.x;
    const float* p = y + (size_t)bd * per_image;
    const long lo = (long)ch * GN_CHUNK, hi = min(per_image, lo + GN_CHUNK);
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long i = lo + (long)(j * 256 + threadIdx.x) * 4;
        v[j] = i < hi ? *reinterpret_cast<const f32x4*>(p + i) : (f32x4){0, 0, 0, 0};
        s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
    s = block_sum<4>(s, red);
    const float m = s / (float)(hi - lo);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (lo + (long)(j * 256 + threadIdx.x) * 4 < hi) {
            const f32x4 d = v[j] - m;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    q = block_sum<4>(q, red + 4);
    if (threadIdx.x == 0) {
        partial[((size_t)bd * nchunk + ch) * 2] = s;
        partial[((size_t)bd * nchunk + ch) * 2 + 1] = q;
    }
}

__global__ __launch_bounds__(64) void gn_finalize_kernel(const float* __restrict__ partial, float* __restrict__ stats,
                                                         long per_image, int nchunk, float eps) {
    const int bd = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nchunk; i += 64) s += partial[((size_t)bd * nchunk + i) * 2];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const double mu = s / per_image;                       // (the butterfly leaves the same sum in every lane)
    double q = 0.0;
    for (int i = threadIdx.x; i < nchunk; i += 64) {
        const float sc = partial[((size_t)bd * nchunk + i) * 2];
        const float nc = (float)min((long)GN_CHUNK, per_image - (long)i * GN_CHUNK);
        const float mc = sc / nc;                          // the centre gn_partial_kernel used for this chunk
        const double dm = (double)mc - mu;
        q += partial[((size_t)bd * nchunk + i) * 2 + 1] + dm * (2.0 * ((double)sc - (double)nc * mc) + (double)nc * dm);
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    if (threadIdx.x == 0) {
        const double var = fmax(q / per_image, 0.0);
        stats[bd * 2] = (float)mu;
        stats[bd * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// ---- normalise + affine + positional + date encodings, written into the group sequence. One wave per token.
__global__ __launch_bounds__(256) void embed_finish_kernel(const float* __restrict__ y, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ pos, const float* __restrict__ date,
                                                           float* __restrict__ xg, int B, int D, int L, int E, int tok_off,
                                                           int Lgroup, int date_rows, int date_off) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * D * L) return;
    const int bd = row / L, l = row - bd * L, b = bd / D, d = bd - b * D;
    const float mu = stats[bd * 2], rs = stats[bd * 2 + 1];
    const float* yr = y + (size_t)row * E;
    float* o = xg + ((size_t)b * Lgroup + tok_off + d * L + l) * E;
    const float* pr = pos + (size_t)l * E;
    const float* dr = date ? date + ((size_t)b * date_rows + date_off + d) * 8 : nullptr;
    for (int c = lane * 4; c < E; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(yr + c);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + c);
        const f32x4 ps = *reinterpret_cast<const f32x4*>(pr + c);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (v[e] - mu) * rs * g[e] + bt[e] + ps[e];
        if (dr && c >= E - 8) r += *reinterpret_cast<const f32x4*>(dr + (c - (E - 8)));
        *reinterpret_cast<f32x4*>(o + c) = r;
    }
}

// ---- GroupNorm backward of the patch embed, two passes (launch_embed_bwd).  Both keep a row's columns in registers: NV =
// ceil(E / 256) four-column chunks per lane, a lane owns the same columns in every row of its wave.
// WIDE (E > 1024, the plain and deterministic entry points only; no model size is that wide): the same body once per pass of
// 256 NV = 1024 columns.
// MAP (mh_embed_finish_bwd_ends): dxg is the gradient of the VISIBLE rows [B, n_vis, E] and inv [B, Lgroup] maps a group position
// to its visible row (< 0: masked = a zero gradient).

// ---- pass 1: per image S1 = sum(dz), S2 = sum(dz*z); dgamma/dbeta (atomic). EB_ROWS tokens per wave.
// The dgamma / dbeta partial sums of a wave's EB_ROWS rows stay in registers and touch LDS once at the end (round 6; they used to be
// read-modify-written in LDS for every element: two LDS round trips per element in a kernel that streams 8 bytes per element from
// HBM).  WIDE: a lane adds its S1 / S2 terms pass by pass, i.e. columns outermost; the per-column sums keep their order.
// DET (deterministic mode, mh_embed_finish_bwd_det): no atomics -- the block writes its (S1, S2) to sums[bd, blockIdx.x, 2] and its
// dgamma | dbeta row to dgamma[(bd * gridDim.x + blockIdx.x), 2 E] (dbeta unused); LDS then carries 8 more floats for the waves' sums.
// MAP: a masked row adds nothing to any of the sums: the wave skips it (the branch is wave-uniform) and issues none of its loads.
constexpr int EB_ROWS = 8;
template <int NV, bool DET, bool MAP, bool WIDE = false>
__global__ __launch_bounds__(256) void embed_bwd_stats_kernel(const float* __restrict__ dxg, const float* __restrict__ y,
                                                              const float* __restrict__ stats, const float* __restrict__ gamma,
                                                              float* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int B, int D, int L, int E,
                                                              int tok_off, int Lgroup, const int* __restrict__ inv, int n_vis) {
    static_assert(!WIDE || (NV == 4 && !MAP), "column passes: full-width ones, without the position map");
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4][2][P]; DET: + the waves' [4][2] (S1, S2)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bd = blockIdx.y, b = bd / D, d = bd - b * D;
    const float mu = stats[bd * 2], rs = stats[bd * 2 + 1];
    const int P = WIDE ? 256 * NV : E;           // a pass's columns = the pitch of the LDS rows
    float* rg = red + (size_t)w * 2 * P;         // (a fixed pitch, so that this stays in front of the loop: the !WIDE forms then compile
                                                 //  to the instructions they had without it)
    float s1 = 0.f, s2 = 0.f;
    const int l0 = (blockIdx.x * 4 + w) * EB_ROWS;
    int c0 = 0;
    do {                                         // columns c0 .. c0 + W of every row; !WIDE: the one pass, W = E
        const int W = WIDE ? min(E - c0, P) : E;
        f32x4 gz[NV], gd[NV], gm[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane * 4 + 256 * j;
            gz[j] = (f32x4){0, 0, 0, 0}; gd[j] = (f32x4){0, 0, 0, 0};
            gm[j] = c < W ? *reinterpret_cast<const f32x4*>(gamma + c0 + c) : (f32x4){0, 0, 0, 0};
        }
#pragma unroll 2
        for (int rr = 0; rr < EB_ROWS; ++rr) {
            const int l = l0 + rr;
            if (l >= L) break;
            const float* yr = y + ((size_t)bd * L + l) * E + c0;
            const float* gr = dxg + ((size_t)b * Lgroup + tok_off + d * L + l) * E + c0;
            if constexpr (MAP) {
                const int iv = inv[(size_t)b * Lgroup + tok_off + d * L + l];
                if (iv < 0) continue;
                gr = dxg + ((size_t)b * n_vis + iv) * E;
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = lane * 4 + 256 * j;
                if (c < W) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(yr + c);
                    const f32x4 dd = *reinterpret_cast<const f32x4*>(gr + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = (v[e] - mu) * rs, dz = dd[e] * gm[j][e];
                        s1 += dz; s2 += dz * z;
                        gz[j][e] += dd[e] * z;
                        gd[j][e] += dd[e];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane * 4 + 256 * j;
            if (c < W) {
                *reinterpret_cast<f32x4*>(rg + c) = gz[j];
                *reinterpret_cast<f32x4*>(rg + P + c) = gd[j];
            }
        }
        if (!WIDE || c0 + 256 * NV >= E) {       // the last pass: the lane's S1, S2 are complete
            s1 = wave_sum(s1); s2 = wave_sum(s2);
            if constexpr (DET) {
                if (lane == 0) { red[8 * P + 2 * w] = s1; red[8 * P + 2 * w + 1] = s2; }
            } else {
            if (lane == 0) { atomicAdd(sums + bd * 2, s1); atomicAdd(sums + bd * 2 + 1, s2); }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < 2 * W; c += 256) {
            const int i = WIDE && c >= W ? P + (c - W) : c;                  // of a wave's dgamma[0 .. P) | dbeta[0 .. P) in LDS
            const float t = red[i] + red[2 * P + i] + red[4 * P + i] + red[6 * P + i];
            const int col = WIDE ? c0 + (c < W ? c : E + (c - W)) : c;      // of the row dgamma[0 .. E) | dbeta[0 .. E)
            if constexpr (DET) {
                dgamma[((size_t)bd * gridDim.x + blockIdx.x) * 2 * E + col] = t;
            } else {
            if (col < E) atomicAdd(dgamma + col, t); else atomicAdd(dbeta + (col - E), t);
            }
        }
        if constexpr (WIDE) __syncthreads();     // (the next pass overwrites the waves' rows)
    } while (WIDE && (c0 += 256 * NV) < E);
    if constexpr (DET) {
        if (threadIdx.x < 2) {
            const float* ws = red + 8 * P + threadIdx.x;
            sums[((size_t)bd * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = ((ws[0] + ws[2]) + ws[4]) + ws[6];
        }
    }
}

// deterministic mode: sums[bd, k] = the ordered sum (reduce_det.hpp) of blk_sums[bd, 0 .. nblk, k]; one thread per output
__global__ __launch_bounds__(64) void embed_bwd_sums_det_kernel(const float* __restrict__ blk_sums, float* __restrict__ sums, int nblk) {
    if (threadIdx.x < 2)
        sums[blockIdx.x * 2 + threadIdx.x] = 0.f + ordered_job_total(blk_sums + (size_t)blockIdx.x * nblk * 2 + threadIdx.x, nblk, 2);
}

__global__ __launch_bounds__(256) void zero_f32_kernel(float* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// ---- pass 2: dy = rstd * (dz - S1/n - z*S2/n) as bf16 (A operand of the patch-embed wgrad GEMM).
// Rows per wave: EA_ROWS where the column sums want them, one otherwise -- with eight, the plain and deterministic calls took 1 - 5 us
// longer at all three shapes of scripts/bench_embed_bwd.py (profiles/embed_bwd_unify.md: fewer, fatter workgroups for a pass that
// only streams).
// CS (mh_embed_finish_bwd_ends): with the conv bias gradient -- the column sums of the bf16 values a lane stores stay in its
// registers; the block's four waves meet in LDS and store one partial row.
// MAP: a masked row is a zero gradient -- its dyc row still depends on yconv -- and its gradient loads are skipped.
constexpr int EA_ROWS = 8;
template <int NV, bool MAP, bool CS, bool WIDE = false>
__global__ __launch_bounds__(256) void embed_bwd_apply_kernel(const float* __restrict__ dxg, const int* __restrict__ inv, int n_vis,
                                                              const float* __restrict__ y, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ sums,
                                                              bf16_t* __restrict__ dyc, float* __restrict__ cs_partial,
                                                              int B, int D, int L, int E, int tok_off, int Lgroup) {
    static_assert(!WIDE || (NV == 4 && !MAP && !CS), "column passes: full-width ones, without the position map or the column sums");
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int ROWS = CS ? EA_ROWS : 1;
    const long rows = (long)B * D * L, row0 = ((long)blockIdx.x * 4 + w) * ROWS;
    const float n = (float)L * (float)E;
    f32x4 cs[NV];
    int c0 = 0;
    do {                                         // columns c0 .. of every row; !WIDE: the one pass
        f32x4 gm[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = c0 + lane * 4 + 256 * j;
            cs[j] = (f32x4){0, 0, 0, 0};
            gm[j] = c < E ? *reinterpret_cast<const f32x4*>(gamma + c) : (f32x4){0, 0, 0, 0};
        }
#pragma unroll 2
        for (int rr = 0; rr < ROWS; ++rr) {
            const long row = row0 + rr;
            if (row >= rows) break;
            const int bd = (int)(row / L), l = (int)(row - (long)bd * L), b = bd / D, d = bd - b * D;
            const float mu = stats[bd * 2], rs = stats[bd * 2 + 1];
            const float c1 = sums[bd * 2] / n, c2 = sums[bd * 2 + 1] / n;
            const float* yr = y + (size_t)row * E;
            const float* gr = dxg + ((size_t)b * Lgroup + tok_off + d * L + l) * E;
            bool vis = true;
            if constexpr (MAP) {
                const int iv = inv[(size_t)b * Lgroup + tok_off + d * L + l];
                vis = iv >= 0;
                gr = dxg + ((size_t)b * n_vis + (vis ? iv : 0)) * E;
            }
            bf16_t* o = dyc + (size_t)row * E;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = c0 + lane * 4 + 256 * j;
                if (c < E) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(yr + c);
                    f32x4 dd = {0.f, 0.f, 0.f, 0.f};
                    if (vis) dd = *reinterpret_cast<const f32x4*>(gr + c);
                    float r[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = (v[e] - mu) * rs;
                        r[e] = rs * (dd[e] * gm[j][e] - c1 - z * c2);
                    }
                    const u32x2 pk = {pack_bf2(r[0], r[1]), pack_bf2(r[2], r[3])};
                    *reinterpret_cast<u32x2*>(o + c) = pk;
                    if constexpr (CS) cs[j] += bf2x2_to_f32x4(pk[0], pk[1]);
                }
            }
        }
    } while (WIDE && (c0 += 256 * NV) < E);
    if constexpr (CS) {     // (the tail of mask.hip's gather_rows_bf16_cs_kernel: see the note there)
        __shared__ f32x4 red[4][64 * NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) red[w][lane + 64 * j] = cs[j];
        __syncthreads();
        const float* cr = reinterpret_cast<const float*>(red);
        for (int c = threadIdx.x; c < E; c += 256)
            cs_partial[(size_t)blockIdx.x * E + c] = (cr[c] + cr[256 * NV + c]) + (cr[512 * NV + c] + cr[768 * NV + c]);
    }
}

// ---- patch layout -> image layout
__global__ __launch_bounds__(256) void depatchify_kernel(const float* __restrict__ patches, float* __restrict__ img,
                                                         int C, int S, int P, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // index into img [BD, C, S, S]
    if (i >= total) return;
    const int x = i % S; long r = i / S;
    const int yy = r % S; r /= S;
    const int c = r % C; const long bd = r / C;
    const int g = S / P, ph = yy / P, p1 = yy - ph * P, pw = x / P, p2 = x - pw * P;
    img[i] = patches[((bd * g + ph) * g + pw) * (long)(P * P * C) + (p1 * P + p2) * C + c];
}

// ---- date features (maestro/layers/utils.py:128-167), same fp32 operation order as the reference:
// out[b, row_off + d, :] = fac * [diff x4, sin(2pi doy/365.25), cos, sin(2pi hour/24), cos], diff = (year+doy')-(year_ref+doy_ref')
__global__ __launch_bounds__(256) void date_features_kernel(const int16_t* __restrict__ dates, const int16_t* __restrict__ ref,
                                                            float* __restrict__ out, int B, int D, int rows, int row_off, float fac) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, d = i - b * D;
    const int16_t* dt = dates + (size_t)i * 3;
    const float year = (float)dt[0], doy = (float)dt[1] / 365.25f, hour = (float)dt[2] / 24.0f;
    const float year_ref = (float)ref[b * 3], doy_ref = (float)ref[b * 3 + 1] / 365.25f;
    const float diff = (year + doy) - (year_ref + doy_ref);
    const float a = 6.283185307179586f * doy, h = 6.283185307179586f * hour;
    float* o = out + ((size_t)b * rows + row_off + d) * 8;
    o[0] = o[1] = o[2] = o[3] = diff * fac;
    o[4] = sinf(a) * fac; o[5] = cosf(a) * fac; o[6] = sinf(h) * fac; o[7] = cosf(h) * fac;
}

// ---- out = img with channels >= 1 replaced by 30 * (ch0 - ch)   (maestro/ssl/mim.py:433-436)
__global__ __launch_bounds__(256) void rescale_elev_kernel(const float* __restrict__ img, float* __restrict__ out, int C, long plane, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long px = i % plane; const long r = i / plane; const int c = r % C; const long bd = r / C;
    const float v = img[i];
    out[i] = c == 0 ? v : 30.f * (img[(bd * C) * plane + px] - v);
}

// ---- raster resize to image_size (maestro/ssl/mim.py:427-432 -> F.interpolate, align_corners=False): PyTorch's index maps
// mode 0 nearest: src = min(floor(dst * in/out), in-1); mode 1 bilinear: src = max((dst+0.5)*in/out - 0.5, 0);
// mode 2 bicubic: src = (dst+0.5)*in/out - 0.5 (not clamped), 4x4 taps at floor(src)-1..+2 clamped to the image, cubic
// convolution weights with A = -0.75 (PyTorch's upsample_bicubic2d)
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x3 = 2.f - t, x2 = 1.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}
__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ in, float* __restrict__ out, int Hin, int Win,
                                                     int Hout, int Wout, int mode, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = i % Wout; const long r = i / Wout; const int y = r % Hout; const long plane = r / Hout;
    const float* src = in + plane * (long)Hin * Win;
    const float sy = (float)Hin / (float)Hout, sx = (float)Win / (float)Wout;
    if (mode == 0) {
        const int yy = min((int)floorf(y * sy), Hin - 1), xx = min((int)floorf(x * sx), Win - 1);
        out[i] = src[(long)yy * Win + xx];
        return;
    }
    if (mode == 2) {
        const float ry = sy * (y + 0.5f) - 0.5f, rx = sx * (x + 0.5f) - 0.5f;
        const int iy = (int)floorf(ry), ix = (int)floorf(rx);
        float wy[4], wx[4];
        cubic_weights(ry - iy, wy);
        cubic_weights(rx - ix, wx);
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int yy = min(max(iy - 1 + a, 0), Hin - 1);
            float row = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) row += wx[b] * src[(long)yy * Win + min(max(ix - 1 + b, 0), Win - 1)];
            acc += wy[a] * row;
        }
        out[i] = acc;
        return;
    }
    const float fy = fmaxf(sy * (y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * (x + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < Hin - 1 ? 1 : 0), x1 = x0 + (x0 < Win - 1 ? 1 : 0);
    const float ly = fy - y0, lx = fx - x0, hy = 1.f - ly, hx = 1.f - lx;
    out[i] = hy * (hx * src[(long)y0 * Win + x0] + lx * src[(long)y0 * Win + x1]) +
             ly * (hx * src[(long)y1 * Win + x0] + lx * src[(long)y1 * Win + x1]);
}

// ---- per-sample dihedral augmentation of square rasters (maestro/dataset/dataset.py:224-257: flip axis 2, flip axis 3,
// swap axes 2 and 3 of the per-sample [D, C, H, W] array, in that order).  flags[b]: bit0 = flip rows, bit1 = flip columns,
// bit2 = transpose.  out[y, x] = in[yy, xx] with (yy, xx) = transpose ? (x, y) : (y, x), then xx -> S-1-xx if bit1,
// yy -> S-1-yy if bit0.  32x32 tiles through LDS so that the transposed case still reads and writes whole row segments.
template <typename T>
__global__ __launch_bounds__(256) void dihedral_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                       const uint8_t* __restrict__ flags, int S, long planes) {
    __shared__ T tile[32][33];
    const int b = blockIdx.z, f = flags[b], tiles = (S + 31) / 32;
    const bool fh = f & 1, fw = f & 2, tr = f & 4;
    const int ty = blockIdx.x / tiles, tx = blockIdx.x % tiles;
    const size_t base = ((size_t)b * planes + blockIdx.y) * S * S;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    if (!tr) {
        for (int j = ly; j < 32; j += 8) {
            const int y = ty * 32 + j, x = tx * 32 + lx;
            if (y < S && x < S) out[base + (size_t)y * S + x] = in[base + (size_t)(fh ? S - 1 - y : y) * S + (fw ? S - 1 - x : x)];
        }
        return;
    }
    for (int j = ly; j < 32; j += 8) {
        const int dx = tx * 32 + j, dy = ty * 32 + lx;      // destination column / row served by this source element
        if (dx < S && dy < S) tile[j][lx] = in[base + (size_t)(fh ? S - 1 - dx : dx) * S + (fw ? S - 1 - dy : dy)];
    }
    __syncthreads();
    for (int j = ly; j < 32; j += 8) {
        const int y = ty * 32 + j, x = tx * 32 + lx;
        if (y < S && x < S) out[base + (size_t)y * S + x] = tile[lx][j];
    }
}

}  // namespace

extern "C" int mh_resize(const float* in, float* out, long planes, int Hin, int Win, int Hout, int Wout, int mode, void* stream) {
    MH_CHECK_ARG(in && out && in != out && planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "mh_resize: bad arguments");
    MH_CHECK_ARG(mode >= 0 && mode <= 2, "mh_resize: mode %d (0 nearest, 1 bilinear, 2 bicubic)", mode);
    const long total = planes * Hout * Wout;
    hipLaunchKernelGGL(resize_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, in, out, Hin, Win, Hout, Wout,
                       mode, total);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_dihedral(const void* in, void* out, const uint8_t* flags, int B, long planes, int S, int elem_bytes,
                           void* stream) {
    MH_CHECK_ARG(in && out && in != out && flags && B > 0 && B < 65536 && planes > 0 && planes < 65536 && S > 0,
                 "mh_dihedral: bad arguments (out of place, B and planes per sample < 65536)");
    const int tiles = ceil_div(S, 32);
    dim3 grid(tiles * tiles, (unsigned)planes, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (elem_bytes) {
        case 1: hipLaunchKernelGGL(dihedral_kernel<uint8_t>, grid, block, 0, s, (const uint8_t*)in, (uint8_t*)out, flags, S, planes); break;
        case 2: hipLaunchKernelGGL(dihedral_kernel<uint16_t>, grid, block, 0, s, (const uint16_t*)in, (uint16_t*)out, flags, S, planes); break;
        case 4: hipLaunchKernelGGL(dihedral_kernel<uint32_t>, grid, block, 0, s, (const uint32_t*)in, (uint32_t*)out, flags, S, planes); break;
        case 8: hipLaunchKernelGGL(dihedral_kernel<uint64_t>, grid, block, 0, s, (const uint64_t*)in, (uint64_t*)out, flags, S, planes); break;
        default: return mh_fail(-1, "mh_dihedral: element size %d (1, 2, 4 or 8 bytes)", elem_bytes);
    }
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_date_features(const int16_t* dates, const int16_t* ref_date, float* out, int B, int D, int rows, int row_off,
                                float fac, void* stream) {
    MH_CHECK_ARG(dates && ref_date && out && row_off + D <= rows, "mh_date_features: bad arguments");
    hipLaunchKernelGGL(date_features_kernel, dim3(ceil_div(B * D, 256)), dim3(256), 0, (hipStream_t)stream, dates, ref_date, out, B, D,
                       rows, row_off, fac);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_rescale_elev(const float* img, float* out, int BD, int C, int S, void* stream) {
    MH_CHECK_ARG(img && out && img != out, "mh_rescale_elev: bad arguments (out of place only)");
    const long plane = (long)S * S, total = (long)BD * C * plane;
    hipLaunchKernelGGL(rescale_elev_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, img, out, C, plane, total);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_patchify(const float* img, void* cols, float* target, int BD, int Ctot, int S, int P, int Kpad,
                           const int* norm_bands, int n_norm_groups, int normalise, int rescale_elev, void* stream) {
    MH_CHECK_ARG(cols, "mh_patchify: null pointer");
    return mh_patchify_bands(img, cols, target, BD, Ctot, 0, Ctot, S, P, Kpad, norm_bands, n_norm_groups, normalise, rescale_elev,
                             stream);
}

extern "C" int mh_patchify_bands(const float* img, void* cols, float* target, int BD, int Csrc, int c0, int Ctot, int S, int P,
                                 int Kpad, const int* norm_bands, int n_norm_groups, int normalise, int rescale_elev,
                                 void* stream) {
    MH_CHECK_ARG(img && (cols || target), "mh_patchify: null pointer");
    MH_CHECK_ARG(c0 >= 0 && Ctot > 0 && c0 + Ctot <= Csrc, "mh_patchify_bands: band window [%d, %d) outside %d channels", c0, c0 + Ctot, Csrc);
    MH_CHECK_ARG(S % P == 0 && Kpad >= Ctot * P * P && Kpad % 8 == 0, "mh_patchify: bad geometry S=%d P=%d Kpad=%d", S, P, Kpad);
    MH_CHECK_ARG(!normalise || !target || (norm_bands && n_norm_groups > 0), "mh_patchify: norm_bands missing");
    const int K = Ctot * P * P, g = S / P;
    if (P == 16 && Ctot <= 4 && S % 4 == 0 && ((uintptr_t)img % 16) == 0 && (!cols || (uintptr_t)cols % 8 == 0) &&
        (!target || (uintptr_t)target % 16 == 0)) {   // one wave per patch (see patchify_wave16_kernel)
        const int n_tok = BD * g * g;
        dim3 grid(ceil_div(n_tok, 4)), block(256);
        hipStream_t s = (hipStream_t)stream;
#define PATCHIFY16(CT) hipLaunchKernelGGL(patchify_wave16_kernel<CT>, grid, block, 0, s, img, (bf16_t*)cols, target, Csrc, c0, S, Kpad, \
                                          norm_bands, n_norm_groups, normalise, rescale_elev, n_tok)
        switch (Ctot) { case 1: PATCHIFY16(1); break; case 2: PATCHIFY16(2); break; case 3: PATCHIFY16(3); break; default: PATCHIFY16(4); }
#undef PATCHIFY16
        MH_LAUNCH_CHECK();
        return 0;
    }
    const int threads = K <= 128 ? 64 : 256;
    const size_t lds = (size_t)(K + 8) * sizeof(float);
    MH_CHECK_ARG(lds <= 64 * 1024, "mh_patchify: patch too large for LDS (%d floats)", K);
    hipLaunchKernelGGL(patchify_kernel, dim3(BD * g * g), dim3(threads), lds, (hipStream_t)stream, img, (bf16_t*)cols,
                       target, Csrc, c0, Ctot, S, P, Kpad, norm_bands, n_norm_groups, normalise, rescale_elev);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_groupnorm_stats(const float* y, float* partial, float* stats, int BD, int L, int E, float eps,
                                  void* stream) {
    MH_CHECK_ARG(y && partial && stats && E % 4 == 0, "mh_groupnorm_stats: bad arguments");
    const long per_image = (long)L * E;
    const int nchunk = ceil_div(per_image, GN_CHUNK);
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunk, BD), dim3(256), 0, (hipStream_t)stream, y, partial, per_image, nchunk);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(BD), dim3(64), 0, (hipStream_t)stream, partial, stats, per_image, nchunk, eps);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_groupnorm_partial_size(int BD, int L, int E) { return BD * ceil_div((long)L * E, GN_CHUNK) * 2; }

extern "C" int mh_embed_finish(const float* y, const float* stats, const float* gamma, const float* beta,
                               const float* pos, const float* date, int date_rows, int date_off, float* xg, int B, int D,
                               int L, int E, int tok_off, int Lgroup, void* stream) {
    MH_CHECK_ARG(y && stats && gamma && beta && pos && xg && E % 4 == 0 && E >= 8, "mh_embed_finish: bad arguments");
    MH_CHECK_ARG(tok_off + D * L <= Lgroup, "mh_embed_finish: modality does not fit its group sequence");
    hipLaunchKernelGGL(embed_finish_kernel, dim3(ceil_div((long)B * D * L, 4)), dim3(256), 0, (hipStream_t)stream, y, stats,
                       gamma, beta, pos, date, xg, B, D, L, E, tok_off, Lgroup, date_rows, date_off);
    MH_LAUNCH_CHECK();
    return 0;
}

// Host side of the three GroupNorm-backward entries: the shared size checks, the width dispatch, the grids, the LDS size and the
// launches -- always in this order, because the calls are captured into hipGraphs.  ``det``: blk_sums and the ordered finish instead of
// the zeroed, atomically accumulated sums (dgamma is then the parameter partial, dbeta unused).  ``cs_partial``: the ends form (whose
// entry refuses E > 1024), with ``inv`` / ``n_vis`` if the gradient comes through the position map.
struct EmbedBwd {
    const float* dxg; const int* inv; int n_vis;
    const float *y, *stats, *gamma;
    bf16_t* dyc; float *dgamma, *dbeta, *sums, *blk_sums, *cs_partial;
    int B, D, L, E, tok_off, Lgroup;
};

template <int NV, bool DET, bool MAP, bool CS, bool WIDE>
static void launch_embed_bwd_form(const EmbedBwd& a, hipStream_t s) {
    const int nblk = ceil_div(a.L, 4 * EB_ROWS);
    const dim3 grid(nblk, a.B * a.D), grid2(ceil_div((long)a.B * a.D * a.L, 4 * (CS ? EA_ROWS : 1))), block(256);
    const size_t lds = (size_t)(8 * std::min(a.E, 256 * NV) + (DET ? 8 : 0)) * sizeof(float);
    // (a KERNEL, not hipMemsetAsync: these entry points are captured into hipGraphs, and on ROCm 7.2 the 16-byte memset node of a
    //  [B = 2, D = 1] modality replayed wrongly -- garbage in `sums` from the second replay on, found in round 3 by the order of
    //  the GPU tests; every other node of the graph was fine)
    if (!DET) hipLaunchKernelGGL(zero_f32_kernel, dim3(ceil_div((long)a.B * a.D * 2, 256)), block, 0, s, a.sums, a.B * a.D * 2);
    hipLaunchKernelGGL((embed_bwd_stats_kernel<NV, DET, MAP, WIDE>), grid, block, lds, s, a.dxg, a.y, a.stats, a.gamma,
                       DET ? a.blk_sums : a.sums, a.dgamma, a.dbeta, a.B, a.D, a.L, a.E, a.tok_off, a.Lgroup, a.inv, a.n_vis);
    if (DET) hipLaunchKernelGGL(embed_bwd_sums_det_kernel, dim3(a.B * a.D), dim3(64), 0, s, a.blk_sums, a.sums, nblk);
    hipLaunchKernelGGL((embed_bwd_apply_kernel<NV, MAP, CS, WIDE>), grid2, block, 0, s, a.dxg, a.inv, a.n_vis, a.y, a.stats, a.gamma,
                       a.sums, a.dyc, a.cs_partial, a.B, a.D, a.L, a.E, a.tok_off, a.Lgroup);
}

static int launch_embed_bwd(const char* name, bool det, const EmbedBwd& a, void* stream) {
    MH_CHECK_ARG(a.B > 0 && a.D > 0 && a.L > 0 && a.E > 0 && a.E % 4 == 0 && a.tok_off >= 0 && a.tok_off + a.D * a.L <= a.Lgroup,
                 "%s: bad sizes B=%d D=%d L=%d E=%d (E %% 4 == 0) tok_off=%d Lgroup=%d", name, a.B, a.D, a.L, a.E, a.tok_off, a.Lgroup);
    hipStream_t s = (hipStream_t)stream;
    for_row_nv(a.E, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (a.cs_partial) {
            if (a.inv) launch_embed_bwd_form<NV, false, true, true, false>(a, s); else launch_embed_bwd_form<NV, false, false, true, false>(a, s);
        } else if (a.E <= 256 * NV) {
            if (det) launch_embed_bwd_form<NV, true, false, false, false>(a, s); else launch_embed_bwd_form<NV, false, false, false, false>(a, s);
        } else if constexpr (NV == 4) {          // E > 1024: column passes
            if (det) launch_embed_bwd_form<4, true, false, false, true>(a, s); else launch_embed_bwd_form<4, false, false, false, true>(a, s);
        }
    });
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_embed_finish_bwd(const float* dxg, const float* y, const float* stats, const float* gamma, void* dyc,
                                   float* dgamma, float* dbeta, float* sums, int B, int D, int L, int E, int tok_off,
                                   int Lgroup, void* stream) {
    MH_CHECK_ARG(dxg && y && stats && gamma && dyc && dgamma && dbeta && sums, "mh_embed_finish_bwd: null pointer");
    return launch_embed_bwd("mh_embed_finish_bwd", false,
                            {dxg, nullptr, 0, y, stats, gamma, (bf16_t*)dyc, dgamma, dbeta, sums, nullptr, nullptr, B, D, L, E, tok_off, Lgroup},
                            stream);
}

extern "C" int mh_embed_bwd_cs_rows(long rows) { return rows > 0 ? (int)ceil_div(rows, (long)(4 * EA_ROWS)) : 0; }

extern "C" int mh_embed_finish_bwd_ends(const float* dx, const int* inv, int n_vis, const float* y, const float* stats,
                                        const float* gamma, void* dyc, float* dgamma, float* dbeta, float* sums, float* cs_partial,
                                        int B, int D, int L, int E, int tok_off, int Lgroup, void* stream) {
    MH_CHECK_ARG(dx && y && stats && gamma && dyc && dgamma && dbeta && sums && cs_partial, "mh_embed_finish_bwd_ends: null pointer");
    MH_CHECK_ARG(E <= 1024 && (!inv || (n_vis > 0 && n_vis <= Lgroup)), "mh_embed_finish_bwd_ends: bad sizes E=%d (E <= 1024) n_vis=%d Lgroup=%d",
                 E, n_vis, Lgroup);
    return launch_embed_bwd("mh_embed_finish_bwd_ends", false,
                            {dx, inv, n_vis, y, stats, gamma, (bf16_t*)dyc, dgamma, dbeta, sums, nullptr, cs_partial, B, D, L, E, tok_off, Lgroup},
                            stream);
}

extern "C" int mh_embed_bwd_partial_rows(int BD, int L) { return BD > 0 && L > 0 ? BD * ceil_div(L, 4 * EB_ROWS) : 0; }

extern "C" int mh_embed_finish_bwd_det(const float* dxg, const float* y, const float* stats, const float* gamma, void* dyc,
                                       float* param_partial, float* blk_sums, float* sums, int B, int D, int L, int E, int tok_off,
                                       int Lgroup, void* stream) {
    MH_CHECK_ARG(dxg && y && stats && gamma && dyc && param_partial && blk_sums && sums, "mh_embed_finish_bwd_det: null pointer");
    return launch_embed_bwd("mh_embed_finish_bwd_det", true,
                            {dxg, nullptr, 0, y, stats, gamma, (bf16_t*)dyc, param_partial, nullptr, sums, blk_sums, nullptr, B, D, L, E, tok_off,
                             Lgroup},
                            stream);
}

extern "C" int mh_depatchify(const float* patches, float* img, int BD, int C, int S, int P, void* stream) {
    MH_CHECK_ARG(patches && img && S % P == 0, "mh_depatchify: bad arguments");
    const long total = (long)BD * C * S * S;
    hipLaunchKernelGGL(depatchify_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, patches, img, C, S, P, total);
    MH_LAUNCH_CHECK();
    return 0;
}
