// LayerNorm forward/backward for the fp32 residual stream (see include/maestro_hip.h).
// One wave (64 lanes) per row, row held in registers as float4 (dim <= 2048), two-pass statistics, wavefront
// shuffles for the reductions.  Rows are addressed through (sample, j) maps so that "split / concat of group
// sequences" (reference mim.py:408-423) is done by addressing instead of copies:
//     row(b, j) = b * L + off + j,  j < n.
#include "gemm_common.hpp"
#include <type_traits>

namespace {

struct RowMap { int L, off; };
__device__ __forceinline__ size_t map_row(RowMap m, int b, int j) { return (size_t)b * m.L + m.off + j; }

// NV = float4 per lane (dim <= 256*NV); registers are sized exactly for the row width (no spills).
template <int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, RowMap xm, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, void* __restrict__ y, RowMap ym,
                                                     int y_is_f32, float* __restrict__ mean, float* __restrict__ rstd,
                                                     int B, int n, int dim, float eps, uint8_t* __restrict__ y8,
                                                     const float* __restrict__ y8_scale, float* __restrict__ y8_amax,
                                                     uint8_t* __restrict__ y8s, int ld_y8s) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B * n) return;
    const int b = row / n, j = row - b * n;
    const float* xr = x + map_row(xm, b, j) * dim;
    const int nv = dim >> 2;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (f32x4){0, 0, 0, 0};
        if (c < nv) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * c);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mu = wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mu; q += d * d; }
        }
    }
    const float rs = rsqrtf(wave_sum(q) / dim + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    const size_t yrow = map_row(ym, b, j) * dim;
    const bool t8 = y8 && !y8s;                // per-tensor e4m3 copy; y8s: the MX copy of the bf16 output (dim %% 32 == 0)
    const float s8 = t8 ? *y8_scale : 0.f;     // fp8 path: an e4m3 copy of the output (the next GEMM's A operand) + its absmax
    float amax8 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        u32x2 pk16 = {0u, 0u};
        if (c < nv) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mu) * rs * g[e] + bt[e];
            if (y_is_f32) {
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(y) + yrow + 4 * c) = o;
            } else {
                u32x2 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
                *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(y) + yrow + 4 * c) = pk;
                pk16 = pk;
            }
            if (t8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) amax8 = amax_fold(amax8, o[e]);
                *reinterpret_cast<uint32_t*>(y8 + yrow + 4 * c) = pack_e4m3x4(o, s8);
            }
        }
        if (y8s) {      // (every lane: the 8 lanes of a 32-element block are all inside the row or all beyond it)
            const f32x4 q = bf2x2_to_f32x4(pk16[0], pk16[1]);
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) a = amax_fold(a, q[e]);
            const uint32_t sbyte = mx_scale_byte(group_amax<8>(a));
            if (c < nv) {
                *reinterpret_cast<uint32_t*>(y8 + yrow + 4 * c) = pack_e4m3x4(q, mx_inv_scale(sbyte));
                if ((lane & 7) == 0) y8s[map_row(ym, b, j) * ld_y8s + (c >> 3)] = (uint8_t)sbyte;
            }
        }
    }
    if (t8 && y8_amax) {
        amax8 = wave_amax(amax8);
        if (lane == 0 && amax_nonzero(amax8)) atomic_max_pos(y8_amax, amax8);
    }
}

// Straight-line forward for the step's own case (dim == 256 * NV: every lane holds NV float4; bf16 output, optional e4m3 copy).
// Same operations in the same order as ln_fwd_kernel (results equal up to the compiler's fma contraction: a few fp32 ulp,
// tests/test_kernels_gpu.py), but no lane predicates and no output-type branches, so that the code is ONE scheduling region.  In the generic kernel's ISA (gfx950, -O3) every predicated chunk
// ends in `s_waitcnt vmcnt(0)`: the row's NV loads went out as NV dependent round trips, gamma / beta were fetched after
// the two reductions, chunk by chunk, and each chunk's wait also covered the previous chunk's STORES -- 7-8 memory round
// trips per row, one after the other.  Here the row, gamma and beta are requested back to back before anything is
// waited for, and the stores leave together at the end.
// Wave sum of the straight-line kernels (all 64 lanes active there): each 16-lane row all-reduces by four DPP rotations
// (row_ror:8, 4, 2, 1: one v_add_f32_dpp each, no LDS crossbar round trip), then the four row sums meet through v_readlane.
// With the loads no longer serialized the twelve ds_bpermute round trips per row of the shuffle butterfly (wave_sum) show:
// forward -4 ... -7 % per launch, backward -1 ... -9 % (profiles/r03_ln_straightline.txt).  The sums differ from the generic
// kernels' in their last bits by fma contraction and by the order of the 64 partial sums.
__device__ __forceinline__ float ln_wave_sum(float v) {
#define MH_ROR(n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (n), 0xf, 0xf, false))
    v += MH_ROR(8); v += MH_ROR(4); v += MH_ROR(2); v += MH_ROR(1);
#undef MH_ROR
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}
// Y8 = LN_Y8_TENSOR (mh_layernorm_fwd_fp8): the same kernel also writes the e4m3 copy of the output (the next GEMM's A operand)
// and folds |y| into the tensor's amax row; Y8 = LN_Y8_MX (mh_layernorm_fwd_mx): the MX copy of the BF16 output -- a lane holds
// 4 consecutive values per i, so 8 lanes hold one 32-element block (3 xor shuffles for its max), lane (l & 7) == 0 writes the
// scale byte.  The bf16 output is the SAME instruction sequence in all three, hence bit-identical to Y8 = LN_Y8_NONE.  (Other
// widths with dim %% 32 == 0 -- the small models' 384 -- take the generic ln_fwd_kernel, which writes the MX copy the same way.)
enum { LN_Y8_NONE = 0, LN_Y8_TENSOR = 1, LN_Y8_MX = 2 };
template <int NV, int Y8>
__global__ __launch_bounds__(256) void ln_fwd_fast_kernel(const float* __restrict__ x, RowMap xm, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, bf16_t* __restrict__ y, RowMap ym,
                                                          float* __restrict__ mean, float* __restrict__ rstd, int B, int n,
                                                          float eps, uint8_t* __restrict__ y8, const float* __restrict__ y8_scale,
                                                          float* __restrict__ y8_amax, uint8_t* __restrict__ y8s, int ld_y8s) {
    constexpr int dim = 256 * NV;
    constexpr bool FP8 = Y8 == LN_Y8_TENSOR;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B * n) return;
    const int b = row / n, j = row - b * n;
    const float* xr = x + map_row(xm, b, j) * dim;
    f32x4 v[NV], g[NV], bt[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * (lane + 64 * i));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = *reinterpret_cast<const f32x4*>(gamma + 4 * (lane + 64 * i));
        bt[i] = *reinterpret_cast<const f32x4*>(beta + 4 * (lane + 64 * i));
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    const float mu = ln_wave_sum(s) / dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mu; q += d * d; }
    }
    const float rs = rsqrtf(ln_wave_sum(q) / dim + eps);
    const size_t yrow = map_row(ym, b, j) * dim;
    bf16_t* yr = y + yrow;
    float s8 = 0.f;
    if constexpr (FP8) s8 = *y8_scale;
    float amax8 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mu) * rs * g[i][e] + bt[i][e];
        const u32x2 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
        *reinterpret_cast<u32x2*>(yr + 4 * (lane + 64 * i)) = pk;
        if constexpr (Y8 == LN_Y8_MX) {
            const f32x4 q = bf2x2_to_f32x4(pk[0], pk[1]);
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) a = amax_fold(a, q[e]);
            const uint32_t sbyte = mx_scale_byte(group_amax<8>(a));
            *reinterpret_cast<uint32_t*>(y8 + yrow + 4 * (lane + 64 * i)) = pack_e4m3x4(q, mx_inv_scale(sbyte));
            if ((lane & 7) == 0) y8s[map_row(ym, b, j) * ld_y8s + ((lane + 64 * i) >> 3)] = (uint8_t)sbyte;
        }
        if constexpr (FP8) {
#pragma unroll
            for (int e = 0; e < 4; ++e) amax8 = amax_fold(amax8, o[e]);
            *reinterpret_cast<uint32_t*>(y8 + yrow + 4 * (lane + 64 * i)) = pack_e4m3x4(o, s8);
        }
    }
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    if constexpr (FP8) {
        if (y8_amax) {
            amax8 = wave_amax(amax8);
            if (lane == 0 && amax_nonzero(amax8)) atomic_max_pos(y8_amax, amax8);
        }
    }
}

// Backward. Each wave walks ROWS_PER_WAVE rows keeping per-column partials of dgamma, dbeta and colsum(dx) in
// registers; the block reduces them through LDS and writes ONE partial row [3*dim] to the workspace (plain stores);
// ln_bwd_reduce_kernel then sums the partial rows (few atomics per column, no same-address storm).
constexpr int ROWS_PER_WAVE = 4;  // 16 rows per block, >= 2 blocks per CU at M = 8192 (8 was bandwidth-starved: 256 blocks)

// The block tail of the backward kernels: every wave parks gsum | bsum | csum in LDS ([4 waves][3][dim]), the block adds the
// four waves and stores one partial row.  FULL: dim == 256 * NV, every lane holds all of its NV chunks (no lane predicate).
template <int NV, bool FULL>
__device__ __forceinline__ void ln_bwd_store_partial(float* red, float* __restrict__ partial, const f32x4 (&gsum)[NV],
                                                     const f32x4 (&bsum)[NV], const f32x4 (&csum)[NV], int w, int lane, int dim) {
    float* rg = red + (size_t)w * 3 * dim;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (FULL || c < (dim >> 2)) {
            *reinterpret_cast<f32x4*>(rg + 4 * c) = gsum[i];
            *reinterpret_cast<f32x4*>(rg + dim + 4 * c) = bsum[i];
            *reinterpret_cast<f32x4*>(rg + 2 * dim + 4 * c) = csum[i];
        }
    }
    __syncthreads();
    float* prow = partial + (size_t)blockIdx.x * 3 * dim;
    for (int c = threadIdx.x; c < 3 * dim; c += 256)
        prow[c] = red[c] + red[3 * dim + c] + red[6 * dim + c] + red[9 * dim + c];
}

template <int NV>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy, RowMap dym, int dy_is_f32,
                                                     const float* __restrict__ x, RowMap xm,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dres,
                                                     float* __restrict__ dx, bf16_t* __restrict__ dx_bf16,
                                                     float* __restrict__ partial, int B, int n, int dim) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves][3][dim]
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nv = dim >> 2;
    f32x4 gsum[NV], bsum[NV], csum[NV], gm[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        gsum[i] = (f32x4){0, 0, 0, 0}; bsum[i] = (f32x4){0, 0, 0, 0}; csum[i] = (f32x4){0, 0, 0, 0};
        const int c = lane + 64 * i;
        gm[i] = c < nv ? *reinterpret_cast<const f32x4*>(gamma + 4 * c) : (f32x4){0, 0, 0, 0};
    }
    const int row0 = (blockIdx.x * 4 + w) * ROWS_PER_WAVE;
    const int rows = B * n;
    // Software pipeline over the wave's rows: every operand of row r+1 (x, dy and the residual gradient) is requested
    // before row r is reduced, so a wave keeps two rows of loads in flight instead of two dependent round trips per row.
    f32x4 xv_n[NV], rs_n[NV];
    u32x4 dy_n[NV];      // bf16: .xy hold 4 values; f32: all four lanes
    float mu_n = 0.f, rstd_n = 0.f;
    size_t xrow_n = 0;
    auto fetch = [&](int row) {
        const int b = row / n, j = row - b * n;
        xrow_n = map_row(xm, b, j) * dim;
        const size_t dyrow = map_row(dym, b, j) * dim;
        mu_n = mean[row]; rstd_n = rstd[row];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                xv_n[i] = *reinterpret_cast<const f32x4*>(x + xrow_n + 4 * c);
                if (dy_is_f32) {
                    dy_n[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(dy) + dyrow + 4 * c);
                } else {
                    const u32x2 pk = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(dy) + dyrow + 4 * c);
                    dy_n[i] = (u32x4){pk[0], pk[1], 0u, 0u};
                }
                rs_n[i] = dres ? *reinterpret_cast<const f32x4*>(dres + xrow_n + 4 * c) : (f32x4){0, 0, 0, 0};
            }
        }
    };
    if (row0 < rows) fetch(row0);
    for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
        const int row = row0 + rr;
        if (row >= rows) break;
        const size_t xrow = xrow_n;
        const float mu = mu_n, rs = rstd_n;
        f32x4 xh[NV], dz[NV], rsd[NV];
        u32x4 dyv[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) { xh[i] = xv_n[i]; dyv[i] = dy_n[i]; rsd[i] = rs_n[i]; }
        if (rr + 1 < ROWS_PER_WAVE && row + 1 < rows) fetch(row + 1);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            const f32x4 xv = xh[i];
            xh[i] = (f32x4){0, 0, 0, 0}; dz[i] = (f32x4){0, 0, 0, 0};
            if (c < nv) {
                f32x4 d;
                if (dy_is_f32) {
                    d = __builtin_bit_cast(f32x4, dyv[i]);
                } else {
                    // (bf2x2_to_f32x4 written out: through the call the NV = 8 form takes 446 + 190 registers instead of 444 + 188)
                    d = (f32x4){__uint_as_float(dyv[i][0] << 16), __uint_as_float(dyv[i][0] & 0xffff0000u),
                                __uint_as_float(dyv[i][1] << 16), __uint_as_float(dyv[i][1] & 0xffff0000u)};
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xh[i][e] = (xv[e] - mu) * rs;
                    dz[i][e] = d[e] * gm[i][e];
                    s1 += dz[i][e];
                    s2 += dz[i][e] * xh[i][e];
                    gsum[i][e] += d[e] * xh[i][e];
                    bsum[i][e] += d[e];
                }
            }
        }
        const float c1 = wave_sum(s1) / dim, c2 = wave_sum(s2) / dim;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rs * (dz[i][e] - c1 - xh[i][e] * c2);
                o += rsd[i];
                csum[i] += o;
                *reinterpret_cast<f32x4*>(dx + xrow + 4 * c) = o;
                if (dx_bf16) {
                    u32x2 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
                    *reinterpret_cast<u32x2*>(dx_bf16 + xrow + 4 * c) = pk;
                }
            }
        }
    }
    if (!partial) return;
    ln_bwd_store_partial<NV, false>(red, partial, gsum, bsum, csum, w, lane, dim);
}

// Straight-line backward for the step's own cases: dim == 256 * NV, a bf16 copy of dx to write, rows % ROWS_PER_WAVE == 0 (a
// wave's rows exist together).  Same operations, same order, same partial-row layout as ln_bwd_kernel (results equal up to fma
// contraction / packing: a few fp32 ulp).  Why it exists: in the generic kernel the run-time cases
// (dy type, dres / dx_bf16 present, lane < nv) are branches INSIDE the software pipeline; its ISA waits `vmcnt(0)` after
// each chunk's dy load (the bf16 words are moved into the f32-sized registers of the other case) and again at the loop
// head (store counts are not static across the branches), so the "prefetch" of the next row was NV + 1 dependent round
// trips and also waited for the previous row's stores: ~5 us per row and wave, whatever the bandwidth.  Here the wave's
// rows are unrolled, the operands of DEPTH rows are in flight before the first one is reduced, the waits carry exact
// counts, and the sched_barriers pin the issue order (loads of row r + DEPTH, then the arithmetic and stores of row r).
// Three forms are launched, all decided at compile time so that nothing is decided inside the pipeline:
//   <., ., false, true>    the transformer blocks: bf16 dy, a residual gradient to add (RES);
//   <., ., false, false>   the final LayerNorms of the step (decoder per modality, joint / encoder per group): no residual gradient;
//   <., ., true,  false>   the same with fp32 dy (DY_F32: one 16-byte load per chunk, nothing to unpack).
// ONE __global__ template whose differences are `if constexpr`, not a __device__ body shared by several kernels: routed through
// an inlined function the blocks' form once grew from 177 to 200 registers at dim 768 and from 238 to 262 at dim 1024; as one
// template every form keeps the registers its hand-written kernel had (74 / 121 / 177 / 238 with RES, 66 / 104 / 149 / 209 and
// 68 / 104 / 150 / 214 without, NV = 1 .. 4: profiles/ln_unify.md).
constexpr int ln_bwd_depth(int nv) { return nv <= 3 ? 4 : 2; }   // rows of operands in flight per wave before the first is reduced (two at dim 1024: registers)
template <int NV, int DEPTH, bool DY_F32, bool RES>
__global__ __launch_bounds__(256) void ln_bwd_fast_kernel(const void* __restrict__ dy, RowMap dym, const float* __restrict__ x,
                                                          RowMap xm, const float* __restrict__ gamma,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ dres, float* __restrict__ dx,
                                                          bf16_t* __restrict__ dx_bf16, float* __restrict__ partial, int B, int n) {
    constexpr int dim = 256 * NV;
    static_assert(DEPTH >= 1 && DEPTH <= ROWS_PER_WAVE, "prefetch distance in rows");
    static_assert(!(DY_F32 && RES), "fp32 dy with a residual gradient takes the generic kernel: nothing launches this form");
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves][3][dim]
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    f32x4 gsum[NV], bsum[NV], csum[NV], gm[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        gsum[i] = (f32x4){0, 0, 0, 0}; bsum[i] = (f32x4){0, 0, 0, 0}; csum[i] = (f32x4){0, 0, 0, 0};
        gm[i] = *reinterpret_cast<const f32x4*>(gamma + 4 * (lane + 64 * i));
    }
    const int row0 = (blockIdx.x * 4 + w) * ROWS_PER_WAVE;
    if (row0 < B * n) {
        f32x4 xq[ROWS_PER_WAVE][NV], rq[RES ? ROWS_PER_WAVE : 1][NV];
        std::conditional_t<DY_F32, f32x4, u32x2> dq[ROWS_PER_WAVE][NV];
        float muq[ROWS_PER_WAVE], rsq[ROWS_PER_WAVE];
        size_t xrowq[ROWS_PER_WAVE];
        auto fetch = [&](int p) {
            const int row = row0 + p, b = row / n, j = row - b * n;
            xrowq[p] = map_row(xm, b, j) * dim;
            const size_t dyrow = map_row(dym, b, j) * dim;
            muq[p] = mean[row]; rsq[p] = rstd[row];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c4 = 4 * (lane + 64 * i);
                xq[p][i] = *reinterpret_cast<const f32x4*>(x + xrowq[p] + c4);
                if constexpr (DY_F32) dq[p][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(dy) + dyrow + c4);
                else dq[p][i] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(dy) + dyrow + c4);
                if constexpr (RES) rq[p][i] = *reinterpret_cast<const f32x4*>(dres + xrowq[p] + c4);
            }
        };
#pragma unroll
        for (int p = 0; p < DEPTH; ++p) fetch(p);
#pragma unroll
        for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
            if (rr + DEPTH < ROWS_PER_WAVE) fetch(rr + DEPTH);
            __builtin_amdgcn_sched_barrier(0);
            const float mu = muq[rr], rs = rsq[rr];
            f32x4 xh[NV], dz[NV];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                f32x4 d;
                if constexpr (DY_F32) d = dq[rr][i];
                else d = bf2x2_to_f32x4(dq[rr][i][0], dq[rr][i][1]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xh[i][e] = (xq[rr][i][e] - mu) * rs;
                    dz[i][e] = d[e] * gm[i][e];
                    s1 += dz[i][e];
                    s2 += dz[i][e] * xh[i][e];
                    gsum[i][e] += d[e] * xh[i][e];
                    bsum[i][e] += d[e];
                }
            }
            const float c1 = ln_wave_sum(s1) / dim, c2 = ln_wave_sum(s2) / dim;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c4 = 4 * (lane + 64 * i);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rs * (dz[i][e] - c1 - xh[i][e] * c2);
                if constexpr (RES) o += rq[rr][i];
                csum[i] += o;
                *reinterpret_cast<f32x4*>(dx + xrowq[rr] + c4) = o;
                const u32x2 pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
                *reinterpret_cast<u32x2*>(dx_bf16 + xrowq[rr] + c4) = pk;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (!partial) return;
    ln_bwd_store_partial<NV, true>(red, partial, gsum, bsum, csum, w, lane, dim);
}

constexpr int RED_ROWS = 8;   // 8 partial rows per thread: short dependent-free load chains, 4x more (cheap) atomics
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ partial, int nblk, int dim,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float* __restrict__ dcol) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 3 * dim) return;
    const int r0 = blockIdx.y * RED_ROWS, r1 = min(nblk, r0 + RED_ROWS);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += partial[(size_t)r * 3 * dim + c];
    if (c < dim) atomicAdd(dgamma + c, s);
    else if (c < 2 * dim) atomicAdd(dbeta + (c - dim), s);
    else if (dcol) atomicAdd(dcol + (c - 2 * dim), s);
}

// One launch for many small column sums (LayerNorm partial rows, bias block sums): workgroup b runs the host-listed work item
// blocks[b] = (job, column block, row chunk), so jobs of very different shapes share a dense grid.
__global__ __launch_bounds__(256) void colsum_batched_kernel(const MhColsumJob* __restrict__ jobs, int n_jobs,
                                                             const uint64_t* __restrict__ blocks) {
    const uint64_t e = blocks[blockIdx.x];
    const int ji = (int)(e >> 48);
    if (ji >= n_jobs) return;
    const MhColsumJob j = jobs[ji];
    const int c = (int)((e >> 32) & 0xFFFF) * 256 + threadIdx.x;
    const int r0 = (int)(e & 0xFFFFFFFFu) * MH_COLSUM_ROWS;
    if (c >= j.cols || r0 >= j.rows) return;
    const int r1 = min(j.rows, r0 + MH_COLSUM_ROWS);
    // the chunk's loads go out together (the rolled loop was load -> s_waitcnt vmcnt(0) -> add: MH_COLSUM_ROWS dependent
    // round trips per thread); the adds keep their order
    const float* src = j.src + (size_t)r0 * j.ld + c;
    float v[MH_COLSUM_ROWS];
#pragma unroll
    for (int i = 0; i < MH_COLSUM_ROWS; ++i) v[i] = r0 + i < r1 ? src[(size_t)i * j.ld] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MH_COLSUM_ROWS; ++i) s += v[i];
    atomicAdd(j.dst + c, s);
}

}  // namespace

static int ln_nv(int dim) { const int v = (dim / 4 + 63) / 64; return v <= 4 ? v : 8; }
// f(std::integral_constant<int, NV>) for the value of ln_nv: the one place that turns the row width into a template argument.
// WIDE: the generic kernels, which also have the NV = 8 form (dim <= 2048); the straight-line ones end at NV = 4.
template <int V> using ln_c = std::integral_constant<int, V>;
template <bool WIDE, class F>
static void ln_for_nv(int nvs, F f) {
    switch (nvs) {
        case 1: f(ln_c<1>{}); break;
        case 2: f(ln_c<2>{}); break;
        case 3: f(ln_c<3>{}); break;
        case 4: f(ln_c<4>{}); break;
        default: if constexpr (WIDE) f(ln_c<8>{});
    }
}

static int layernorm_fwd_impl(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L,
                              int y_off, int y_is_f32, float* mean, float* rstd, int B, int n, int dim, float eps, void* y8,
                              const float* y8_scale, float* y8_amax, void* stream, void* y8s, int ld_y8s);

extern "C" int mh_layernorm_fwd(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y,
                                int y_L, int y_off, int y_is_f32, float* mean, float* rstd, int B, int n, int dim,
                                float eps, void* stream) {
    return layernorm_fwd_impl(x, x_L, x_off, gamma, beta, y, y_L, y_off, y_is_f32, mean, rstd, B, n, dim, eps, nullptr, nullptr,
                              nullptr, stream, nullptr, 0);
}

extern "C" int mh_layernorm_fwd_fp8(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y,
                                    int y_L, int y_off, float* mean, float* rstd, int B, int n, int dim, float eps, void* y8,
                                    const float* y8_scale, float* y8_amax, void* stream) {
    MH_CHECK_ARG(y8 && y8_scale && ((uintptr_t)y8 % 4) == 0, "mh_layernorm_fwd_fp8: y8 (4-byte aligned) and its scale are required");
    return layernorm_fwd_impl(x, x_L, x_off, gamma, beta, y, y_L, y_off, 0, mean, rstd, B, n, dim, eps, y8, y8_scale, y8_amax, stream,
                              nullptr, 0);
}

extern "C" int mh_layernorm_fwd_mx(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L,
                                   int y_off, float* mean, float* rstd, int B, int n, int dim, float eps, void* y8, void* y8_scales,
                                   int ld_y8s, void* stream) {
    MH_CHECK_ARG(y8 && ((uintptr_t)y8 % 4) == 0, "mh_layernorm_fwd_mx: y8 (4-byte aligned) is required");
    MH_CHECK_ARG(y8_scales, "mh_layernorm_fwd_mx: null scale pointer (y8_scales)");
    MH_CHECK_ARG(ld_y8s % 4 == 0 && ld_y8s >= dim / 32, "mh_layernorm_fwd_mx: ld_y8s must be a multiple of 4 and >= dim / 32 (%d)", ld_y8s);
    return layernorm_fwd_impl(x, x_L, x_off, gamma, beta, y, y_L, y_off, 0, mean, rstd, B, n, dim, eps, y8, nullptr, nullptr, stream,
                              y8_scales, ld_y8s);
}

static int layernorm_fwd_impl(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L,
                              int y_off, int y_is_f32, float* mean, float* rstd, int B, int n, int dim, float eps, void* y8,
                              const float* y8_scale, float* y8_amax, void* stream, void* y8s, int ld_y8s) {
    MH_CHECK_ARG(x && gamma && beta && y && mean && rstd, "mh_layernorm_fwd: null pointer");
    MH_CHECK_ARG(dim % 4 == 0 && dim >= 4 && dim <= 2048, "mh_layernorm_fwd: dim %d unsupported", dim);
    MH_CHECK_ARG(B > 0 && n > 0 && x_off + n <= x_L && y_off + n <= y_L, "mh_layernorm_fwd: bad row map");
    const int rows = B * n;
    dim3 grid(ceil_div(rows, 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const RowMap xm{x_L, x_off}, ym{y_L, y_off};
    const int nvs = ln_nv(dim);
    MH_CHECK_ARG(!y8s || (dim % 32 == 0 && !y_is_f32), "mh_layernorm_fwd_mx: dim %% 32 == 0 required, got %d", dim);
    if (nvs <= 4 && dim == 256 * nvs && !y_is_f32) {     // the step's own case: straight-line kernel (with or without an e4m3 / MX copy)
        auto fast = [&](auto y8_form) {
            ln_for_nv<false>(nvs, [&](auto nv) {
                hipLaunchKernelGGL((ln_fwd_fast_kernel<decltype(nv)::value, decltype(y8_form)::value>), grid, block, 0, s, x, xm, gamma,
                                   beta, (bf16_t*)y, ym, mean, rstd, B, n, eps, (uint8_t*)y8, y8_scale, y8_amax, (uint8_t*)y8s, ld_y8s);
            });
        };
        if (y8s) fast(ln_c<LN_Y8_MX>{}); else if (y8) fast(ln_c<LN_Y8_TENSOR>{}); else fast(ln_c<LN_Y8_NONE>{});
    } else {
        ln_for_nv<true>(nvs, [&](auto nv) {
            hipLaunchKernelGGL(ln_fwd_kernel<decltype(nv)::value>, grid, block, 0, s, x, xm, gamma, beta, y, ym, y_is_f32, mean, rstd, B, n,
                               dim, eps, (uint8_t*)y8, y8_scale, y8_amax, (uint8_t*)y8s, ld_y8s);
        });
    }
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" long mh_layernorm_bwd_workspace(int rows, int dim) {
    return (long)ceil_div(rows, 4 * ROWS_PER_WAVE) * 3 * dim;
}

static int layernorm_bwd_impl(const void* dy, int dy_L, int dy_off, int dy_is_f32, const float* x, int x_L, int x_off,
                              const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                              void* dx_bf16, float* dgamma, float* dbeta, float* dcol, float* workspace, bool partial_only,
                              int B, int n, int dim, void* stream) {
    const int rows = B * n, nblk = ceil_div(rows, 4 * ROWS_PER_WAVE);
    const size_t lds = (size_t)4 * 3 * dim * sizeof(float);
    dim3 grid(nblk), block(256);
    hipStream_t s = (hipStream_t)stream;
    float* part = (dgamma || partial_only) ? workspace : nullptr;
    const RowMap dym{dy_L, dy_off}, xm{x_L, x_off};
    const int nvs = ln_nv(dim);
    const bool fast = nvs <= 4 && dim == 256 * nvs && dx_bf16 && rows % ROWS_PER_WAVE == 0;
    auto fast_form = [&](auto dy_f32, auto res) {      // straight-line kernel, all of a wave's rows in flight (two at dim 1024)
        ln_for_nv<false>(nvs, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            hipLaunchKernelGGL((ln_bwd_fast_kernel<NV, ln_bwd_depth(NV), decltype(dy_f32)::value, decltype(res)::value>), grid, block,
                               lds, s, dy, dym, x, xm, gamma, mean, rstd, dres, dx, (bf16_t*)dx_bf16, part, B, n);
        });
    };
    if (fast && !dres) {              // the final LayerNorms: no residual gradient, dy bf16 or fp32
        if (dy_is_f32) fast_form(std::true_type{}, std::false_type{}); else fast_form(std::false_type{}, std::false_type{});
    } else if (fast && !dy_is_f32) {  // the transformer blocks' own case
        fast_form(std::false_type{}, std::true_type{});
    } else {
        ln_for_nv<true>(nvs, [&](auto nv) {
            hipLaunchKernelGGL(ln_bwd_kernel<decltype(nv)::value>, grid, block, lds, s, dy, dym, dy_is_f32, x, xm, gamma, mean, rstd, dres,
                               dx, (bf16_t*)dx_bf16, part, B, n, dim);
        });
    }
    if (dgamma && !partial_only)
        hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3(ceil_div(3 * dim, 256), ceil_div(nblk, RED_ROWS)), dim3(256), 0, s,
                           workspace, nblk, dim, dgamma, dbeta, dcol);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_layernorm_bwd(const void* dy, int dy_L, int dy_off, int dy_is_f32, const float* x, int x_L, int x_off,
                                const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                                void* dx_bf16, float* dgamma, float* dbeta, float* dcol, float* workspace, int B, int n,
                                int dim, void* stream) {
    MH_CHECK_ARG(dy && x && gamma && mean && rstd && dx, "mh_layernorm_bwd: null pointer");
    MH_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "mh_layernorm_bwd: dgamma/dbeta must come together");
    MH_CHECK_ARG(!dgamma || workspace, "mh_layernorm_bwd: parameter gradients need the workspace");
    MH_CHECK_ARG(!dcol || dgamma, "mh_layernorm_bwd: dcol needs dgamma/dbeta");
    MH_CHECK_ARG(dim % 4 == 0 && dim >= 4 && dim <= 2048, "mh_layernorm_bwd: dim %d unsupported", dim);
    MH_CHECK_ARG(B > 0 && n > 0 && x_off + n <= x_L && dy_off + n <= dy_L, "mh_layernorm_bwd: bad row map");
    return layernorm_bwd_impl(dy, dy_L, dy_off, dy_is_f32, x, x_L, x_off, gamma, mean, rstd, dres, dx, dx_bf16, dgamma, dbeta, dcol,
                              workspace, false, B, n, dim, stream);
}

extern "C" int mh_layernorm_bwd_partial(const void* dy, int dy_L, int dy_off, int dy_is_f32, const float* x, int x_L, int x_off,
                                        const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                                        void* dx_bf16, float* workspace, int B, int n, int dim, void* stream) {
    MH_CHECK_ARG(dy && x && gamma && mean && rstd && dx && workspace, "mh_layernorm_bwd_partial: null pointer");
    MH_CHECK_ARG(dim % 4 == 0 && dim >= 4 && dim <= 2048, "mh_layernorm_bwd_partial: dim %d unsupported", dim);
    MH_CHECK_ARG(B > 0 && n > 0 && x_off + n <= x_L && dy_off + n <= dy_L, "mh_layernorm_bwd_partial: bad row map");
    return layernorm_bwd_impl(dy, dy_L, dy_off, dy_is_f32, x, x_L, x_off, gamma, mean, rstd, dres, dx, dx_bf16, nullptr, nullptr,
                              nullptr, workspace, true, B, n, dim, stream);
}

extern "C" int mh_colsum_batched(const MhColsumJob* jobs_device, int n_jobs, const uint64_t* blocks_device, int n_blocks,
                                 void* stream) {
    MH_CHECK_ARG(jobs_device && blocks_device && n_jobs > 0 && n_jobs < 65536 && n_blocks > 0, "mh_colsum_batched: bad arguments");
    hipLaunchKernelGGL(colsum_batched_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device, n_jobs, blocks_device);
    MH_LAUNCH_CHECK();
    return 0;
}
