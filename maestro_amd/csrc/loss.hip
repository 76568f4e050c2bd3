// Masked reconstruction loss at patch layout + its gradient, bias-gradient column sums, casts, fused AdamW.
#include "gemm_common.hpp"
#include "philox.hpp"
#include "../../include/maestro_hip_optim.h"
#include "../../include/maestro_hip_moments.h"
#include <type_traits>

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
            if (CS && masked)
                *colsum += (f32x4){__uint_as_float(pk[0] << 16), __uint_as_float(pk[0] & 0xffff0000u),
                                   __uint_as_float(pk[1] << 16), __uint_as_float(pk[1] & 0xffff0000u)};
        };
        if constexpr (CS) {
#pragma unroll
            for (int j = 0; j < LOSS_CS_NV; ++j)
                if (lane * 4 + 256 * j < PPC) chunk(lane * 4 + 256 * j, &cs[j]);
        } else {
            for (int c = lane * 4; c < PPC; c += 256) chunk(c, nullptr);
        }
    }
    if constexpr (CS) {
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
                acc += (f32x4){__uint_as_float(pk[0] << 16), __uint_as_float(pk[0] & 0xffff0000u),
                               __uint_as_float(pk[1] << 16), __uint_as_float(pk[1] & 0xffff0000u)};
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

// torch.optim.AdamW step (decoupled weight decay, bias correction), 4 elements per thread, grid-stride free.
// fp8 shadows (C5 path): p8 = a flat uint8 buffer with the parameters' offsets; slot_map[i / 64] = scale slot of the weight
// element i belongs to (-1: not an fp8 GEMM operand).  The cast uses the scale derived from the PREVIOUS step's absmax and
// records this step's (delayed scaling: a weight moves by one learning-rate step at a time).
struct Fp8Shadow { uint8_t* p8; const short* slot_map; const float* scale; float* amax; };

// bf16 moments (include/maestro_hip_moments.h): what the stochastic rounding of a launch draws from.  One Philox call per lane
// (= per quad) gives the eight 16-bit words of its four m and four v elements.  The ten rounds are twenty 32 x 32 -> 64-bit
// multiplies (v_mad_u64_u32) and some 60 xor / add per wave beside 5.6 KB of HBM traffic per wave (22 bytes x 256 elements): at
// ~10 B / cycle / CU a CU moves a wave's bytes in ~560 cycles, i.e. each of its four SIMDs has ~2200 cycles per wave it owns, and
// the rounds issue in under half that -- measured, the kernel runs at mh_adamw's bandwidth (profiles/adamw_moments.md).
struct MomentSR { uint32_t k0, k1, step; long elem_base; };
struct NoSR {};

// u = fp32 bits, r < 65536 -> bf16 bits: the magnitude goes up with probability low16(u) / 65536; inf / NaN pass (a NaN stays
// one), a finite value never becomes inf.  On integers: sr_bf16_reference in maestro_amd/hip.py is the same lines.
__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return (u >> 16) | (((u & 0x007fffffu) && !(u & 0x007f0000u)) ? 0x40u : 0u);
    const uint32_t t = u + r;
    return ((t & 0x7f800000u) == 0x7f800000u ? u : t) >> 16;
}

// The ONE update of the library, on how the moments are held: MT = float (m / v fp32, SR = NoSR: mh_adamw and its kin) or bf16_t
// (upcast exactly on load, stored by stochastic rounding, SR = MomentSR); the arithmetic between load and store is the same text.
// returns the fp8 scale slot of this lane's four elements (-1: none) and their absmax in *amax_out
template <typename MT = float, typename SR = NoSR>
__device__ __forceinline__ int adamw_update(float* __restrict__ p, const float* __restrict__ g, MT* __restrict__ m,
                                             MT* __restrict__ v, bf16_t* __restrict__ pb, long n, float lr, float b1, float b2,
                                             float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                             Fp8Shadow f8 = Fp8Shadow{nullptr, nullptr, nullptr, nullptr},
                                             float* amax_out = nullptr, SR sr = SR{}) {
    constexpr bool BF16M = std::is_same<MT, bf16_t>::value;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return -1;
    // Every stream of this kernel is touched once per step (30 bytes per parameter, 5.3 GB on C3): nontemporal loads AND stores keep
    // them from displacing each other in the L2 / Infinity Cache -- 925 -> 858 us on 176 M parameters (5.7 -> 6.2 TB/s); either half
    // alone gains 1 %, two or four quads per lane nothing (scripts/micro_adamw.hip, profiles/r05_experiments.md).
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i)) * gscale;
    f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + i));
    f32x4 mv, vv;
    if constexpr (BF16M) {
        const u32x2 m2 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(m + i));
        const u32x2 v2 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(v + i));
        mv = (f32x4){__uint_as_float(m2[0] << 16), __uint_as_float(m2[0] & 0xffff0000u),
                     __uint_as_float(m2[1] << 16), __uint_as_float(m2[1] & 0xffff0000u)};
        vv = (f32x4){__uint_as_float(v2[0] << 16), __uint_as_float(v2[0] & 0xffff0000u),
                     __uint_as_float(v2[1] << 16), __uint_as_float(v2[1] & 0xffff0000u)};
    } else {
        mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m + i));
        vv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v + i));
    }
    // Every rounding is written out: which products fuse into an fma is the text below, not the optimiser's choice per
    // instantiation (left to it, the bf16 form packed b2 * v with (1 - b2) * g and ADDED, where the fp32 form fused) -- both forms
    // give the same p, m and v bits from the same operands.  The fused places are the ones mh_adamw has always compiled to.
    {
#pragma clang fp contract(off)
        const float decay = __builtin_fmaf(-lr, wd, 1.f), rate = lr / bc1, c1 = 1.f - b1, c2 = 1.f - b2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mv[e] = __builtin_fmaf(c1, gv[e], b1 * mv[e]);
            vv[e] = __builtin_fmaf(c2 * gv[e], gv[e], b2 * vv[e]);
            const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
            pv[e] = __builtin_fmaf(decay, pv[e], -(rate * (mv[e] / denom)));
        }
    }
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(p + i));
    if constexpr (BF16M) {
        const u32x4 w = philox4x32_10((uint32_t)((sr.elem_base + i) >> 2), sr.step, 0u, MH_ADAMW_SR_TAG, sr.k0, sr.k1);
        const u32x2 m2 = {sr_bf16(mv[0], w[0] & 0xffffu) | sr_bf16(mv[1], w[0] >> 16) << 16,
                          sr_bf16(mv[2], w[1] & 0xffffu) | sr_bf16(mv[3], w[1] >> 16) << 16};
        const u32x2 v2 = {sr_bf16(vv[0], w[2] & 0xffffu) | sr_bf16(vv[1], w[2] >> 16) << 16,
                          sr_bf16(vv[2], w[3] & 0xffffu) | sr_bf16(vv[3], w[3] >> 16) << 16};
        __builtin_nontemporal_store(m2, reinterpret_cast<u32x2*>(m + i));
        __builtin_nontemporal_store(v2, reinterpret_cast<u32x2*>(v + i));
    } else {
        __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(m + i));
        __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v + i));
    }
    if (pb) {
        u32x2 pk = {pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3])};
        __builtin_nontemporal_store(pk, reinterpret_cast<u32x2*>(pb + i));
    }
    if (f8.p8) {
        const int slot = f8.slot_map[i >> 6];
        if (slot >= 0) {
            const float s8 = f8.scale[slot];
            float mx = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = amax_fold(mx, pv[e]);     // keeps inf / NaN (common.hpp)
            __builtin_nontemporal_store(pack_e4m3x4(pv, s8), reinterpret_cast<uint32_t*>(f8.p8 + i));
            *amax_out = mx;
            return slot;
        }
    }
    return -1;
}
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ pb, long n, float lr, float b1,
                                                    float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
    adamw_update(p, g, m, v, pb, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
}
__global__ __launch_bounds__(256) void adamw_fp8_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ pb, long n, float lr, float b1,
                                                        float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                                        Fp8Shadow f8) {
    // absmax: 80 M lanes adding to one word per tensor took 22 ms per step -- fold per wave and per workgroup first (a workgroup
    // spans 1024 elements, i.e. one tensor except at the few tensor boundaries), then one add into a sub-slot of the amax row
    __shared__ float red_mx[4];
    __shared__ int red_slot[4];
    float mx = 0.f;
    const int slot = adamw_update(p, g, m, v, pb, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, f8, &mx);
    const int w = threadIdx.x >> 6;
    const int slot0 = __builtin_amdgcn_readfirstlane(slot);      // first ACTIVE lane: all lanes are active here
    const bool uniform = __all(slot == slot0);
    if (uniform) {
        mx = wave_amax(mx);
    } else if (slot >= 0 && amax_nonzero(mx)) {
        atomic_max_pos(f8.amax + (size_t)slot * MH_FP8_AMAX_PITCH, mx);   // a wave across a tensor boundary: rare
    }
    if ((threadIdx.x & 63) == 0) { red_mx[w] = uniform ? mx : 0.f; red_slot[w] = uniform ? slot0 : -1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (red_slot[0] == red_slot[1] && red_slot[0] == red_slot[2] && red_slot[0] == red_slot[3]) {
            const float m4 = amax_fold(amax_fold(amax_fold(red_mx[0], red_mx[1]), red_mx[2]), red_mx[3]);
            if (red_slot[0] >= 0 && amax_nonzero(m4)) atomic_max_pos(f8.amax + (size_t)red_slot[0] * MH_FP8_AMAX_PITCH, m4);
        } else {
            for (int k = 0; k < 4; ++k)
                if (red_slot[k] >= 0 && amax_nonzero(red_mx[k])) atomic_max_pos(f8.amax + (size_t)red_slot[k] * MH_FP8_AMAX_PITCH, red_mx[k]);
        }
    }
}
// per-step scalars from device memory: the launch is captured once and replayed with new values (see mh_adamw_dev)
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ pb, long n, float b1, float b2,
                                                        float eps, float wd, const float* __restrict__ hyper) {
    if (hyper[4] == 0.f) return;
    adamw_update(p, g, m, v, pb, n, hyper[0], b1, b2, eps, wd, hyper[1], hyper[2], hyper[3]);
}

// Parameter groups (include/maestro_hip_optim.h): group_of[i >> 6] names the group of element i, lr_scale / wd are 256-entry
// tables, so every value of the map byte indexes inside them.  A lane's four elements lie in one 64-element block, a wave spans
// four blocks: the group is per lane, not per wave.  The map (1 byte per 64 parameters) and the tables (2 KiB) are re-read by every
// workgroup beside 30 bytes per parameter of nontemporal traffic: PLAIN loads, which the vector L1 serves (nontemporal loads
// bypass it), while the streams above leave no line behind that could displace them.  lr_g is one explicitly rounded product:
// what follows in adamw_update sees the float mh_adamw would have been handed for this group.
template <typename MT = float, typename SR = NoSR>
__device__ __forceinline__ void adamw_group_update(float* __restrict__ p, const float* __restrict__ g, MT* __restrict__ m,
                                                   MT* __restrict__ v, bf16_t* __restrict__ pb,
                                                   const uint8_t* __restrict__ group_of, const float* __restrict__ lr_scale,
                                                   const float* __restrict__ wd, long n, float lr, float b1, float b2, float eps,
                                                   float bc1, float bc2_sqrt, float gscale, SR sr = SR{}) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;                      // before the map is read: its last byte is the one of element n - 1
    const unsigned grp = group_of[i >> 6];
    const float lr_g = __fmul_rn(lr, lr_scale[grp]);
    adamw_update(p, g, m, v, pb, n, lr_g, b1, b2, eps, wd[grp], bc1, bc2_sqrt, gscale, Fp8Shadow{nullptr, nullptr, nullptr, nullptr},
                 nullptr, sr);
}
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, bf16_t* __restrict__ pb,
                                                           const uint8_t* __restrict__ group_of, const float* __restrict__ lr_scale,
                                                           const float* __restrict__ wd, long n, float lr, float b1, float b2,
                                                           float eps, float bc1, float bc2_sqrt, float gscale) {
    adamw_group_update(p, g, m, v, pb, group_of, lr_scale, wd, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale);
}
__global__ __launch_bounds__(256) void adamw_groups_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v, bf16_t* __restrict__ pb,
                                                               const uint8_t* __restrict__ group_of,
                                                               const float* __restrict__ lr_scale, const float* __restrict__ wd,
                                                               long n, float b1, float b2, float eps,
                                                               const float* __restrict__ hyper) {
    if (hyper[4] == 0.f) return;
    adamw_group_update(p, g, m, v, pb, group_of, lr_scale, wd, n, hyper[0], b1, b2, eps, hyper[1], hyper[2], hyper[3]);
}

// bf16 moments (include/maestro_hip_moments.h): the four launches above with m / v as bf16 and the rounding draws' key, step and
// layout offset.  The device forms take the step from the low 32 bits of *step_dev (the guard's MhGuardState.t).
__global__ __launch_bounds__(256) void adamw_bf16m_kernel(float* __restrict__ p, const float* __restrict__ g, bf16_t* __restrict__ m,
                                                          bf16_t* __restrict__ v, bf16_t* __restrict__ pb, long n, float lr,
                                                          float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                          float gscale, MomentSR sr) {
    adamw_update(p, g, m, v, pb, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, Fp8Shadow{nullptr, nullptr, nullptr, nullptr}, nullptr, sr);
}
__global__ __launch_bounds__(256) void adamw_bf16m_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              bf16_t* __restrict__ m, bf16_t* __restrict__ v, bf16_t* __restrict__ pb,
                                                              long n, float b1, float b2, float eps, float wd,
                                                              const float* __restrict__ hyper, const long long* __restrict__ step_dev,
                                                              MomentSR sr) {
    if (hyper[4] == 0.f) return;
    sr.step = (uint32_t)*step_dev;
    adamw_update(p, g, m, v, pb, n, hyper[0], b1, b2, eps, wd, hyper[1], hyper[2], hyper[3], Fp8Shadow{nullptr, nullptr, nullptr, nullptr},
                 nullptr, sr);
}
__global__ __launch_bounds__(256) void adamw_groups_bf16m_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 bf16_t* __restrict__ m, bf16_t* __restrict__ v, bf16_t* __restrict__ pb,
                                                                 const uint8_t* __restrict__ group_of,
                                                                 const float* __restrict__ lr_scale, const float* __restrict__ wd,
                                                                 long n, float lr, float b1, float b2, float eps, float bc1,
                                                                 float bc2_sqrt, float gscale, MomentSR sr) {
    adamw_group_update(p, g, m, v, pb, group_of, lr_scale, wd, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale, sr);
}
__global__ __launch_bounds__(256) void adamw_groups_bf16m_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                     bf16_t* __restrict__ m, bf16_t* __restrict__ v,
                                                                     bf16_t* __restrict__ pb, const uint8_t* __restrict__ group_of,
                                                                     const float* __restrict__ lr_scale, const float* __restrict__ wd,
                                                                     long n, float b1, float b2, float eps,
                                                                     const float* __restrict__ hyper,
                                                                     const long long* __restrict__ step_dev, MomentSR sr) {
    if (hyper[4] == 0.f) return;
    sr.step = (uint32_t)*step_dev;
    adamw_group_update(p, g, m, v, pb, group_of, lr_scale, wd, n, hyper[0], b1, b2, eps, hyper[1], hyper[2], hyper[3], sr);
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

extern "C" int mh_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float lr, float b1, float b2,
                        float eps, float wd, int step, float grad_scale, void* stream) {
    MH_CHECK_ARG(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "mh_adamw: bad arguments (n %% 4 == 0, step >= 1)");
    const float bc1 = 1.f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, n, lr,
                       b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_fp8(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_fp8, const short* slot_map,
                            const float* scale, float* amax, long n, float lr, float b1, float b2, float eps, float wd, int step,
                            float grad_scale, void* stream) {
    MH_CHECK_ARG(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "mh_adamw_fp8: bad arguments (n %% 4 == 0, step >= 1)");
    MH_CHECK_ARG(p_fp8 && slot_map && scale && amax && ((uintptr_t)p_fp8 % 4) == 0, "mh_adamw_fp8: fp8 shadow, slot map, scale and amax tables are required");
    const float bc1 = 1.f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
    hipLaunchKernelGGL(adamw_fp8_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, n, lr,
                       b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, Fp8Shadow{(uint8_t*)p_fp8, slot_map, scale, amax});
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_dev(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float b1, float b2, float eps,
                            float wd, const float* hyper, void* stream) {
    MH_CHECK_ARG(p && g && m && v && hyper && n > 0 && n % 4 == 0, "mh_adamw_dev: bad arguments (n %% 4 == 0)");
    hipLaunchKernelGGL(adamw_dev_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16,
                       n, b1, b2, eps, wd, hyper);
    MH_LAUNCH_CHECK();
    return 0;
}

static bool adamw_groups_aligned(const void* p, const void* g, const void* m, const void* v, const void* p_bf16) {
    return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) == 0 && ((uintptr_t)p_bf16 % 8) == 0;
}

extern "C" int mh_adamw_groups(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                               const float* lr_scale, const float* wd, long n, float lr, float b1, float b2, float eps, int step,
                               float grad_scale, void* stream) {
    MH_CHECK_ARG(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "mh_adamw_groups: bad arguments (n %% 4 == 0, step >= 1)");
    MH_CHECK_ARG(group_of && lr_scale && wd, "mh_adamw_groups: the group map and both tables are required (null pointer)");
    MH_CHECK_ARG(adamw_groups_aligned(p, g, m, v, p_bf16), "mh_adamw_groups: p, g, m, v must be 16-byte, p_bf16 8-byte aligned");
    const float bc1 = 1.f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16,
                       group_of, lr_scale, wd, n, lr, b1, b2, eps, bc1, bc2_sqrt, grad_scale);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                                   const float* lr_scale, const float* wd, long n, float b1, float b2, float eps,
                                   const float* hyper, void* stream) {
    MH_CHECK_ARG(p && g && m && v && hyper && n > 0 && n % 4 == 0, "mh_adamw_groups_dev: bad arguments (n %% 4 == 0)");
    MH_CHECK_ARG(group_of && lr_scale && wd, "mh_adamw_groups_dev: the group map and both tables are required (null pointer)");
    MH_CHECK_ARG(adamw_groups_aligned(p, g, m, v, p_bf16), "mh_adamw_groups_dev: p, g, m, v must be 16-byte, p_bf16 8-byte aligned");
    hipLaunchKernelGGL(adamw_groups_dev_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       (bf16_t*)p_bf16, group_of, lr_scale, wd, n, b1, b2, eps, hyper);
    MH_LAUNCH_CHECK();
    return 0;
}

// ---- bf16 moments (include/maestro_hip_moments.h)
static bool adamw_bf16m_aligned(const void* p, const void* g, const void* m16, const void* v16, const void* p_bf16) {
    return (((uintptr_t)p | (uintptr_t)g) % 16) == 0 && (((uintptr_t)m16 | (uintptr_t)v16 | (uintptr_t)p_bf16) % 8) == 0;
}
#define MH_ADAMW_BF16M_CHECK(name, block, extra)                                                                                    \
    MH_CHECK_ARG(p && g && m16 && v16 && (extra) && n > 0 && n % 4 == 0,                                                           \
                 name ": bad arguments (null pointer, n > 0, n %% 4 == 0, step >= 1)");                                              \
    MH_CHECK_ARG(elem_base >= 0 && elem_base % block == 0, name ": elem_base %ld must be a non-negative multiple of %d", elem_base, block); \
    MH_CHECK_ARG(adamw_bf16m_aligned(p, g, m16, v16, p_bf16), name ": p, g must be 16-byte, m16, v16, p_bf16 8-byte aligned")
static MomentSR moment_sr(uint64_t seed, long long step, long elem_base) {
    return MomentSR{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)step, elem_base};
}

extern "C" int mh_adamw_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed,
                              float lr, float b1, float b2, float eps, float wd, int step, float grad_scale, void* stream) {
    MH_ADAMW_BF16M_CHECK("mh_adamw_bf16m", 4, step >= 1);
    const float bc1 = 1.f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
    hipLaunchKernelGGL(adamw_bf16m_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, (bf16_t*)m16,
                       (bf16_t*)v16, (bf16_t*)p_bf16, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, moment_sr(seed, step, elem_base));
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base,
                                  uint64_t seed, float b1, float b2, float eps, float wd, const float* hyper,
                                  const long long* step_dev, void* stream) {
    MH_ADAMW_BF16M_CHECK("mh_adamw_bf16m_dev", 4, hyper && step_dev);
    hipLaunchKernelGGL(adamw_bf16m_dev_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, (bf16_t*)m16,
                       (bf16_t*)v16, (bf16_t*)p_bf16, n, b1, b2, eps, wd, hyper, step_dev, moment_sr(seed, 0, elem_base));
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_groups_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                                     const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float lr,
                                     float b1, float b2, float eps, int step, float grad_scale, void* stream) {
    MH_ADAMW_BF16M_CHECK("mh_adamw_groups_bf16m", MH_ADAMW_GROUP_BLOCK, step >= 1);
    MH_CHECK_ARG(group_of && lr_scale && wd, "mh_adamw_groups_bf16m: the group map and both tables are required (null pointer)");
    const float bc1 = 1.f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
    hipLaunchKernelGGL(adamw_groups_bf16m_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, (bf16_t*)m16,
                       (bf16_t*)v16, (bf16_t*)p_bf16, group_of, lr_scale, wd, n, lr, b1, b2, eps, bc1, bc2_sqrt, grad_scale,
                       moment_sr(seed, step, elem_base));
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_adamw_groups_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16,
                                         const unsigned char* group_of, const float* lr_scale, const float* wd, long n,
                                         long elem_base, uint64_t seed, float b1, float b2, float eps, const float* hyper,
                                         const long long* step_dev, void* stream) {
    MH_ADAMW_BF16M_CHECK("mh_adamw_groups_bf16m_dev", MH_ADAMW_GROUP_BLOCK, hyper && step_dev);
    MH_CHECK_ARG(group_of && lr_scale && wd, "mh_adamw_groups_bf16m_dev: the group map and both tables are required (null pointer)");
    hipLaunchKernelGGL(adamw_groups_bf16m_dev_kernel, dim3(ceil_div(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, g, (bf16_t*)m16,
                       (bf16_t*)v16, (bf16_t*)p_bf16, group_of, lr_scale, wd, n, b1, b2, eps, hyper, step_dev,
                       moment_sr(seed, 0, elem_base));
    MH_LAUNCH_CHECK();
    return 0;
}
