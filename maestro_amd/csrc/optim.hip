// Fused AdamW over a flat parameter buffer: one update body, one kernel template over how the moments are held, whether
// parameter groups apply and where the per-step scalars live, the fp8-shadow kernel, and one host launcher for all of them.
#include "gemm_common.hpp"
#include "philox.hpp"
#include "../../include/maestro_hip.h"
#include <type_traits>

namespace {

// torch.optim.AdamW step (decoupled weight decay, bias correction), 4 elements per thread, grid-stride free.
// fp8 shadows (C5 path): p8 = a flat uint8 buffer with the parameters' offsets; slot_map[i / 64] = scale slot of the weight
// element i belongs to (-1: not an fp8 GEMM operand).  The cast uses the scale derived from the PREVIOUS step's absmax and
// records this step's (delayed scaling: a weight moves by one learning-rate step at a time).
struct Fp8Shadow { uint8_t* p8; const short* slot_map; const float* scale; float* amax; };

// bf16 moments (mh_adamw_bf16m and its kin): what the stochastic rounding of a launch draws from.  One Philox call per lane
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

// Parameter groups (mh_adamw_groups and its kin): group_of[i >> 6] names the group of element i, lr_scale / wd are 256-entry
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

// The eight forms {fp32 | bf16 moments} x {plain | grouped} x {host | device scalars} of the update.  An instantiation reads only
// the arguments of its form; the launcher passes null / zero for the rest.
//   GROUPED: group_of, lr_scale and wd_of replace the one wd.
//   DEV: the per-step scalars come from device memory, so that the launch is captured once and replayed with new values:
//        hyper = {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active}; with active == 0 the kernel returns before it touches anything
//        else.  With bf16 moments the rounding draws' step is the low 32 bits of *step_dev (the guard's MhGuardState.t).
//   MT = bf16_t: sr carries the draws' key, step and layout offset.
template <typename MT, bool GROUPED, bool DEV>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, MT* __restrict__ m,
                                                    MT* __restrict__ v, bf16_t* __restrict__ pb,
                                                    const uint8_t* __restrict__ group_of, const float* __restrict__ lr_scale,
                                                    const float* __restrict__ wd_of, long n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2_sqrt, float gscale,
                                                    const float* __restrict__ hyper, const long long* __restrict__ step_dev,
                                                    MomentSR sr) {
    constexpr bool BF16M = std::is_same<MT, bf16_t>::value;
    if constexpr (DEV) {
        if (hyper[4] == 0.f) return;
        lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2], gscale = hyper[3];
        if constexpr (BF16M) sr.step = (uint32_t)*step_dev;
    }
    auto update = [&](auto draws) {
        if constexpr (GROUPED) adamw_group_update(p, g, m, v, pb, group_of, lr_scale, wd_of, n, lr, b1, b2, eps, bc1, bc2_sqrt, gscale, draws);
        else adamw_update(p, g, m, v, pb, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, Fp8Shadow{nullptr, nullptr, nullptr, nullptr}, nullptr, draws);
    };
    if constexpr (BF16M) update(sr); else update(NoSR{});
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

// What an entry point has beyond p, g, m, v, p_bf16, n, b1, b2, eps and the stream; what its form does not have stays null / zero.
struct AdamwArgs {
    const unsigned char* group_of = nullptr; const float* lr_scale = nullptr; const float* wd_of = nullptr;   // GROUPED
    float wd = 0.f;                                                                                           // not GROUPED
    float lr = 0.f, grad_scale = 0.f; int step = 0;                                                           // host scalars
    const float* hyper = nullptr; const long long* step_dev = nullptr;                                        // DEV (step_dev: bf16 moments)
    long elem_base = 0; uint64_t seed = 0;                                                                    // bf16 moments
    const Fp8Shadow* f8 = nullptr;                                                                            // mh_adamw_fp8
};

// Host side of all nine entries: the checks, the float32 bias corrections (powf / sqrtf: hip.adamw_bias_corrections mirrors them
// bit for bit), the rounding draws' key, the grid and the launch.  ``name``: the entry's own name, for its messages.
// ``aligned``: the entry refuses misaligned operands (mh_adamw, mh_adamw_dev and mh_adamw_fp8 never did) -- p, g and fp32 moments
// 16-byte, bf16 moments and the bf16 shadow 8-byte.
template <typename MT, bool GROUPED, bool DEV>
int launch_adamw(const char* name, bool aligned, float* p, const float* g, void* m, void* v, void* p_bf16, long n, float b1,
                 float b2, float eps, const AdamwArgs& a, void* stream) {
    constexpr bool BF16M = std::is_same<MT, bf16_t>::value;
    MH_CHECK_ARG(p && g && m && v && n > 0 && n % 4 == 0 && (DEV ? a.hyper && (!BF16M || a.step_dev) : a.step >= 1),
                 "%s: bad arguments (null pointer, n > 0, n %% 4 == 0%s)", name, DEV ? "" : ", step >= 1");
    if (GROUPED) MH_CHECK_ARG(a.group_of && a.lr_scale && a.wd_of, "%s: the group map and both tables are required (null pointer)", name);
    const int block = GROUPED ? MH_ADAMW_GROUP_BLOCK : 4;
    if (BF16M) MH_CHECK_ARG(a.elem_base >= 0 && a.elem_base % block == 0, "%s: elem_base %ld must be a non-negative multiple of %d", name, a.elem_base, block);
    const uintptr_t pg = (uintptr_t)p | (uintptr_t)g, mv = (uintptr_t)m | (uintptr_t)v, pb = (uintptr_t)p_bf16;
    MH_CHECK_ARG(!aligned || (BF16M ? pg % 16 == 0 && (mv | pb) % 8 == 0 : (pg | mv) % 16 == 0 && pb % 8 == 0),
                 "%s: p, g%s must be 16-byte, %sp_bf16 8-byte aligned", name, BF16M ? "" : ", m, v", BF16M ? "m16, v16, " : "");
    float lr = a.lr, bc1 = 0.f, bc2_sqrt = 0.f;
    if (!DEV) {
        bc1 = 1.f - powf(b1, (float)a.step);
        bc2_sqrt = sqrtf(1.f - powf(b2, (float)a.step));
    }
    const dim3 grid(ceil_div(n, 1024)), block_dim(256);
    if (a.f8) {
        hipLaunchKernelGGL(adamw_fp8_kernel, grid, block_dim, 0, (hipStream_t)stream, p, g, (float*)m, (float*)v, (bf16_t*)p_bf16, n, lr,
                           b1, b2, eps, a.wd, bc1, bc2_sqrt, a.grad_scale, *a.f8);
    } else {
        const MomentSR sr{(uint32_t)(a.seed & 0xFFFFFFFFu), (uint32_t)(a.seed >> 32), (uint32_t)a.step, a.elem_base};
        hipLaunchKernelGGL((adamw_kernel<MT, GROUPED, DEV>), grid, block_dim, 0, (hipStream_t)stream, p, g, (MT*)m, (MT*)v,
                           (bf16_t*)p_bf16, a.group_of, a.lr_scale, a.wd_of, n, lr, b1, b2, eps, a.wd, bc1, bc2_sqrt, a.grad_scale,
                           a.hyper, a.step_dev, sr);
    }
    MH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int mh_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float lr, float b1, float b2,
                        float eps, float wd, int step, float grad_scale, void* stream) {
    AdamwArgs a; a.wd = wd, a.lr = lr, a.step = step, a.grad_scale = grad_scale;
    return launch_adamw<float, false, false>("mh_adamw", false, p, g, m, v, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_fp8(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_fp8, const short* slot_map,
                            const float* scale, float* amax, long n, float lr, float b1, float b2, float eps, float wd, int step,
                            float grad_scale, void* stream) {
    MH_CHECK_ARG(p_fp8 && slot_map && scale && amax && ((uintptr_t)p_fp8 % 4) == 0, "mh_adamw_fp8: fp8 shadow, slot map, scale and amax tables are required");
    const Fp8Shadow f8{(uint8_t*)p_fp8, slot_map, scale, amax};
    AdamwArgs a; a.wd = wd, a.lr = lr, a.step = step, a.grad_scale = grad_scale, a.f8 = &f8;
    return launch_adamw<float, false, false>("mh_adamw_fp8", false, p, g, m, v, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_dev(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float b1, float b2, float eps,
                            float wd, const float* hyper, void* stream) {
    AdamwArgs a; a.wd = wd, a.hyper = hyper;
    return launch_adamw<float, false, true>("mh_adamw_dev", false, p, g, m, v, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_groups(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                               const float* lr_scale, const float* wd, long n, float lr, float b1, float b2, float eps, int step,
                               float grad_scale, void* stream) {
    AdamwArgs a; a.group_of = group_of, a.lr_scale = lr_scale, a.wd_of = wd, a.lr = lr, a.step = step, a.grad_scale = grad_scale;
    return launch_adamw<float, true, false>("mh_adamw_groups", true, p, g, m, v, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                                   const float* lr_scale, const float* wd, long n, float b1, float b2, float eps,
                                   const float* hyper, void* stream) {
    AdamwArgs a; a.group_of = group_of, a.lr_scale = lr_scale, a.wd_of = wd, a.hyper = hyper;
    return launch_adamw<float, true, true>("mh_adamw_groups_dev", true, p, g, m, v, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed,
                              float lr, float b1, float b2, float eps, float wd, int step, float grad_scale, void* stream) {
    AdamwArgs a; a.wd = wd, a.lr = lr, a.step = step, a.grad_scale = grad_scale, a.elem_base = elem_base, a.seed = seed;
    return launch_adamw<bf16_t, false, false>("mh_adamw_bf16m", true, p, g, m16, v16, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base,
                                  uint64_t seed, float b1, float b2, float eps, float wd, const float* hyper,
                                  const long long* step_dev, void* stream) {
    AdamwArgs a; a.wd = wd, a.hyper = hyper, a.step_dev = step_dev, a.elem_base = elem_base, a.seed = seed;
    return launch_adamw<bf16_t, false, true>("mh_adamw_bf16m_dev", true, p, g, m16, v16, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_groups_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                                     const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float lr,
                                     float b1, float b2, float eps, int step, float grad_scale, void* stream) {
    AdamwArgs a; a.group_of = group_of, a.lr_scale = lr_scale, a.wd_of = wd, a.lr = lr, a.step = step, a.grad_scale = grad_scale;
    a.elem_base = elem_base, a.seed = seed;
    return launch_adamw<bf16_t, true, false>("mh_adamw_groups_bf16m", true, p, g, m16, v16, p_bf16, n, b1, b2, eps, a, stream);
}

extern "C" int mh_adamw_groups_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16,
                                         const unsigned char* group_of, const float* lr_scale, const float* wd, long n,
                                         long elem_base, uint64_t seed, float b1, float b2, float eps, const float* hyper,
                                         const long long* step_dev, void* stream) {
    AdamwArgs a; a.group_of = group_of, a.lr_scale = lr_scale, a.wd_of = wd, a.hyper = hyper, a.step_dev = step_dev;
    a.elem_base = elem_base, a.seed = seed;
    return launch_adamw<bf16_t, true, true>("mh_adamw_groups_bf16m_dev", true, p, g, m16, v16, p_bf16, n, b1, b2, eps, a, stream);
}
