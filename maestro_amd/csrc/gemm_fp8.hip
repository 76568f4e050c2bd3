// fp8 MFMA GEMM for gfx950 (BASELINE configs[4]: "ViT-Base MAE fp8 MFMA path"): C = descale_a * descale_b * A8 B8^T with
// the fused epilogues of mh_gemm_bf16, operands OCP e4m3 (weights, activations) or e5m2 (gradients), fp32 accumulation.
//
//   MFMA  v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (E8M0 127): the block-scaled form is the one that runs at
//         the fp8 rate on CDNA4 (K = 128 per instruction, 2x the bf16 FLOP per clock; the plain fp8 16x16x32 form runs at the
//         bf16 rate).  Per-TENSOR scaling: the quantisers (quant.hip) multiply by a power-of-two scale kept on the device, the
//         epilogue multiplies the accumulators by the two descale factors.
//   tile  256 x 256 x 128 per 512-thread workgroup (8 waves, 2 x 4, 128 x 64 per wave = 8 x 4 MFMA tiles) or 128 x 128 x 128
//         per 256-thread workgroup (small problems, two workgroups per CU), both operands
//         K-minor ("NT": the dgrad uses a transposed fp8 weight shadow instead of a K-major read), so per output FLOP the
//         kernel moves HALF the operand bytes of the bf16 kernels through L2 -> LDS -- the path that bounds those kernels.
//   LDS   2-stage ring of (A + B tile: 64 KiB / 32 KiB), operands by LDS-DMA (buffer_load ... lds, 8 one-KiB pieces per wave and K
//         step), one raw s_barrier per K step; 128-byte rows, 16-byte chunk position p holds source chunk p ^ (row & 7)
//         (swizzle on the per-lane SOURCE offset and again on the fragment reads: conflict-free ds_read_b128).
//   operand map (checked with exact integer data, tests/test_fp8_gpu.py): lane l holds row (l & 15), K block (l >> 4) of 32
//         consecutive bytes; C / D as every 16 x 16 MFMA: column l & 15, rows 4 (l >> 4) + r.
//   MX    (mh_gemm_mx, template flag MX of the same body): OCP MX block scales instead of the unit ones.  Each MFMA takes one
//         E8M0 byte per lane and operand: A's scale of row (l & 15), block 4t + (l >> 4), and B's likewise (the weight fragment is
//         the builtin's FIRST source, so its scale is the first scale operand); the fragments are read in the MFMA's own K order
//         (read_frag8<true>: lane group g holds 16-byte chunks g and g + 4), checked with exact data in tests/test_mx_gpu.py.
//         The scales ride in the LDS ring: per stage a [BM][4]-byte A image and a [BN][4]-byte B image (one u32 = one K step of
//         a row), filled by ONE 4-byte-per-lane LDS-DMA load per wave and K step (rows 64 w .. 64 w + 63: (BM + BN) / 64 = the
//         wave count on every tile), counted in the same vmcnt waits as the operand pieces, and read back as one byte per lane and
//         fragment.  Ring: 132 KiB on the 256 and 128D tiles, 66 KiB on the 128 tile (two workgroups per CU still fit in
//         160 KiB).  Chosen over per-lane global loads of the scale bytes WITHOUT measuring that alternative: those would need
//         a register double buffer whose rotation forces a vmcnt wait per step (a copy of a register with a load in flight is a
//         use); in the ring the scales arrive under the same wait as the operands and cost 4 + MT ds_read_u8 per lane and step.
//         Measured on the C5 step (profiles/mx_observed_errors.md): 6.70 ms of MX GEMM per step against 6.36 ms per-tensor
//         (+5 %), same tiles and launches.  Epilogue: no descale, c8 block-scaled (gemm_common.hpp).
#include "gemm_common.hpp"

namespace {

constexpr int BK8 = 128;

// Tile geometry: WM x WN waves, each a (16 MT) x 64 accumulator block.
//   <2,4,8> 256 x 256, 512 threads, 128 KiB ring, one workgroup per CU: the large decoder / joint problems
//   <2,2,4> 128 x 128, 256 threads,  64 KiB ring, TWO workgroups per CU (one's epilogue overlaps the other's main loop): the
//           per-group encoder problems of C5 (M = 512 .. 4608 token rows: 54 .. 216 tiles of 256 x 256 would leave most of the
//           256 CUs idle).  At one byte per element this tile moves the same operand bytes per FLOP as the bf16 256 x 256 tile.
//   <2,2,4,4> the same 128 x 128 tile with a FOUR-stage ring (128 KiB, one workgroup per CU, three K steps in flight) for long-K
//           launches with at most one tile per CU anyway: measured (scripts/bench_fp8_gemm.py, isolated) 4608 x 768 x 3072:
//           24.2 -> 21.9 us, 4608 x 512 x 3072: 23.2 -> 20.9; but 3-4 % SLOWER below 128 tiles or at K = 768 (512 x 768 x 3072:
//           18.8 -> 19.6 us -- those launches are bound by the exposed wait -> barrier -> fragment-read -> MFMA chain of a
//           single wave per SIMD, 0.8 us per K step, not by the DMA round trip), hence the narrow dispatch rule below.
template <int WM_, int WN_, int MT_, int S8_ = 2>
struct Tile8 {
    static constexpr int WM = WM_, WN = WN_, MT = MT_, S8 = S8_;
    static constexpr int BM = 16 * MT * WM, BN = 64 * WN, NW = WM * WN, NT = 64 * NW;
    static constexpr int A_BYTES = BM * BK8, B_BYTES = BN * BK8, STAGE_BYTES = A_BYTES + B_BYTES, LDS_BYTES = S8 * STAGE_BYTES;
    static constexpr int PA = A_BYTES / 1024 / NW, PB = B_BYTES / 1024 / NW;   // one-KiB DMA pieces per wave and K step
    static constexpr int MIN_WAVES = NT >= 512 ? 2 : 2;                        // waves per SIMD the register budget must allow
    static_assert(PA * NW * 1024 == A_BYTES && PB * NW * 1024 == B_BYTES, "pieces must divide evenly over the waves");
    static_assert(LDS_BYTES >= NW * 32 * 68 * 4, "the ring doubles as epilogue staging");
    static_assert((BM + BN) / 64 == NW, "MX: one 256-byte scale piece per wave and K step");
};
// the ring of one instantiation: MX stages also hold the [BM + BN][4]-byte scale images of the K step
template <class T, bool MX>
struct Ring8 {
    static constexpr int SC_BYTES = MX ? 4 * (T::BM + T::BN) : 0, STAGE_BYTES = T::STAGE_BYTES + SC_BYTES;
    static constexpr int LDS_BYTES = T::S8 * STAGE_BYTES, PS = MX ? 1 : 0;     // PS: scale pieces per wave and K step
};
typedef Tile8<2, 4, 8> T8_256;
typedef Tile8<2, 2, 4> T8_128;
typedef Tile8<2, 2, 4, 4> T8_128D;

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((address_space(3))) void lds_void8;

// fragment of rows (rc0 + lane & 15): 32 bytes along k = 32 (lane >> 4) + j.  MX: the scaled MFMA reads byte j of lane group g as
// k = 64 (j >> 4) + 16 g + (j & 15) -- its scale for block b (k = 32 b .. 32 b + 31) comes from lane group b (measured: one-hot
// data, a distinct exponent per row and block) -- so that lane group g holds the 16-byte chunks g and g + 4 of the row: the
// hardware's K order is then the memory order and block b of the scale matrix is the MFMA's block b.  (Without block scales the
// two orders give the same sums; the per-tensor path keeps its chunks 2g, 2g + 1.)
template <bool MX = false>
__device__ __forceinline__ i32x8 read_frag8(const unsigned char* img, int rc0) {
    const int l = threadIdx.x & 63, row = rc0 + (l & 15), g = l >> 4, sw = row & 7;
    const int c0 = MX ? g : 2 * g, c1 = MX ? g + 4 : 2 * g + 1;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(img + row * 128 + ((c0 ^ sw) << 4));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(img + row * 128 + ((c1 ^ sw) << 4));
    return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// A_E5M2: the A operand (activations / gradients, the MFMA's second source here) is e5m2 instead of e4m3
// (Body as a __device__ function template, the kernel a thin wrapper: the host pass of hipcc 7.2 does not emit the launch stub
// of a kernel template whose own body holds the LDS-DMA builtin inside a lambda.)
template <class T, bool A_E5M2, bool MX>
__device__ __forceinline__ void gemm_fp8_body(const GemmParams& p, unsigned char* smem) {
    constexpr int MT = T::MT, NW = T::NW, PA = T::PA, PB = T::PB, PS = Ring8<T, MX>::PS, STAGE = Ring8<T, MX>::STAGE_BYTES;
    const int nwg = p.tiles_m * p.tiles_n;
    const int id = xcd_remap(blockIdx.x, nwg);
    int tile_m, tile_n;
    raster_tile<4>(p, id, tile_m, tile_n);
    const int m0 = tile_m * T::BM, n0 = tile_n * T::BN;
    const int nk = p.K / BK8;

    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int wm = (w / T::WN) * (16 * MT), wn = (w % T::WN) * 64;
    const __amdgpu_buffer_rsrc_t ra = buffer_rsrc(p.A, (int)p.a_bytes);
    const __amdgpu_buffer_rsrc_t rb = buffer_rsrc(p.B, (int)p.b_bytes);
    int va[PA], vb[PB];   // per-lane source byte offsets of this wave's pieces (piece = 8 rows x 128 B), k = 0
#pragma unroll
    for (int h = 0; h < PA; ++h) {
        const int row = (w + NW * h) * 8 + (l >> 3), pos = l & 7;
        va[h] = (m0 + row) * p.lda + ((pos ^ (row & 7)) << 4);
    }
#pragma unroll
    for (int h = 0; h < PB; ++h) {
        const int row = (w + NW * h) * 8 + (l >> 3), pos = l & 7;
        vb[h] = (n0 + row) * p.ldb + ((pos ^ (row & 7)) << 4);
    }
    // MX: waves 0 .. BM/64 - 1 fetch A scale rows 64 w + l, the others B scale rows (wave-uniform choice of descriptor)
    const bool is_a = w < T::BM / 64;
    const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(is_a ? p.sa : p.sb, (int)(is_a ? p.sa_bytes : p.sb_bytes));
    const int vs = !MX ? 0 : is_a ? (m0 + 64 * w + l) * p.ldsa : (n0 + 64 * (w - T::BM / 64) + l) * p.ldsb;
    constexpr int S8 = T::S8, DEPTH = S8 - 1;     // K steps in flight
    auto issue = [&](int t) {
        unsigned char* slot = smem + (t % S8) * STAGE;
#pragma unroll
        for (int h = 0; h < PA; ++h)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void8*)(slot + (w + NW * h) * 1024), 16, va[h], t * BK8, 0, 0);
#pragma unroll
        for (int h = 0; h < PB; ++h)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void8*)(slot + T::A_BYTES + (w + NW * h) * 1024), 16, vb[h],
                                                     t * BK8, 0, 0);
        if constexpr (MX)   // rows beyond M / N read as zero (byte 0: 2^-127 times operand rows that are zero as well)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void8*)(slot + T::STAGE_BYTES + w * 256), 4, vs, t * (BK8 / 32), 0, 0);
    };

    f32x4 acc[4][MT];   // [j (n tile)][i (m tile)]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (d < nk) issue(d);
    for (int t = 0; t < nk; ++t) {
        // my pieces of step t have landed: at most the later steps' pieces (PA + PB per step and wave) may still be in flight
        if constexpr (DEPTH == 1) {
            wait_vmcnt<0>();
        } else {
            const int later = min(nk - 1 - t, DEPTH - 1);
            if (later >= 2) wait_vmcnt<2 * (PA + PB + PS)>();
            else if (later == 1) wait_vmcnt<PA + PB + PS>();
            else wait_vmcnt<0>();
        }
        __builtin_amdgcn_s_barrier();     // everybody's have; step t-1 has been read by everybody -> its slot can be refilled
        const unsigned char* ta = smem + (t % S8) * STAGE;
        const unsigned char* tb = ta + T::A_BYTES;
        i32x8 fb[4], fa[4];
        int scb[4], sca[MT];     // MX: this lane's E8M0 bytes (row (l & 15) of each fragment, K block l >> 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) scb[j] = sca[j] = 0x7f7f7f7f;
#pragma unroll
        for (int i = 4; i < MT; ++i) sca[i] = 0x7f7f7f7f;
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = read_frag8<MX>(tb, wn + 16 * j);
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = read_frag8<MX>(ta, wm + 16 * i);
        if constexpr (MX) {
            const unsigned char* tsc = ta + T::STAGE_BYTES + (l >> 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) scb[j] = tsc[4 * (T::BM + wn + 16 * j + (l & 15))];
#pragma unroll
            for (int i = 0; i < MT; ++i) sca[i] = tsc[4 * (wm + 16 * i + (l & 15))];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t + DEPTH < nk) issue(t + DEPTH);     // streams under this and the next steps' MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int half = 0; half < MT / 4; ++half) {     // four m-tiles at a time: A fragments are 8 registers each
            if (half > 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = read_frag8<MX>(ta, wm + 64 * half + 16 * i);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j][4 * half + i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                        fb[j], fa[i], acc[j][4 * half + i], 0, A_E5M2 ? 1 : 0, 0, scb[j], 0, sca[4 * half + i]);
        }
    }
    __builtin_amdgcn_s_barrier();   // all reads of the ring are done: reuse it as epilogue staging
    float* st = reinterpret_cast<float*>(smem) + w * (32 * 68);
    gemm_epilogue_store<MT, 32, MX>(p, acc, st, m0 + wm, n0 + wn);
}

template <class T, bool A_E5M2, bool MX = false>
__global__ __launch_bounds__(T::NT, T::S8 > 2 ? 1 : 2) void gemm_fp8_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Ring8<T, MX>::LDS_BYTES];   // the ONLY LDS object
    gemm_fp8_body<T, A_E5M2, MX>(p, smem);
}

template <class T>
void launch_fp8(GemmParams& p, int a_format, bool mx, hipStream_t s) {
    p.tiles_m = ceil_div(p.M, T::BM); p.tiles_n = ceil_div(p.N, T::BN);
    dim3 grid(p.tiles_m * p.tiles_n), block(T::NT);
    if (mx) hipLaunchKernelGGL((gemm_fp8_kernel<T, false, true>), grid, block, 0, s, p);
    else if (a_format == MH_FP8_E5M2) hipLaunchKernelGGL((gemm_fp8_kernel<T, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((gemm_fp8_kernel<T, false>), grid, block, 0, s, p);
}

// The size rule shared by mh_gemm_fp8 and mh_gemm_mx.
// 128 x 128 tiles (two workgroups per CU: one's epilogue under the other's main loop, and room for other streams' kernels
// beside it) unless the problem is long in K and fills the chip with 256 x 256 tiles for several rounds -- measured
// (scripts/bench_fp8_gemm.py): 128^2 is as fast or faster on every shape of the C5 / C3 steps (e.g. 8192 x 768 x 3072:
// 1403 vs 855 TFLOP/s; 32768 x 3072 x 512: 1090 vs 1061), 256^2 wins at 16384 x 4096 x 4096 (2140 vs 1796).
// MH_GEMM_FP8_TILE_* bits in `flags` force one (experiments, tests; the library reads no environment).
void dispatch_fp8(GemmParams& p, int flags, int a_format, bool mx, hipStream_t stream) {
    const int M = p.M, N = p.N, K = p.K;
    const long tiles256 = (long)ceil_div(M, 256) * ceil_div(N, 256), tiles128 = (long)ceil_div(M, 128) * ceil_div(N, 128);
    const int force = flags & (MH_GEMM_FP8_TILE_256 | MH_GEMM_FP8_TILE_128 | MH_GEMM_FP8_TILE_128D);
    p.flags = flags & ~force;
    const bool big = force ? (force & MH_GEMM_FP8_TILE_256) != 0 : (tiles256 >= 768 && K >= 2048);
    const bool deep = force ? (force & MH_GEMM_FP8_TILE_128D) != 0 : (tiles128 > 128 && tiles128 <= 256 && K >= 2048);   // (256 CUs: at most one tile per CU)
    if (big) launch_fp8<T8_256>(p, a_format, mx, stream);
    else if (deep) launch_fp8<T8_128D>(p, a_format, mx, stream);
    else launch_fp8<T8_128>(p, a_format, mx, stream);
}

}  // namespace

// Checks shared by mh_gemm_fp8 and mh_gemm_mx (operands, epilogue flags, descriptor range); fills everything but the scaling.
static int fp8_gemm_params(const char* fn, int M, int N, int K, const void* A8, int lda, const void* B8, int ldb, void* C, int ldc,
                           int flags, const float* bias, const float* res, int ldr, const void* aux_in, void* aux_out, int ldaux,
                           float* colsum, GemmParams& p) {
    MH_CHECK_ARG(M > 0 && N > 0 && K >= BK8 && K % BK8 == 0, "%s: K must be a positive multiple of 128 (%d %d %d)", fn, M, N, K);
    MH_CHECK_ARG(A8 && B8 && C, "%s: null operand pointer", fn);
    MH_CHECK_ARG(lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K, "%s: lda / ldb must be multiples of 16 and >= K", fn);
    MH_CHECK_ARG(((uintptr_t)A8 | (uintptr_t)B8 | (uintptr_t)C) % 16 == 0, "%s: bases must be 16-B aligned", fn);
    MH_CHECK_ARG(N % 8 == 0 && ldc % 8 == 0, "%s: N, ldc %% 8 == 0", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_ATOMIC), "%s: no atomic accumulate", fn);
    MH_CHECK_ARG((flags & MH_GEMM_OUT_F32) || !(flags & MH_GEMM_RESIDUAL), "%s: residual epilogue needs f32 output", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_OUT_F32) || !(flags & (MH_GEMM_GELU | MH_GEMM_DGELU | MH_GEMM_MULAUX | MH_GEMM_COLSUM)),
                 "%s: GELU / aux / colsum epilogues need bf16 output", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_BIAS) || bias, "%s: bias flag without pointer", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_RESIDUAL) || (res && ldr % 4 == 0), "%s: residual needs pointer, ldr %% 4 == 0", fn);
    MH_CHECK_ARG(!(flags & (MH_GEMM_DGELU | MH_GEMM_MULAUX)) || (aux_in && ldaux % 8 == 0), "%s: aux_in / ldaux", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_AUX_DGELU) || ((flags & MH_GEMM_GELU) && aux_out), "%s: aux_dgelu needs GELU + aux_out", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_GELU) || !aux_out || ldaux % 8 == 0, "%s: ldaux %% 8", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_AUX_U8) || ((flags & (MH_GEMM_AUX_DGELU | MH_GEMM_MULAUX)) && !(flags & MH_GEMM_DGELU)),
                 "%s: MH_GEMM_AUX_U8 applies to the saved GELU derivative only (AUX_DGELU / MULAUX)", fn);
    MH_CHECK_ARG(!(flags & MH_GEMM_COLSUM) || colsum, "%s: colsum flag without pointer", fn);
    MH_CHECK_ARG(gemm_in_reach((long)ceil_div(M, 256) * 256 * lda) && gemm_in_reach((long)ceil_div(N, 256) * 256 * ldb),
                 "%s: operand beyond the 2 GiB buffer-descriptor range", fn);
    gemm_fill(p, M, N, K, A8, lda, B8, ldb, C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux, colsum);
    p.k_per_split = K; p.fast = 1;
    p.a_bytes = (unsigned)gemm_extent(false, M, K, lda, 1); p.b_bytes = (unsigned)gemm_extent(false, N, K, ldb, 1);   // one byte per element
    return 0;
}

extern "C" int mh_gemm_fp8(int M, int N, int K, const void* A8, int lda, int a_format, const void* B8, int ldb, void* C, int ldc,
                           int flags, const float* descale_a, const float* descale_b, const float* bias, const float* res,
                           int ldr, const void* aux_in, void* aux_out, int ldaux, float* colsum, void* c8, int ldc8,
                           const float* c8_scale, float* c8_amax, void* stream) {
    MH_CHECK_ARG(descale_a && descale_b, "mh_gemm_fp8: null operand / descale pointer");
    MH_CHECK_ARG(a_format == MH_FP8_E4M3 || a_format == MH_FP8_E5M2, "mh_gemm_fp8: a_format %d", a_format);
    MH_CHECK_ARG(!c8 || (!(flags & MH_GEMM_OUT_F32) && c8_scale && ldc8 % 8 == 0 && (uintptr_t)c8 % 8 == 0),
                 "mh_gemm_fp8: the fp8 output copy needs a bf16-output epilogue, a scale and ldc8 %% 8 == 0");
    GemmParams p;
    const int rc = fp8_gemm_params("mh_gemm_fp8", M, N, K, A8, lda, B8, ldb, C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux,
                                   colsum, p);
    if (rc) return rc;
    p.descale_a = descale_a; p.descale_b = descale_b;
    p.c8 = (uint8_t*)c8; p.c8_scale = c8_scale; p.c8_amax = c8_amax; p.ldc8 = ldc8;
    dispatch_fp8(p, flags, a_format, false, (hipStream_t)stream);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_gemm_mx(int M, int N, int K, const void* A8, int lda, const void* sa, int ldsa, const void* B8, int ldb,
                          const void* sb, int ldsb, void* C, int ldc, int flags, const float* bias, const float* res, int ldr,
                          const void* aux_in, void* aux_out, int ldaux, float* colsum, void* c8, int ldc8, void* c8_scales,
                          int ldc8s, void* stream) {
    MH_CHECK_ARG(M > 0 && N > 0 && K >= BK8 && K % BK8 == 0, "mh_gemm_mx: K must be a positive multiple of 128 (%d %d %d)", M, N, K);
    MH_CHECK_ARG(sa && sb, "mh_gemm_mx: null scale pointer (sa / sb)");
    MH_CHECK_ARG(ldsa % 4 == 0 && ldsb % 4 == 0 && ldsa >= K / 32 && ldsb >= K / 32 && ((uintptr_t)sa | (uintptr_t)sb) % 4 == 0,
                 "mh_gemm_mx: ldsa / ldsb must be multiples of 4 and >= K / 32 (%d %d), scale bases 4-B aligned", ldsa, ldsb);
    MH_CHECK_ARG((long)ceil_div(M, 256) * 256 * ldsa + 1024 < (1L << 31) && (long)ceil_div(N, 256) * 256 * ldsb + 1024 < (1L << 31),
                 "mh_gemm_mx: scales beyond the 2 GiB buffer-descriptor range");
    MH_CHECK_ARG(!c8 || (!(flags & MH_GEMM_OUT_F32) && (uintptr_t)c8 % 8 == 0 && ldc8 % 8 == 0 && N % 32 == 0),
                 "mh_gemm_mx: the MX output copy needs a bf16-output epilogue, ldc8 %% 8 == 0 and N %% 32 == 0");
    MH_CHECK_ARG(!c8 || (c8_scales && ldc8s % 4 == 0 && ldc8s >= N / 32), "mh_gemm_mx: the MX output copy needs c8_scales and "
                 "ldc8s %% 4 == 0, ldc8s >= N / 32 (%d)", ldc8s);
    MH_CHECK_ARG(!(flags & MH_GEMM_C8_E5M2), "mh_gemm_mx: the MX output copy is e4m3");
    GemmParams p;
    const int rc = fp8_gemm_params("mh_gemm_mx", M, N, K, A8, lda, B8, ldb, C, ldc, flags, bias, res, ldr, aux_in, aux_out, ldaux,
                                   colsum, p);
    if (rc) return rc;
    p.sa = (const uint8_t*)sa; p.sb = (const uint8_t*)sb; p.ldsa = ldsa; p.ldsb = ldsb;
    p.sa_bytes = (unsigned)((long)(M - 1) * ldsa + K / 32); p.sb_bytes = (unsigned)((long)(N - 1) * ldsb + K / 32);
    p.c8 = (uint8_t*)c8; p.ldc8 = ldc8; p.c8_scales = (uint8_t*)c8_scales; p.ldc8s = ldc8s;
    dispatch_fp8(p, flags, MH_FP8_E4M3, true, (hipStream_t)stream);
    MH_LAUNCH_CHECK();
    return 0;
}
