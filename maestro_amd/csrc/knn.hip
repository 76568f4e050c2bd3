// Nearest neighbours of exported encoder features: row normalisation, the top-k cosine neighbours of bf16 queries in a bf16
// bank, and the weighted vote over their labels.  C declarations and the full contract: include/maestro_hip.h.
//
// mh_knn_topk is the project's bf16 NT tile loop (gemm_reg.hpp: buffer loads -> registers -> swizzled LDS -> ds_read_b128
// fragments -> v_mfma_f32_16x16x32_bf16) with a selection for an epilogue, so the [Nq, Nb] similarities never leave the
// accumulators.  A workgroup owns 64 queries and walks the 128-row bank tiles of its split.  Per query it keeps the sorted list of
// its k best pairs in LDS, with the k-th pair as a threshold; every accumulator element is compared with its row's threshold, and
// the few that pass are appended to the row's candidate strip (an LDS slot counter: the result is defined by a total order, not
// by arrival order).  Then each wave takes 16 rows and inserts the candidates of a row with the list in registers -- lane t holds
// entries t and t + 64; the position is a ballot count, the shift one shuffle.  Nothing here is a global atomic; the partial
// lists of the splits are merged by a second kernel under the same order.
#include "gemm_reg.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr int KQ = 64, KB = 128;                              // query rows and bank rows of a workgroup's tile
constexpr int KA_BYTES = KQ * 128, KB_BYTES = KB * 128;       // one 64-column K step of each operand in LDS
constexpr int K_OPER = 2 * KA_BYTES + 2 * KB_BYTES;           // A0 A1 B0 B1: 48 KiB
constexpr int KNN_SLOTS = 512;                                // workgroup slots mh_knn_splits fills: 256 CUs x 2
constexpr int KNN_MAX_SPLITS = 65535;
constexpr int MERGE_MAX_WAVES = 16;
constexpr float NEG_INF = -__builtin_inff();

// Rounded one by one (the build's default contracts a * b + c).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// The order rule of include/maestro_hip.h: (s, i) comes before (ts, ti).  Indices compare as unsigned, so the -1 of an unfilled slot comes
// after every real index; a NaN s comes before nothing.
__device__ __forceinline__ bool before(float s, int i, float ts, int ti) {
    return s > ts || (s == ts && (unsigned)i < (unsigned)ti);
}

// The value lane `src` holds, `src` the same in every lane (v_readlane_b32)
__device__ __forceinline__ int lane_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float lane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// A sorted list of k <= 128 pairs across the 64 lanes of a wave: lane t holds entries t (s0, i0) and t + 64 (s1, i1).
struct TopList { float s0, s1; int i0, i1; };

// Insert (s, i), the same in every lane, if it comes before the k-th entry.  Called by whole waves only.
__device__ __forceinline__ void toplist_insert(TopList& t, float s, int i, int k, int lane) {
    const bool two = k > 64;
    int pos = __popcll(__ballot(lane < k && before(t.s0, t.i0, s, i)));             // entries that come before it: a prefix
    if (two) pos += __popcll(__ballot(lane + 64 < k && before(t.s1, t.i1, s, i)));
    if (pos >= k) return;
    const float p0s = __shfl_up(t.s0, 1, 64);
    const int p0i = __shfl_up(t.i0, 1, 64);
    if (two) {
        const float cs = lane_f(t.s0, 63), p1s = __shfl_up(t.s1, 1, 64);            // entry 63 moves to lane 0 of the second half
        const int ci = lane_i(t.i0, 63), p1i = __shfl_up(t.i1, 1, 64);
        const int slot = lane + 64;
        if (slot > pos) { t.s1 = lane == 0 ? cs : p1s; t.i1 = lane == 0 ? ci : p1i; }
        else if (slot == pos) { t.s1 = s; t.i1 = i; }
    }
    if (lane > pos) { t.s0 = p0s; t.i0 = p0i; }
    else if (lane == pos) { t.s0 = s; t.i0 = i; }
}
__device__ __forceinline__ void toplist_kth(const TopList& t, int k, float& s, int& i) {
    const int src = (k - 1) & 63;                             // uniform: v_readlane, not a trip through the LDS crossbar
    s = lane_f(k > 64 ? t.s1 : t.s0, src);
    i = lane_i(k > 64 ? t.i1 : t.i0, src);
}

// Fold the 64 lanes' candidates (cs, ci; ci < 0: none) into the list: those that come before the running k-th pair (ks, ki), one
// by one in lane order; the rest cost one ballot together.  Called by whole waves only.
__device__ __forceinline__ void toplist_fold(TopList& t, float& ks, int& ki, float cs, int ci, int k, int lane) {
    unsigned long long m = __ballot(ci >= 0 && before(cs, ci, ks, ki));
    while (m) {
        const int u = __ffsll((long long)m) - 1;
        toplist_insert(t, lane_f(cs, u), lane_i(ci, u), k, lane);
        toplist_kth(t, k, ks, ki);
        m &= __ballot(ci >= 0 && before(cs, ci, ks, ki)) & ~((2ull << u) - 1ull);       // what still passes, behind lane u
    }
}

// blockIdx.x = the 64-query tile, blockIdx.y = the split.  KP = list pitch (k <= KP).
// LDS: operand images (the candidate strips lie over them between two tiles: f32 [KQ][KB] similarities, u8 [KQ][KB] tile columns)
// | int cnt[KQ] | the thresholds f32 [KQ], i32 [KQ] | the lists f32 [KQ][KP], i32 [KQ][KP].
template <int KP>
__global__ __launch_bounds__(NT) void knn_topk_kernel(const bf16_t* __restrict__ q, int ldq, const bf16_t* __restrict__ bank, int ldb,
                                                      int index_base, float* __restrict__ ws_s, int* __restrict__ ws_i, int Nq, int Nb,
                                                      int E, int k, int splits) {
    static_assert(KQ * KB * 5 <= K_OPER, "the candidate strips lie over the operand images");
    __shared__ __attribute__((aligned(16))) unsigned char smem[K_OPER + 3 * KQ * 4 + KQ * KP * 8];
    unsigned char* const sb = smem + 2 * KA_BYTES;
    float* const cand_s = reinterpret_cast<float*>(smem);
    unsigned char* const cand_c = smem + KQ * KB * 4;
    int* const cnt = reinterpret_cast<int*>(smem + K_OPER);
    float* const thr_s = reinterpret_cast<float*>(cnt + KQ);
    int* const thr_i = reinterpret_cast<int*>(thr_s + KQ);
    float* const ls = reinterpret_cast<float*>(thr_i + KQ);
    int* const li = reinterpret_cast<int*>(ls + KQ * KP);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, lm = l & 15;
    const int m0 = blockIdx.x * KQ, split = blockIdx.y;
    const int b_tiles = (Nb + KB - 1) / KB;
    const int t_beg = (int)((long)split * b_tiles / splits), t_end = (int)((long)(split + 1) * b_tiles / splits);
    const int wm = (w >> 1) * 32, wn = (w & 1) * 64;
    const int nk = (E + BK - 1) / BK, nsub = E / 32;          // K steps of 64 columns; MFMA blocks of 32 (the last step may hold one)

    for (int e = tid; e < KQ * KP; e += NT) { ls[e] = NEG_INF; li[e] = -1; }
    if (tid < KQ) { cnt[tid] = 0; thr_s[tid] = NEG_INF; thr_i[tid] = -1; }
    __syncthreads();

    // One descriptor per tile: rows past the operand's end read as zero (and are never candidates)
    const __amdgpu_buffer_rsrc_t ra_src = buffer_rsrc(q + (size_t)m0 * ldq, (int)matrix_bytes(min(KQ, Nq - m0), E, ldq, 2));
    int va[2], vb[4];
    tile_offsets<false, 2>(ldq, 0, va);
    tile_offsets<false, 4>(ldb, 0, vb);

    for (int bt = t_beg; bt < t_end; ++bt) {
        const int n0 = bt * KB, b_rows = min(KB, Nb - n0);
        const __amdgpu_buffer_rsrc_t rb_src = buffer_rsrc(bank + (size_t)n0 * ldb, (int)matrix_bytes(b_rows, E, ldb, 2));
        f32x4 acc[4][2];                                      // [j (bank 16-row block)][i (query 16-row block)]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto half = [&](const unsigned char* ta, const unsigned char* tb, int s) {
            bf16x8 fa[2], fb[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = read_frag<false>(ta, wm + 16 * i, s);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = read_frag<false>(tb, wn + 16 * j, s);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[j][i], 0, 0, 0);
        };
        u32x4 ra[2], rb[4];
        load_tile_fast(ra_src, va, 0, ra);
        load_tile_fast(rb_src, vb, 0, rb);
        store_tile<false, 2>(smem, ra);
        store_tile<false>(sb, rb);
        if (nk > 1) {
            load_tile_fast(ra_src, va, BK * 2, ra);
            load_tile_fast(rb_src, vb, BK * 2, rb);
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {                     // one barrier per K step, as gemm.hip's closing steps
            const int cur = kt & 1;
            const unsigned char* ta = smem + cur * KA_BYTES;
            const unsigned char* tb = sb + cur * KB_BYTES;
            half(ta, tb, 0);
            if (kt + 1 < nk) {
                store_tile<false, 2>(smem + (cur ^ 1) * KA_BYTES, ra);
                store_tile<false>(sb + (cur ^ 1) * KB_BYTES, rb);
                if (kt + 2 < nk) {
                    load_tile_fast(ra_src, va, (kt + 2) * BK * 2, ra);
                    load_tile_fast(rb_src, vb, (kt + 2) * BK * 2, rb);
                }
            }
            if (2 * kt + 1 < nsub) half(ta, tb, 1);           // (E % 64 == 32: the columns past E are never multiplied)
            __syncthreads();
        }

        // selection, 1: every accumulator element against its row's k-th pair (the operand images are free now)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wm + 16 * i + lm;
            const float ts = thr_s[row];
            const int ti = thr_i[row];
            const bool row_ok = m0 + row < Nq;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = wn + 16 * j + 4 * g + r;
                    const float s = acc[j][i][r];
                    if (row_ok && col < b_rows && before(s, index_base + n0 + col, ts, ti)) {
                        const int slot = atomicAdd(&cnt[row], 1);             // at most KB per row and tile: the strip's length
                        cand_s[row * KB + slot] = s;
                        cand_c[row * KB + slot] = (unsigned char)col;
                    }
                }
        }
        __syncthreads();
        // selection, 2: wave w inserts the candidates of rows w, w + 4, ... (interleaved: a short last query tile loads all four)
        for (int rr = 0; rr < 16; ++rr) {
            const int row = 4 * rr + w;
            const int n = __builtin_amdgcn_readfirstlane(cnt[row]);
            if (n == 0) continue;
            TopList t;
            t.s0 = l < k ? ls[row * KP + l] : NEG_INF;
            t.i0 = l < k ? li[row * KP + l] : -1;
            t.s1 = l + 64 < k ? ls[row * KP + l + 64] : NEG_INF;
            t.i1 = l + 64 < k ? li[row * KP + l + 64] : -1;
            float ks = thr_s[row];                                 // the list's k-th pair
            int ki = thr_i[row];
            for (int c0 = 0; c0 < n; c0 += 64) {
                float cs = NEG_INF;
                int ci = -1;
                if (c0 + l < n) {
                    cs = cand_s[row * KB + c0 + l];
                    ci = index_base + n0 + cand_c[row * KB + c0 + l];
                }
                toplist_fold(t, ks, ki, cs, ci, k, l);
            }
            if (l < k) { ls[row * KP + l] = t.s0; li[row * KP + l] = t.i0; }
            if (l + 64 < k) { ls[row * KP + l + 64] = t.s1; li[row * KP + l + 64] = t.i1; }
            if (l == 0) { thr_s[row] = ks; thr_i[row] = ki; cnt[row] = 0; }
        }
        __syncthreads();
    }

    for (int e = tid; e < KQ * k; e += NT) {
        const int row = e / k, t = e - row * k;
        if (m0 + row < Nq) {
            const size_t o = ((size_t)split * Nq + m0 + row) * k + t;
            ws_s[o] = ls[row * KP + t];
            ws_i[o] = li[row * KP + t];
        }
    }
}

// One query per workgroup of blockDim.x / 64 waves.  The candidates are the splits' lists [splits][Nq][k] and, with
// `accumulate`, the incoming row of sims / idx; every wave folds a contiguous share of them, wave 0 folds the waves' lists.
__global__ __launch_bounds__(64 * MERGE_MAX_WAVES) void knn_merge_kernel(const float* __restrict__ ws_s, const int* __restrict__ ws_i,
                                                                         float* sims, int* idx, int accumulate, int Nq, int k,
                                                                         int splits) {
    __shared__ float ms[MERGE_MAX_WAVES * MH_KNN_MAX_K];
    __shared__ int mi[MERGE_MAX_WAVES * MH_KNN_MAX_K];
    const int qi = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int total = (splits + (accumulate ? 1 : 0)) * k;
    const int per = ((total + nw - 1) / nw + 63) & ~63;
    const int beg = min(total, w * per), end = min(total, beg + per);
    TopList t = {NEG_INF, NEG_INF, -1, -1};
    float ks = NEG_INF;
    int ki = -1;
    auto fold = [&](float cs, int ci) { toplist_fold(t, ks, ki, cs, ci, k, l); };
    for (int c0 = beg; c0 < end; c0 += 64) {
        const int c = c0 + l;
        float cs = NEG_INF;
        int ci = -1;
        if (c < end) {
            const int sp = c / k, e = c - sp * k;
            if (sp < splits) {
                const size_t o = ((size_t)sp * Nq + qi) * k + e;
                cs = ws_s[o];
                ci = ws_i[o];
            } else {
                cs = sims[(size_t)qi * k + e];
                ci = idx[(size_t)qi * k + e];
            }
        }
        fold(cs, ci);
    }
    if (l < k) { ms[w * MH_KNN_MAX_K + l] = t.s0; mi[w * MH_KNN_MAX_K + l] = t.i0; }
    if (l + 64 < k) { ms[w * MH_KNN_MAX_K + l + 64] = t.s1; mi[w * MH_KNN_MAX_K + l + 64] = t.i1; }
    __syncthreads();
    if (w != 0) return;
    for (int ww = 1; ww < nw; ++ww)
        for (int c0 = 0; c0 < k; c0 += 64) {
            const int c = c0 + l;
            fold(c < k ? ms[ww * MH_KNN_MAX_K + c] : NEG_INF, c < k ? mi[ww * MH_KNN_MAX_K + c] : -1);
        }
    if (l < k) { sims[(size_t)qi * k + l] = t.s0; idx[(size_t)qi * k + l] = t.i0; }
    if (l + 64 < k) { sims[(size_t)qi * k + l + 64] = t.s1; idx[(size_t)qi * k + l + 64] = t.i1; }
}

// One query per wave, four per workgroup.  LDS per wave: the weights and the voting labels (-1: no vote) of its k_eval entries.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ sims, const int* __restrict__ idx,
                                                       const int* __restrict__ labels, long n_labels, int missing_val, float inv_T, int k,
                                                       int k_eval, float* __restrict__ scores, long lds, int* __restrict__ cls, int Nq,
                                                       int C) {
    __shared__ float vw[4][MH_KNN_MAX_K];
    __shared__ int vl[4][MH_KNN_MAX_K];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long qi = (long)blockIdx.x * 4 + w;
    const bool on = qi < Nq;
    int voters = 0;
    if (on) {
        const float s0 = sims[qi * k];
        for (int j = l; j < k_eval; j += 64) {
            const float s = sims[qi * k + j];
            const int id = idx[qi * k + j];
            int lab = -1;
            if (id >= 0 && id < n_labels) {
                const int v = labels[id];
                if (v != missing_val && v >= 0 && v < C) lab = v;
            }
            vw[w][j] = s == s0 ? 1.f : expf(mul_rn(sub_rn(s, s0), inv_T));
            vl[w][j] = lab;
            voters += lab >= 0;
        }
    }
    __syncthreads();
    if (!on) return;
    float best = -1.f;
    int arg = -1;
    for (int c = l; c < C; c += 64) {
        float a = 0.f;
        for (int j = 0; j < k_eval; ++j)
            if (vl[w][j] == c) a = add_rn(a, vw[w][j]);
        if (scores) scores[qi * lds + c] = a;
        if (a > best) { best = a; arg = c; }
    }
    if (!cls) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        voters += __shfl_xor(voters, o, 64);
        if (ob > best || (ob == best && (unsigned)oa < (unsigned)arg)) { best = ob; arg = oa; }
    }
    if (l == 0) cls[qi] = voters > 0 ? arg : -1;
}

// One row per wave, four per workgroup; the order of the sum of squares is the one include/maestro_hip.h states.
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* x, long ldx, float eps, float* y, long ldy, bf16_t* __restrict__ y16,
                                                           long ldy16, long rows, int E) {
    const int l = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * ldx;
    float s = 0.f;
    for (int c = l; c < E; c += 64) {
        const float v = xr[c];
        s = __builtin_fmaf(v, v, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = add_rn(s, __shfl_xor(s, o, 64));
    const float d = fmaxf(__fsqrt_rn(s), eps);
    for (int c = l; c < E; c += 64) {
        const float r = d > 0.f ? __fdiv_rn(xr[c], d) : 0.f;          // (y may be x: this lane alone reads and writes element c)
        if (y) y[row * ldy + c] = r;
        if (y16) y16[row * ldy16 + c] = f2bf(r);
    }
}

bool knn_shape_ok(int Nq, int k) { return Nq > 0 && k >= 1 && k <= MH_KNN_MAX_K; }

}  // namespace

extern "C" int mh_knn_splits(int Nq, int Nb, int E, int k) {
    if (!knn_shape_ok(Nq, k) || Nb < 0 || E < 32 || E > 1024 || E % 32) return 0;
    const int q_tiles = ceil_div(Nq, KQ), b_tiles = ceil_div(Nb, KB);
    // enough splits to fill the workgroup slots, each with at least two bank tiles to walk
    return max(1, min(min(KNN_SLOTS / q_tiles, b_tiles / 2), KNN_MAX_SPLITS));
}

extern "C" long mh_knn_workspace_bytes(int Nq, int k, int splits) {
    if (!knn_shape_ok(Nq, k) || splits < 1 || splits > KNN_MAX_SPLITS) return -1;
    return (long)splits * Nq * k * 8;
}

extern "C" int mh_l2_normalize(const float* x, long ldx, float eps, float* y, long ldy, uint16_t* y16, long ldy16, long rows, int E,
                               void* stream) {
    MH_CHECK_ARG(x, "mh_l2_normalize: null x");
    MH_CHECK_ARG(y || y16, "mh_l2_normalize: no output (y and y16 are both null)");
    MH_CHECK_ARG(rows > 0 && rows <= 0x7fffffffL && E >= 1 && E <= 65536, "mh_l2_normalize: rows = %ld, E = %d", rows, E);
    MH_CHECK_ARG(ldx >= E && (!y || ldy >= E) && (!y16 || ldy16 >= E), "mh_l2_normalize: a pitch below E = %d (ldx %ld, ldy %ld, ldy16 %ld)",
                 E, ldx, ldy, ldy16);
    MH_CHECK_ARG(eps >= 0.f, "mh_l2_normalize: eps = %g (must be >= 0)", (double)eps);
    MH_CHECK_ARG((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)y16 % 2 == 0, "mh_l2_normalize: misaligned base");
    MH_CHECK_ARG((const float*)y != x || ldy == ldx, "mh_l2_normalize: y is x but ldy = %ld != ldx = %ld", ldy, ldx);
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, eps, y, ldy, y16,
                       ldy16, rows, E);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_knn_topk(const uint16_t* q, long ldq, const uint16_t* bank, long ldb, long index_base, float* sims, int* idx,
                           int accumulate, void* ws, long ws_bytes, int splits, int Nq, int Nb, int E, int k, void* stream) {
    MH_CHECK_ARG(q && (bank || Nb == 0) && sims && idx && ws, "mh_knn_topk: null q, bank, sims, idx or ws");
    MH_CHECK_ARG(Nq > 0, "mh_knn_topk: Nq = %d", Nq);
    MH_CHECK_ARG(k >= 1 && k <= MH_KNN_MAX_K, "mh_knn_topk: k = %d (1 ... %d)", k, MH_KNN_MAX_K);
    MH_CHECK_ARG(E >= 32 && E <= 1024 && E % 32 == 0, "mh_knn_topk: E = %d (a multiple of 32 in 32 ... 1024)", E);
    MH_CHECK_ARG(accumulate == 0 || accumulate == 1, "mh_knn_topk: accumulate = %d", accumulate);
    MH_CHECK_ARG(Nb > 0 || (Nb == 0 && accumulate), "mh_knn_topk: Nb = %d (an empty bank only with accumulate)", Nb);
    MH_CHECK_ARG(ldq >= E && ldb >= E && ldq % 8 == 0 && ldb % 8 == 0 && ldq <= (1L << 20) && ldb <= (1L << 20),
                 "mh_knn_topk: ldq = %ld, ldb = %ld (multiples of 8 in E = %d ... 2^20)", ldq, ldb, E);
    MH_CHECK_ARG(((uintptr_t)q | (uintptr_t)bank | (uintptr_t)ws) % 16 == 0, "mh_knn_topk: q, bank and ws must be 16-byte aligned");
    MH_CHECK_ARG(((uintptr_t)sims | (uintptr_t)idx) % 4 == 0, "mh_knn_topk: sims and idx must be 4-byte aligned");
    MH_CHECK_ARG(index_base >= 0 && index_base + Nb <= 0x7fffffffL, "mh_knn_topk: index_base = %ld + Nb = %d leaves int32", index_base, Nb);
    MH_CHECK_ARG(splits >= 1 && splits <= KNN_MAX_SPLITS, "mh_knn_topk: splits = %d (1 ... %d)", splits, KNN_MAX_SPLITS);
    MH_CHECK_ARG((long)Nq * k <= 0x7fffffffL / 8, "mh_knn_topk: Nq * k = %ld too large", (long)Nq * k);
    const long need = mh_knn_workspace_bytes(Nq, k, splits);
    MH_CHECK_ARG(ws_bytes >= need, "mh_knn_topk: workspace of %ld bytes, %ld needed for %d splits", ws_bytes, need, splits);
    float* ws_s = (float*)ws;
    int* ws_i = (int*)ws + (size_t)splits * Nq * k;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(Nq, KQ), (unsigned)splits);
    if (k <= 32)
        hipLaunchKernelGGL(knn_topk_kernel<32>, grid, dim3(NT), 0, s, (const bf16_t*)q, (int)ldq, (const bf16_t*)bank, (int)ldb,
                           (int)index_base, ws_s, ws_i, Nq, Nb, E, k, splits);
    else
        hipLaunchKernelGGL(knn_topk_kernel<MH_KNN_MAX_K>, grid, dim3(NT), 0, s, (const bf16_t*)q, (int)ldq, (const bf16_t*)bank, (int)ldb,
                           (int)index_base, ws_s, ws_i, Nq, Nb, E, k, splits);
    MH_LAUNCH_CHECK();
    const int total = (splits + accumulate) * k;
    const int waves = max(1, min(ceil_div(total, 256), MERGE_MAX_WAVES));
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Nq), dim3(64 * waves), 0, s, ws_s, ws_i, sims, idx, accumulate, Nq, k, splits);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_knn_vote(const float* sims, const int* idx, const int* labels, long n_labels, int missing_val, float inv_T, int k,
                           int k_eval, float* scores, long lds, int* cls, int Nq, int C, void* stream) {
    MH_CHECK_ARG(sims && idx && labels, "mh_knn_vote: null sims, idx or labels");
    MH_CHECK_ARG(scores || cls, "mh_knn_vote: no output (scores and cls are both null)");
    MH_CHECK_ARG(Nq > 0 && n_labels > 0, "mh_knn_vote: Nq = %d, n_labels = %ld", Nq, n_labels);
    MH_CHECK_ARG(k >= 1 && k <= MH_KNN_MAX_K && k_eval >= 1 && k_eval <= k, "mh_knn_vote: k = %d, k_eval = %d (1 <= k_eval <= k <= %d)", k,
                 k_eval, MH_KNN_MAX_K);
    MH_CHECK_ARG(C >= 2 && C <= 1024, "mh_knn_vote: %d classes (2 ... 1024 are supported)", C);
    MH_CHECK_ARG(inv_T > 0.f && inv_T <= 3.0e38f, "mh_knn_vote: inv_T = %g (must be positive and finite)", (double)inv_T);
    MH_CHECK_ARG(!scores || lds >= C, "mh_knn_vote: lds = %ld below C = %d", lds, C);
    MH_CHECK_ARG(((uintptr_t)sims | (uintptr_t)idx | (uintptr_t)labels | (uintptr_t)scores | (uintptr_t)cls) % 4 == 0,
                 "mh_knn_vote: misaligned base");
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)ceil_div(Nq, 4)), dim3(256), 0, (hipStream_t)stream, sims, idx, labels, n_labels,
                       missing_val, inv_T, k, k_eval, scores, lds, cls, Nq, C);
    MH_LAUNCH_CHECK();
    return 0;
}
