// Device-side mask draws (mh_mask_draw, include/maestro_hip.h): the structural Bernoulli masks with their rejection loop
// and the per-token noise of maestro/ssl/mae.py:178-246 on Philox4x32-10.  One workgroup per (group, row): first the
// structural row (counted attempt loop, all-masked test = workgroup-wide AND through LDS), then the noise row (four values per
// Philox call, one 16-byte store where the row is 16-byte aligned).  Integer ALU + a few hundred KB of stores; no atomics.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;

__device__ __forceinline__ float to_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

struct Draw {
    uint32_t k0, k1, step;
    __device__ __forceinline__ float u(uint32_t kind, uint32_t stream, uint32_t row, uint32_t attempt, uint32_t i) const {
        const u32x4 w = philox4x32_10(i >> 2, row, step, kind | stream << 4 | attempt << 16, k0, k1);
        return to_uniform(w[i & 3]);
    }
};

__global__ __launch_bounds__(THREADS) void mask_draw_kernel(const MhMaskJob* __restrict__ jobs, const MhMaskSeg* __restrict__ segs,
                                                            uint32_t k0, uint32_t k1, uint32_t step, uint32_t row_base) {
    __shared__ int red[2][WAVES];
    const MhMaskJob job = jobs[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= job.Beff) return;                         // (uniform: the grid is as wide as the largest group)
    const int tid = threadIdx.x, L = job.L;
    const Draw draw{k0, k1, step};

    // ---- structural row
    unsigned char* srow = job.strct + (size_t)r * L;
    const uint32_t s_row = row_base * (uint32_t)job.struct_rpb + (uint32_t)r;
    bool kept = false;
    for (int a = 0; a < MH_MASK_MAX_ATTEMPTS && !kept; ++a) {
        int all = 1;
        int si = -1, seg_end = 0;                      // the segment of the thread's current token (tokens ascend: so do segments)
        MhMaskSeg sg = {};
        bool whole = false;                            // mod | bands: one draw for the whole segment
        for (int t = tid; t < L; t += THREADS) {
            while (t >= seg_end && si + 1 < job.n_segs) {
                sg = segs[job.seg0 + ++si];
                seg_end = sg.tok_off + sg.D * sg.L;
                whole = (sg.p_mod > 0.f && draw.u(MH_MASK_KIND_MOD, sg.stream, s_row, a, 0) < sg.p_mod) ||
                        (sg.p_bands > 0.f && draw.u(MH_MASK_KIND_BANDS, sg.stream, s_row, a, sg.gi) < sg.p_bands);
            }
            bool m = whole;
            if (!m) {
                const int o = t - sg.tok_off, d = o / sg.L, l = o - d * sg.L;
                m = (sg.p_dates > 0.f && draw.u(MH_MASK_KIND_DATES, sg.stream, s_row, a, d) < sg.p_dates) ||
                    (sg.p_loc > 0.f && draw.u(MH_MASK_KIND_LOC, sg.stream, s_row, a, l) < sg.p_loc);
            }
            srow[t] = m ? 1 : 0;
            all &= m ? 1 : 0;
        }
        all = __all(all);
        if ((tid & 63) == 0) red[a & 1][tid >> 6] = all;
        __syncthreads();                               // (two slots: attempt a + 2 writes its slot behind the barrier of a + 1)
        int every = 1;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) every &= red[a & 1][w];
        kept = !every;
    }
    if (!kept)                                         // the bound is exhausted: all-clear
        for (int t = tid; t < L; t += THREADS) srow[t] = 0;

    // ---- noise row
    const uint32_t n_row = row_base * (uint32_t)job.noise_rpb + (uint32_t)((r / job.row_div) * job.row_mul + job.row_add + r % job.row_div);
    float* nrow = job.noise + (size_t)r * L;
    const uint32_t c3 = MH_MASK_KIND_NOISE | (uint32_t)job.noise_stream << 4;
    const bool vec = (L & 3) == 0 && ((uintptr_t)job.noise & 15) == 0;      // every row starts on a 16-byte boundary
    for (int q = tid; 4 * q < L; q += THREADS) {
        const u32x4 w = philox4x32_10(q, n_row, step, c3, k0, k1);
        const f32x4 v = {to_uniform(w[0]), to_uniform(w[1]), to_uniform(w[2]), to_uniform(w[3])};
        if (vec) {
            *reinterpret_cast<f32x4*>(nrow + 4 * q) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < L) nrow[4 * q + j] = v[j];
        }
    }
}

}  // namespace

extern "C" int mh_mask_draw(const MhMaskJob* jobs_host, const MhMaskJob* jobs_device, int n_jobs, const MhMaskSeg* segs_host,
                            const MhMaskSeg* segs_device, int n_segs, uint64_t seed, long long step, long long row_base, void* stream) {
    MH_CHECK_ARG(n_jobs > 0 && n_jobs <= 65535, "mh_mask_draw: n_jobs %d must be 1 ... 65535", n_jobs);
    MH_CHECK_ARG(n_segs > 0, "mh_mask_draw: n_segs %d must be positive", n_segs);
    MH_CHECK_ARG(jobs_host && jobs_device && segs_host && segs_device, "mh_mask_draw: null pointer (job / segment tables)");
    MH_CHECK_ARG(step >= 0 && step <= 0xFFFFFFFFll, "mh_mask_draw: step %lld is not an unsigned 32-bit value", step);
    MH_CHECK_ARG(row_base >= 0 && row_base <= 0xFFFFFFFFll, "mh_mask_draw: row_base %lld out of range", row_base);
    int max_rows = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const MhMaskJob& j = jobs_host[i];
        MH_CHECK_ARG(j.noise && j.strct, "mh_mask_draw: job %d: null pointer", i);
        MH_CHECK_ARG(j.L >= 1 && j.L <= MH_MASK_MAX_L, "mh_mask_draw: job %d: L %d (1 ... %d)", i, j.L, MH_MASK_MAX_L);
        MH_CHECK_ARG(j.Beff >= 1, "mh_mask_draw: job %d: Beff %d", i, j.Beff);
        MH_CHECK_ARG(j.noise_stream >= 0 && j.noise_stream < MH_MASK_MAX_STREAMS, "mh_mask_draw: job %d: noise stream %d", i, j.noise_stream);
        MH_CHECK_ARG(j.row_div >= 1 && j.row_mul >= j.row_div && j.row_add >= 0 && j.row_add + j.row_div <= j.row_mul,
                     "mh_mask_draw: job %d: draw-row map (%d, %d, %d)", i, j.row_div, j.row_mul, j.row_add);
        MH_CHECK_ARG(j.noise_rpb >= 1 && j.struct_rpb >= 1, "mh_mask_draw: job %d: rows per sample (%d, %d)", i, j.noise_rpb, j.struct_rpb);
        // the largest row index of either draw stays an unsigned 32-bit value
        const long long last_noise = row_base * j.noise_rpb + (long long)((j.Beff - 1) / j.row_div) * j.row_mul + j.row_add + j.row_div - 1;
        const long long last_struct = row_base * j.struct_rpb + j.Beff - 1;
        MH_CHECK_ARG(last_noise <= 0xFFFFFFFFll && last_struct <= 0xFFFFFFFFll, "mh_mask_draw: job %d: global row index leaves 32 bits", i);
        MH_CHECK_ARG(j.seg0 >= 0 && j.n_segs >= 1 && j.seg0 <= n_segs - j.n_segs, "mh_mask_draw: job %d: segments %d + %d of %d", i,
                     j.seg0, j.n_segs, n_segs);
        int tok = 0;
        for (int k = j.seg0; k < j.seg0 + j.n_segs; ++k) {
            const MhMaskSeg& s = segs_host[k];
            MH_CHECK_ARG(s.D >= 1 && s.L >= 1 && s.L <= MH_MASK_MAX_L && s.D <= MH_MASK_MAX_L, "mh_mask_draw: segment %d: D %d, L %d", k, s.D, s.L);
            MH_CHECK_ARG(s.tok_off == tok, "mh_mask_draw: segment %d: tok_off %d, expected %d (segments tile the row in order)", k,
                         s.tok_off, tok);
            MH_CHECK_ARG(s.G >= 1 && s.gi >= 0 && s.gi < s.G, "mh_mask_draw: segment %d: band-group %d of %d", k, s.gi, s.G);
            MH_CHECK_ARG(s.stream >= 0 && s.stream < MH_MASK_MAX_STREAMS, "mh_mask_draw: segment %d: stream %d", k, s.stream);
            MH_CHECK_ARG(s.p_mod == s.p_mod && s.p_bands == s.p_bands && s.p_dates == s.p_dates && s.p_loc == s.p_loc,
                         "mh_mask_draw: segment %d: NaN probability", k);
            tok += s.D * s.L;
            MH_CHECK_ARG(tok <= j.L, "mh_mask_draw: job %d: segments cover %d tokens of %d", i, tok, j.L);
        }
        MH_CHECK_ARG(tok == j.L, "mh_mask_draw: job %d: segments cover %d tokens of %d", i, tok, j.L);
        max_rows = j.Beff > max_rows ? j.Beff : max_rows;
    }
    hipLaunchKernelGGL(mask_draw_kernel, dim3(max_rows, n_jobs), dim3(THREADS), 0, (hipStream_t)stream, jobs_device, segs_device,
                       (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)row_base);
    MH_LAUNCH_CHECK();
    return 0;
}
