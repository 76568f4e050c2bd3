// Prediction metrics of the probe / finetune branch (maestro/train/metric.py, fed from maestro/train/base.py:143-146): confusion
// matrices counted on the device from the logits the loss kernels already read.  C ABI: include/maestro_hip.h.
//
// Everything here is integer: LDS histograms of 32-bit counters per workgroup, flushed with 64-bit integer atomics (plain vector
// memory).  The result does not depend on the launch order and there is no float atomic.
#include "common.hpp"
#include "logits_walk.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr long CF_WG_PIXELS = 1L << 31;   // pixels one workgroup counts at most: its 32-bit LDS counters cannot wrap

__device__ __forceinline__ long load_int(const void* p, long i, int bytes) {
    switch (bytes) {
        case 1: return reinterpret_cast<const int8_t*>(p)[i];
        case 2: return reinterpret_cast<const int16_t*>(p)[i];
        case 4: return reinterpret_cast<const int32_t*>(p)[i];
        default: return reinterpret_cast<const int64_t*>(p)[i];
    }
}

// One streaming pass over the logits in MEMORY order: a workgroup stages a tile of whole pixels in LDS with coalesced (16-byte when
// `vec`) loads, the next tile's loads are issued before the current one is scanned, then one thread per pixel gathers the pixel's
// target from the raster, scans its C floats and counts into the workgroup's histogram.  Pad columns are never addressed.
// Counter width: a workgroup counts at most CF_WG_PIXELS = 2^31 pixels (the host sizes the grid for it), so a 32-bit cell cannot wrap.
template <int HW>
__global__ __launch_bounds__(CF_THREADS) void confusion_ce_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                                  int tbytes, long missing, unsigned long long* __restrict__ cm,
                                                                  const CfGeom G) {
    __shared__ uint32_t hist[HW];
    __shared__ __attribute__((aligned(16))) float tile[CF_TILE];
    const int tid = threadIdx.x, C = G.C, CC = C * C;
    for (int i = tid; i < CC; i += CF_THREADS) hist[i] = 0;

    CfPrefetch pre;

    long t = blockIdx.x;
    CfTile T = cf_tile(G, t < G.n_tiles ? t : 0);
    if (G.vec && t < G.n_tiles) cf_prefetch(pre, logits, G, T, tid);
    __syncthreads();                                 // histogram zeroed
    for (; t < G.n_tiles; t += gridDim.x) {
        cf_stage(tile, pre, logits, G, T, tid);
        __syncthreads();
        const CfTile cur = T;
        const long nt = t + gridDim.x;
        if (nt < G.n_tiles) {
            T = cf_tile(G, nt);
            if (G.vec) cf_prefetch(pre, logits, G, T, tid);
        }
        const int npl = cur.nr * cur.pps, S = G.g * G.P, gg = G.g * G.g;
        for (int p = tid; p < npl; p += CF_THREADS) {
            const int r = p / cur.pps, q = cur.pix0 + (p - r * cur.pps);
            const long row = cur.row0 + r, b = row / gg;
            const int tok = (int)(row - b * gg), ty = tok / G.g, tx = tok - ty * G.g, p1 = q / G.P, p2 = q - p1 * G.P;
            const long tv = load_int(target, (b * S + (ty * G.P + p1)) * S + (tx * G.P + p2), tbytes);
            if (tv == missing || tv < 0 || tv >= C) continue;
            float best;
            const int arg = argmax_torch(tile + p * G.Cs, C, 1, best);
            atomicAdd(&hist[(int)tv * C + arg], 1u);
        }
        __syncthreads();
    }
    for (int i = tid; i < CC; i += CF_THREADS) {
        const uint32_t n = hist[i];
        if (n) atomicAdd(&cm[i], (unsigned long long)n);
    }
}

// Multilabel: one wave per row.  A row is used iff none of its targets equals `missing` (base.py:120-123); used rows count
// cm[l][t > 0.5][x > thr] (metric.py:154-166 with sigmoid(x) > p rewritten as x > logit(p)).  A workgroup counts at most
// B <= 2^31 - 1 rows per label: 32-bit counters cannot wrap.
constexpr int CB_MAX_C = 1024;
__global__ __launch_bounds__(256) void confusion_bce_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                            float missing, float thr, unsigned long long* __restrict__ cm, int B,
                                                            int C) {
    __shared__ uint32_t hist[CB_MAX_C * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < C * 4; i += 256) hist[i] = 0;
    __syncthreads();
    for (long b = (long)blockIdx.x * 4 + (tid >> 6); b < B; b += (long)gridDim.x * 4) {
        const float* t = target + b * C;
        const float* x = logits + b * C;
        bool hit = false;
        for (int l = lane; l < C; l += 64) hit = hit || t[l] == missing;
        if (__ballot(hit) != 0ull) continue;
        for (int l = lane; l < C; l += 64) atomicAdd(&hist[l * 4 + (t[l] > 0.5f ? 2 : 0) + (x[l] > thr ? 1 : 0)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < C * 4; i += 256) {
        const uint32_t n = hist[i];
        if (n) atomicAdd(&cm[i], (unsigned long long)n);
    }
}

}  // namespace

extern "C" int mh_confusion_ce(const float* logits, const void* target, int target_bytes, long missing_val, long long* cm, int B,
                               int g, int P, int C, int ld, void* stream) {
    MH_CHECK_ARG(logits && target && cm, "mh_confusion_ce: null pointer");
    MH_CHECK_ARG(B > 0 && g > 0 && P > 0, "mh_confusion_ce: B, g, P must be positive (got %d, %d, %d)", B, g, P);
    MH_CHECK_ARG(C >= 2 && C <= 128, "mh_confusion_ce: %d classes (2 ... 128 are supported)", C);
    MH_CHECK_ARG(target_bytes == 1 || target_bytes == 2 || target_bytes == 4 || target_bytes == 8,
                 "mh_confusion_ce: target width %d (1, 2, 4 or 8 bytes)", target_bytes);
    MH_CHECK_ARG((long)P * P * C <= (long)ld, "mh_confusion_ce: ld %d < P * P * C = %ld", ld, (long)P * P * C);
    MH_CHECK_ARG((long)g * P <= 46340 && (long)g * g <= (1L << 30), "mh_confusion_ce: raster side g * P = %ld too large", (long)g * P);
    const CfGeom G = cf_geometry(logits, (long)B * g * g, g, P, C, ld, false);
    // grid: workgroups resident at once (LDS: histogram + tile), each walking tiles blockIdx.x, + gridDim.x, ...; more of them
    // only when a workgroup would otherwise count more than CF_WG_PIXELS pixels into its 32-bit counters
    const int hw = C * C <= 1024 ? 1024 : (C * C <= 8192 ? 8192 : 16384);
    long grid = hw == 1024 ? 1024 : (hw == 8192 ? 768 : 512);
    const long wg_tiles = CF_WG_PIXELS / G.npt;
    grid = max(grid, (G.n_tiles + wg_tiles - 1) / wg_tiles);
    grid = min(grid, G.n_tiles);
    MH_CHECK_ARG(grid <= 0x7fffffffL, "mh_confusion_ce: problem too large");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(cm);
    if (hw == 1024)
        hipLaunchKernelGGL(confusion_ce_kernel<1024>, dim3((unsigned)grid), dim3(CF_THREADS), 0, s, logits, target, target_bytes, missing_val, out, G);
    else if (hw == 8192)
        hipLaunchKernelGGL(confusion_ce_kernel<8192>, dim3((unsigned)grid), dim3(CF_THREADS), 0, s, logits, target, target_bytes, missing_val, out, G);
    else
        hipLaunchKernelGGL(confusion_ce_kernel<16384>, dim3((unsigned)grid), dim3(CF_THREADS), 0, s, logits, target, target_bytes, missing_val, out, G);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_confusion_bce(const float* logits, const float* target, float missing_val, float logit_threshold, long long* cm,
                                int B, int C, void* stream) {
    MH_CHECK_ARG(logits && target && cm, "mh_confusion_bce: null pointer");
    MH_CHECK_ARG(B > 0, "mh_confusion_bce: B = %d", B);
    MH_CHECK_ARG(C >= 1 && C <= CB_MAX_C, "mh_confusion_bce: %d labels (1 ... %d are supported)", C, CB_MAX_C);
    const int grid = min(ceil_div(B, 4), 64);
    hipLaunchKernelGGL(confusion_bce_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, target, missing_val,
                       logit_threshold, reinterpret_cast<unsigned long long*>(cm), B, C);
    MH_LAUNCH_CHECK();
    return 0;
}
