// Predictions from the resident head logits: class maps, confidences and class probabilities, one dihedral view at a time, and the
// finish after several accumulated views (test-time augmentation).  C declarations and the full contract: include/maestro_hip.h.
//
// The softmax kernel is the walk of confusion_ce_kernel (logits_walk.hpp) writing a prediction instead of a histogram: tiles of
// whole pixels staged in LDS by 16-byte loads in memory order, the next tile's loads in flight, one thread per pixel scanning its C
// floats in LDS (no per-thread class array).  Nothing here is atomic: every output element has one writer.
#include "common.hpp"
#include "logits_walk.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr int PV_MAX_GRID = 2048;     // 256 CUs x 8 resident workgroups (16 KiB of LDS each)
constexpr int PS_MAX_C = 1024;        // labels of the sigmoid form (mh_confusion_bce's limit)

// View pixel (y, x) of sample b -> (y0, x0) of the untransformed raster (the inverse of dihedral_kernel, embed.hip).
__device__ __forceinline__ void undo_dihedral(unsigned f, int S, int y, int x, int& y0, int& x0) {
    y0 = (f & 4) ? x : y;
    x0 = (f & 4) ? y : x;
    if (f & 2) x0 = S - 1 - x0;
    if (f & 1) y0 = S - 1 - y0;
}

// a * b rounded on its own: never contracted into an FMA with a following sum (the build's default allows that), so that an
// accumulating view adds the very number it would have written alone.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__global__ __launch_bounds__(CF_THREADS) void predict_view_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ flags,
                                                                  float* __restrict__ prob, int accumulate, uint8_t* __restrict__ cls,
                                                                  float* __restrict__ conf, const CfGeom G) {
    __shared__ __attribute__((aligned(16))) float tile[CF_TILE];
    const int tid = threadIdx.x, C = G.C, S = G.g * G.P, gg = G.g * G.g;
    const size_t plane = (size_t)S * S;
    CfPrefetch pre;
    long t = blockIdx.x;                              // the grid has at most n_tiles workgroups
    CfTile T = cf_tile(G, t);
    if (G.vec) cf_prefetch(pre, logits, G, T, tid);
    for (; t < G.n_tiles; t += gridDim.x) {
        cf_stage(tile, pre, logits, G, T, tid);
        __syncthreads();
        const CfTile cur = T;
        const long nt = t + gridDim.x;
        if (nt < G.n_tiles) {
            T = cf_tile(G, nt);
            if (G.vec) cf_prefetch(pre, logits, G, T, tid);
        }
        const int npl = cur.nr * cur.pps;
        for (int p = tid; p < npl; p += CF_THREADS) {
            const int r = p / cur.pps, q = cur.pix0 + (p - r * cur.pps);
            const long row = cur.row0 + r, b = row / gg;
            const int tok = (int)(row - b * gg), ty = tok / G.g, tx = tok - ty * G.g, p1 = q / G.P, p2 = q - p1 * G.P;
            int y0, x0;
            undo_dihedral(flags ? flags[b] : 0u, S, ty * G.P + p1, tx * G.P + p2, y0, x0);
            const size_t o = (size_t)y0 * S + x0;
            float* x = tile + p * G.Cs;               // this thread's pixel: nobody else touches these C floats
            float m;
            const int arg = argmax_torch(x, C, 1, m);
            if (cls) cls[b * plane + o] = (uint8_t)arg;
            if (!prob && !conf) continue;
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                const float e = __expf(x[c] - m);
                s += e;
                x[c] = e;
            }
            const float inv = 1.f / s;
            if (conf) conf[b * plane + o] = inv;
            if (prob) {
                float* out = prob + (size_t)b * C * plane + o;
                if (accumulate)
                    for (int c = 0; c < C; ++c) out[c * plane] += mul_rounded(x[c], inv);
                else
                    for (int c = 0; c < C; ++c) out[c * plane] = mul_rounded(x[c], inv);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float sigmoid_f32(float l) { return 1.f / (1.f + __expf(-l)); }     // the form of bce_loss (heads.hip)

__global__ __launch_bounds__(256) void predict_sigmoid_kernel(const float* __restrict__ logits, float thr, float* __restrict__ prob,
                                                              int accumulate, uint8_t* __restrict__ cls, float* __restrict__ conf,
                                                              long n, int C, int ld) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long b = i / C;
        const float l = logits[b * ld + (i - b * C)], s = sigmoid_f32(l);
        if (cls) cls[i] = l > thr ? 1 : 0;
        if (conf) conf[i] = s;
        if (prob) prob[i] = accumulate ? prob[i] + s : s;
    }
}

// Four pixels of one sample per thread: the C planes are read with 16-byte loads, coalesced over the pixels.
typedef __attribute__((ext_vector_type(4))) uint8_t u8x4;
__global__ __launch_bounds__(256) void predict_finish4_kernel(const float* prob, float inv_views, uint8_t* __restrict__ cls,
                                                              float* __restrict__ conf, float* mean, long n_items, int C, long n_pix) {
    const long per = n_pix / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (long)gridDim.x * 256) {
        const long b = i / per, pix = (i - b * per) * 4;
        const float* x = prob + (size_t)b * C * n_pix + pix;
        float* mu = mean ? mean + (size_t)b * C * n_pix + pix : nullptr;     // (may be x itself: element c is read before it is written)
        f32x4 best = *reinterpret_cast<const f32x4*>(x);
        if (mu) *reinterpret_cast<f32x4*>(mu) = best * inv_views;
        u8x4 arg = 0;
        for (int c = 1; c < C; ++c) {                 // the rule of argmax_torch, four pixels side by side
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)c * n_pix);
            if (mu) *reinterpret_cast<f32x4*>(mu + (size_t)c * n_pix) = v * inv_views;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v[j] > best[j] || (v[j] != v[j] && best[j] == best[j])) { best[j] = v[j]; arg[j] = (uint8_t)c; }
        }
        if (cls) *reinterpret_cast<u8x4*>(cls + b * n_pix + pix) = arg;
        if (conf) *reinterpret_cast<f32x4*>(conf + b * n_pix + pix) = best * inv_views;
    }
}

__global__ __launch_bounds__(256) void predict_finish_kernel(const float* prob, float inv_views, uint8_t* __restrict__ cls,
                                                             float* __restrict__ conf, float* mean, long n_items, int C, long n_pix) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (long)gridDim.x * 256) {
        const long b = i / n_pix, pix = i - b * n_pix;
        const size_t o = (size_t)b * C * n_pix + pix;
        float best;
        const int arg = argmax_torch(prob + o, C, (size_t)n_pix, best);
        if (cls) cls[i] = (uint8_t)arg;
        if (conf) conf[i] = best * inv_views;
        if (mean)                                     // after the scan: `mean` may be `prob` itself
            for (int c = 0; c < C; ++c) mean[o + (size_t)c * n_pix] = prob[o + (size_t)c * n_pix] * inv_views;
    }
}

__global__ __launch_bounds__(256) void predict_finish_sigmoid_kernel(const float* prob, float inv_views, float thr,
                                                                     uint8_t* __restrict__ cls, float* __restrict__ conf, float* mean,
                                                                     long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float p = prob[i] * inv_views;
        if (cls) cls[i] = p > thr ? 1 : 0;
        if (conf) conf[i] = p;
        if (mean) mean[i] = p;
    }
}

inline unsigned flat_grid(long n) { return (unsigned)min((n + 255) / 256, 4096L); }

}  // namespace

extern "C" int mh_predict_view(const float* logits, const uint8_t* flags, int act, float threshold, float* prob, int accumulate,
                               uint8_t* cls, float* conf, int B, int g, int P, int C, int ld, void* stream) {
    MH_CHECK_ARG(logits, "mh_predict_view: null logits");
    MH_CHECK_ARG(prob || cls || conf, "mh_predict_view: no output (prob, cls and conf are all null)");
    MH_CHECK_ARG(act == MH_PREDICT_SOFTMAX || act == MH_PREDICT_SIGMOID, "mh_predict_view: activation %d (0 softmax, 1 sigmoid)", act);
    MH_CHECK_ARG(B > 0 && g > 0 && P > 0, "mh_predict_view: B, g, P must be positive (got %d, %d, %d)", B, g, P);
    hipStream_t s = (hipStream_t)stream;
    if (act == MH_PREDICT_SIGMOID) {
        MH_CHECK_ARG(C >= 1 && C <= PS_MAX_C, "mh_predict_view: %d labels (1 ... %d are supported by the sigmoid)", C, PS_MAX_C);
        MH_CHECK_ARG(g == 1 && P == 1, "mh_predict_view: the sigmoid is for classification heads, g = P = 1 (got %d, %d)", g, P);
        MH_CHECK_ARG(C <= ld, "mh_predict_view: ld %d < C = %d", ld, C);
        const long n = (long)B * C;
        hipLaunchKernelGGL(predict_sigmoid_kernel, dim3(flat_grid(n)), dim3(256), 0, s, logits, threshold, prob, accumulate, cls, conf,
                           n, C, ld);
        MH_LAUNCH_CHECK();
        return 0;
    }
    MH_CHECK_ARG(C >= 2 && C <= 128, "mh_predict_view: %d classes (2 ... 128 are supported by the softmax)", C);
    MH_CHECK_ARG((long)P * P * C <= (long)ld, "mh_predict_view: ld %d < P * P * C = %ld", ld, (long)P * P * C);
    MH_CHECK_ARG((long)g * P <= 46340 && (long)g * g <= (1L << 30), "mh_predict_view: raster side g * P = %ld too large", (long)g * P);
    const CfGeom G = cf_geometry(logits, (long)B * g * g, g, P, C, ld, true);
    const long grid = min(G.n_tiles, (long)PV_MAX_GRID);
    hipLaunchKernelGGL(predict_view_kernel, dim3((unsigned)grid), dim3(CF_THREADS), 0, s, logits, flags, prob, accumulate, cls, conf, G);
    MH_LAUNCH_CHECK();
    return 0;
}

extern "C" int mh_predict_finish(const float* prob, float inv_views, int act, float threshold, uint8_t* cls, float* conf, float* mean,
                                 int B, int C, long n_pix, void* stream) {
    MH_CHECK_ARG(prob, "mh_predict_finish: null prob");
    MH_CHECK_ARG(cls || conf || mean, "mh_predict_finish: no output (cls, conf and mean are all null)");
    MH_CHECK_ARG(act == MH_PREDICT_SOFTMAX || act == MH_PREDICT_SIGMOID, "mh_predict_finish: activation %d (0 softmax, 1 sigmoid)", act);
    MH_CHECK_ARG(B > 0 && n_pix > 0 && n_pix <= 46340L * 46340L, "mh_predict_finish: B = %d, n_pix = %ld", B, n_pix);
    MH_CHECK_ARG(inv_views > 0.f && inv_views <= 1.f, "mh_predict_finish: inv_views = %g (1 / the number of views)", (double)inv_views);
    hipStream_t s = (hipStream_t)stream;
    if (act == MH_PREDICT_SIGMOID) {
        MH_CHECK_ARG(C >= 1 && C <= PS_MAX_C, "mh_predict_finish: %d labels (1 ... %d are supported by the sigmoid)", C, PS_MAX_C);
        MH_CHECK_ARG(n_pix == 1, "mh_predict_finish: the sigmoid is for classification heads, n_pix = 1 (got %ld)", n_pix);
        const long n = (long)B * C;
        hipLaunchKernelGGL(predict_finish_sigmoid_kernel, dim3(flat_grid(n)), dim3(256), 0, s, prob, inv_views, threshold, cls, conf,
                           mean, n);
        MH_LAUNCH_CHECK();
        return 0;
    }
    MH_CHECK_ARG(C >= 2 && C <= 128, "mh_predict_finish: %d classes (2 ... 128 are supported by the softmax)", C);
    const bool vec = n_pix % 4 == 0 && (uintptr_t)prob % 16 == 0 && (uintptr_t)conf % 16 == 0 && (uintptr_t)mean % 16 == 0 &&
                     (uintptr_t)cls % 4 == 0;
    if (vec) {
        const long n = (long)B * (n_pix / 4);
        hipLaunchKernelGGL(predict_finish4_kernel, dim3(flat_grid(n)), dim3(256), 0, s, prob, inv_views, cls, conf, mean, n, C, n_pix);
    } else {
        const long n = (long)B * n_pix;
        hipLaunchKernelGGL(predict_finish_kernel, dim3(flat_grid(n)), dim3(256), 0, s, prob, inv_views, cls, conf, mean, n, C, n_pix);
    }
    MH_LAUNCH_CHECK();
    return 0;
}
