// C declarations of the scene-prediction entry points (scene.hip): the window cut in front of the prediction path, the weighted
// accumulation of overlapping windows into a scene canvas behind it, and the canvas finish.  They follow every convention of
// include/maestro_hip.h -- no allocation, no synchronisation, the launch goes to `stream`, 0 on success, -1 for a refused
// argument and a hipError_t for a failed launch with the text in mh_last_error(), arguments checked before anything is launched,
// no environment reads -- and live here until they are folded into that header and the guard-band ledger of the tests.
//
// What they compute: the reference cuts its training crops on the host, every modality at its own pixel scale on one common
// grid of UNITS (maestro/dataset/dataset.py:86-105, the size_gcd / crop_gcd rule of maestro/conf/dataset/utils.py:99-109), and
// has no scene inference.  Here a window is W x W units, W the greatest common divisor of the model's raster sizes, and a raster
// with q pixels per unit shows the window (y0, x0) at pixels [y0 * q, y0 * q + S) x [x0 * q, x0 * q + S), S = W * q.
//
// The window table: int32 rows (n, y0, x0, on) -- scene index, window origin in units, 1 for a real window and 0 for a pad slot
// (pad slots are gathered, so the model sees finite data, and blend nothing).  Every entry point takes the table of the B slots
// twice, as mh_reduce_ordered takes its job table: `table_host` is checked before the launch, `table_dev` is what the kernel
// reads.  A row of `table_dev` that names no scene or leaves the raster is skipped on the device, never followed.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_SCENE_MAX_SLOTS 1024      // B of one launch
#define MH_SCENE_MAX_S 4096          // window side in pixels of mh_predict_blend (its profile sits in LDS)
#define MH_SCENE_UNCOVERED 255       // cls of a canvas pixel no window has reached

// out[b, p, y, x] = scene[n_b, p, y0_b * q + y, x0_b * q + x]: `scene` f32 [N, planes, Hs, Ws], `out` f32 [B, planes, S, S],
// planes = dates * channels.  Pure data movement, bit-exact.  16-byte loads and stores where both bases are 16-byte aligned and
// Ws, S and every x0 * q are multiples of 4, one float at a time otherwise (4-byte aligned bases).  Refused: a row of
// `table_host` with n outside 0 .. N - 1 or a window that leaves the scene.
int mh_window_gather(const float* scene, float* out, const int32_t* table_dev, const int32_t* table_host, int B, int N, int planes,
                     int Hs, int Ws, int S, int q, void* stream);

// The B windows of one batch onto the canvas.  `prob` f32 [B, C, S, S] (the sum over views mh_predict_view leaves), `profile`
// f32 [S], `acc` f32 [N, C, Hc, Wc], `wsum` f32 [N, Hc, Wc].  For every canvas pixel (n, Y, X) that at least one `on` slot covers,
// with b1 < b2 < ... the covering slots and w_b = profile[Y - y0_b * q] * profile[X - x0_b * q]:
//   wsum[n, Y, X]   = ((wsum + w_b1) + w_b2) ...
//   acc[n, c, Y, X] = ((acc + (prob[b1, c, ..] * scale) * w_b1) + (prob[b2, c, ..] * scale) * w_b2) ...
// every product and every sum a separately rounded fp32 operation (nothing is contracted into an FMA).  Pixels that no `on` slot
// covers are neither read nor written.  No atomics: the thread of the LOWEST covering slot owns the pixel and walks the slots in
// order, so the canvas bits depend on the order of the windows alone, not on how they are cut into launches.
// 2 <= C <= 128, B <= MH_SCENE_MAX_SLOTS, S <= MH_SCENE_MAX_S.  Refused: a row of `table_host` as for mh_window_gather.
int mh_predict_blend(const float* prob, float scale, const float* profile, const int32_t* table_dev, const int32_t* table_host,
                     float* acc, float* wsum, int B, int N, int C, int S, int q, int Hc, int Wc, void* stream);

// After the last batch.  `acc` f32 [N, C, n_pix], `wsum` f32 [N, n_pix], n_pix = Hc * Wc.
//   cls  u8  [N, n_pix]: the arg-max over c of acc under the rule of mh_predict_view (one device function: the lowest index among
//        equal maxima, a NaN is the maximum and the first NaN wins)
//   conf f32 [N, n_pix]: that maximum / wsum;  mean f32 [N, C, n_pix] (may be `acc` itself) = acc / wsum
// with correctly rounded divisions; wsum == 0 (no window reached the pixel): cls = MH_SCENE_UNCOVERED, conf = 0, mean = 0.
// Each of cls, conf and mean may be NULL, not all three.  2 <= C <= 128.
int mh_predict_blend_finish(const float* acc, const float* wsum, uint8_t* cls, float* conf, float* mean, int N, int C, long n_pix,
                            void* stream);

#ifdef __cplusplus
}
#endif
