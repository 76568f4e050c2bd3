// C declarations of the prediction entry points (predict.hip).  They follow every convention of include/maestro_hip.h -- no
// allocation, no synchronisation, the launch goes to `stream`, 0 on success, -1 for a refused argument and a hipError_t for a
// failed launch with the text in mh_last_error(), arguments checked before anything is launched, no environment reads -- and live
// here only until they are folded into that header and the guard-band ledger of the tests.
//
// What they compute: the reference has no prediction path; a user of it takes the head's logits [B, 1, C, S, S]
// (maestro/layers/head.py:116-130), torch.argmax over the class axis (maestro/layers/overlay.py:11-23) and, for a confidence,
// torch.softmax.  Test-time augmentation undoes the transforms the models are trained under (maestro/dataset/dataset.py:224-257:
// per sample, flip the rows, flip the columns, swap the two axes, in this order; the flag byte of mh_dihedral).
//
// Operands as for mh_ce_loss / mh_confusion_ce: `logits` is f32 in patch layout [B * g * g, ld >= P * P * C], column
// (p1 * P + p2) * C + c of token row (b * g + ty) * g + tx is class c of pixel (ty * P + p1, tx * P + p2) of the S x S raster,
// S = g * P; classification heads are g = P = 1.  Any ld and a 4-byte aligned base are accepted, 16-byte loads are used where
// ld % 4 == 0 and the base is 16-byte aligned, pad columns are never read, every logit is read once.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_PREDICT_SOFTMAX 0
#define MH_PREDICT_SIGMOID 1

// One view of the batch.  `flags` (u8 [B], or NULL = identity) is the mh_dihedral flag byte that produced sample b's view: bit 0
// flipped the rows, bit 1 the columns, bit 2 then swapped the axes.  Pixel (y, x) of the view is written at its place (y0, x0) of
// the UNTRANSFORMED raster:  (y0, x0) = bit 2 ? (x, y) : (y, x);  bit 1: x0 = S - 1 - x0;  bit 0: y0 = S - 1 - y0.
//
// act = MH_PREDICT_SOFTMAX (2 <= C <= 128), in fp32 with m = max_j l_j:
//   prob  f32 raster [B, C, S, S] (the layout of the logits a reference user holds):
//         prob[b, c, y0, x0] = (accumulate ? old : 0) + exp(l_c - m) / sum_j exp(l_j - m) -- a plain read-modify-write by the one
//         thread that owns the pixel; no atomics
//   cls   u8 [B, S, S]: torch.argmax of the logits -- the lowest index among equal maxima, a NaN is the maximum and the first NaN
//         wins (the rule of mh_confusion_ce, one device function)
//   conf  f32 [B, S, S]: 1 / sum_j exp(l_j - m), the largest class probability
// act = MH_PREDICT_SIGMOID (1 <= C <= 1024, g = P = 1, flags ignored), `threshold` a LOGIT threshold (the decision of
// mh_confusion_bce):
//   prob  f32 [B, C] (+)= 1 / (1 + exp(-l));  cls u8 [B, C] = l > threshold;  conf f32 [B, C] = 1 / (1 + exp(-l))
// Each of prob, cls and conf may be NULL, not all three.  `threshold` is ignored for the softmax.
int mh_predict_view(const float* logits, const uint8_t* flags, int act, float threshold, float* prob, int accumulate, uint8_t* cls,
                    float* conf, int B, int g, int P, int C, int ld, void* stream);

// After 1 / inv_views accumulated views.  `prob` is [B, C, n_pix] (n_pix = S * S, or 1 for classification heads).
//   softmax: cls[b, pix] = arg-max over c of prob[b, c, pix] under the same rule, conf[b, pix] = max * inv_views
//   sigmoid: cls[b, c] = prob * inv_views > threshold (`threshold` a PROBABILITY here), conf[b, c] = prob * inv_views (n_pix = 1)
//   mean (f32, the shape of prob; may be prob itself) = prob * inv_views, the mean probabilities: conf is their largest, bit for bit
// Each of cls, conf and mean may be NULL, not all three.
int mh_predict_finish(const float* prob, float inv_views, int act, float threshold, uint8_t* cls, float* conf, float* mean, int B, int C,
                      long n_pix, void* stream);

#ifdef __cplusplus
}
#endif
