/* C ABI of libmaestro_hip.so, prediction metrics of the probe / finetune branch: the confusion matrices that
 * maestro/train/metric.py keeps per target and stage (fed on every supervised step from maestro/train/base.py:143-146).
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, every pointer is DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, keeps no global mutable
 * state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 = hipError_t; the message is
 * read with the main header's error call.  Results are integers: exact, and independent of the launch order (no float
 * atomics; 32-bit LDS counters per workgroup, 64-bit integer atomics into `cm`).
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them; they then move
 * into maestro_hip.h.
 */
#ifndef MAESTRO_HIP_METRICS_H
#define MAESTRO_HIP_METRICS_H
#ifdef __cplusplus
extern "C" {
#endif

/* Mono-label confusion matrix (maestro/train/metric.py:63-77 "multiclass": argmax over the classes, then
 * torchmetrics.functional.confusion_matrix; the selection of valid entries is maestro/train/base.py:120-138).
 * Operands as the cross-entropy loss entry point of maestro_hip.h (csrc/heads.hip): `logits` f32 at patch layout
 * [B*g*g, ld >= P*P*C], columns (p1*P + p2)*C + c (PixelifyBands' '(p1 p2 c)', maestro/layers/embed.py:153-160); `target` the
 * [B, S, S] raster, S = g*P, signed integers of `target_bytes` = 1, 2, 4 or 8 bytes; classification is g = P = 1.
 *   for every pixel with t != missing_val && 0 <= t < C:   cm[t*C + argmax_c logits] += 1
 * `cm` is int64 [C, C], rows = targets, columns = predictions (torchmetrics' orientation, metric.py:83-84); the call ADDS,
 * the caller zeroes.  The arg-max is torch.argmax's: the lowest index among equal maxima; a NaN compares as the maximum and
 * the first NaN wins.  One pass: every logit is read once, in memory order (16-byte loads when ld % 4 == 0 and `logits` is
 * 16-byte aligned; any ld and 4-byte alignment are accepted); pad columns (ld > P*P*C) are never read.
 * 2 <= C <= 128; ld >= P*P*C; g*P <= 46340. */
int mh_confusion_ce(const float* logits, const void* target, int target_bytes, long missing_val, long long* cm, int B, int g,
                    int P, int C, int ld, void* stream);

/* Multilabel confusion matrices (maestro/train/metric.py:154-160 "multilabel", read at metric.py:164-166; also the binary
 * 2x2 of "change_detect", metric.py:68-77, with C = 1).  Operands as the BCE loss entry point: `logits`, `target` f32 [B, C]
 * dense.  A row is used iff none of its targets equals missing_val (base.py:120-123); for every used (b, l)
 *   cm[l][target > 0.5 ? 1 : 0][logit > logit_threshold ? 1 : 0] += 1,      cm int64 [C, 2, 2], the call ADDS.
 * DEVIATION from the reference, which tests sigmoid(logit) > thr in fp32: the host passes logit_threshold =
 * log(thr / (1 - thr)) (0 for the reference's 0.5).  The two forms differ only where the fp32 sigmoid rounds onto thr, i.e. for
 * |logit - logit_threshold| below about 1e-7.
 * 1 <= C <= 1024. */
int mh_confusion_bce(const float* logits, const float* target, float missing_val, float logit_threshold, long long* cm, int B,
                     int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
