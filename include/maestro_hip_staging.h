/* C ABI of libmaestro_hip.so, input staging: the median-date selection of multi-temporal rasters that the reference does per
 * sample on the CPU in maestro/dataset/dataset.py:188-220 (window cut 188-195, cloud mask 196-200, median and deviation 202-203,
 * random_dates 204-206, mean / nanargmin / gather 208-213, float cast, log and norm_fac 215-220).
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, every pointer is DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, keeps no global mutable
 * state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 = hipError_t; the message is
 * read with the main header's error call.  No atomics: the same call on the same operands writes the same bytes.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them; they then move
 * into maestro_hip.h.
 */
#ifndef MAESTRO_HIP_STAGING_H
#define MAESTRO_HIP_STAGING_H
#ifdef __cplusplus
extern "C" {
#endif

/* element type of `raw` */
#define MH_RAW_U8 0
#define MH_RAW_I16 1
#define MH_RAW_U16 2
#define MH_RAW_F32 3
#define MH_SELECT_MAX_WINDOW 64

/* One modality of one batch: out[b, j] = the date of window j of sample b that is closest to the window's per-pixel median.
 *
 *   raw        [B, Tmax, n_elem] of `raw_code` (n_elem = C * S * S, the raster of one date, dense)
 *   mask       u8 [B, Tmax, Cm, n_pix] or null (n_pix = S * S; n_elem % n_pix == 0): cloud / snow cover per pixel
 *   dates      i16 [B, Tmax, 3]
 *   t_start, t_win   i32 [B]: window j of sample b is the raw dates t_start[b] + j * W_b ... + W_b - 1, W_b = t_win[b]
 *              (dataset.py:92-104 and 189-190: t_start is the drawn start_mod_date, W_b = T_b / nd).  Samples are padded to Tmax;
 *              padding and dates outside the nd windows are never read.
 *   w_max      the largest W_b of the batch as the HOST knows it, 1 ... MH_SELECT_MAX_WINDOW: it sizes the workgroup's LDS.
 *   scores     f64 [B, Tmax] or null: given per-date scores (random_dates, dataset.py:204-206)
 *   out        f32 [B, nd, n_elem];  out_dates i16 [B, nd, 3];  out_index i32 [B, nd]: the chosen offset inside each window
 *
 * t_start / t_win live on the device and are TRUSTED: 0 <= t_start[b], 1 <= W_b <= w_max, t_start[b] + nd * W_b <= Tmax is the
 * caller's to check from its host copies (maestro_amd/hip.py does).  As a safety net a workgroup that finds its window outside
 * these limits reads and writes nothing but out_index[b, j] = -1.
 *
 * Per window (dataset.py:193-213):
 *   - a pixel of a date is masked iff any of its Cm mask values is > mask_floor (for an integer m, m > mask_threshold <=>
 *     m > floor(mask_threshold); the caller passes the floor, and no mask at all when mask_threshold >= 100, dataset.py:152);
 *   - a date is dirty iff any of its pixels is masked; if every date of the window is dirty the mask is ignored for that window
 *     (dataset.py:197-199);
 *   - per element the median over the window's unmasked dates (even count: the mean of the two middle values a, b; odd: a = b);
 *   - the score of a date is the sum over the elements of |x - median|; dirty dates are out, the lowest score wins, ties go to
 *     the lowest index (nanargmin).  The reference divides by n_elem (a mean): the same order.
 *   - integer raw data is exact: sum |2x - (a + b)| in int64 = 2 * n_elem * the reference's fp64 mean, which is itself exact
 *     (half-integers far below 2^53), so the choice is the reference's, ties included.
 *   - f32 raw data: median ((a + b) / 2 in fp32) and |x - median| in fp32 as numpy computes them; the score is summed in fp64 in
 *     element order 0 ... n_elem - 1.  That is this entry point's DEFINED semantics.  DEVIATION: the reference sums in fp32,
 *     pairwise, so the two can choose differently only when two scores agree to fp32 rounding (~1e-7 relative * sqrt(n_elem)).
 *     W_b = 2 on float data is a structural tie (|a - m| and |m - b| differ by rounding alone): the reference's own choice is
 *     rounding noise there, this one's is whatever the fp64 sums say, index 0 when they are equal.  f32 data inside the windows
 *     must not hold NaN (the reference would treat it as masked; here it takes part in no comparison).
 *   - scores given: median and score are skipped; the lowest given score among the clean dates wins (NaN scores are passed
 *     over; if no date qualifies, index 0).
 *   - output: the chosen date cast to f32; log_scale != 0: logf(x < 1e-10f ? 1e-10f : x); norm_fac > 0: one IEEE-rounded fp32
 *     division by norm_fac (never a reciprocal multiply: bit-identical to numpy's `/=`); norm_fac <= 0 = the reference's None.
 *
 * One launch, one workgroup per (sample, output date); B * nd <= 2^31 - 1, 1 <= nd <= Tmax, n_elem <= 2^31 - 1. */
int mh_select_dates(const void* raw, int raw_code, const unsigned char* mask, int Cm, int mask_floor, const short* dates,
                    const int* t_start, const int* t_win, int w_max, const double* scores, float* out, short* out_dates,
                    int* out_index, int B, int Tmax, int nd, long n_elem, int n_pix, int log_scale, float norm_fac, void* stream);

#ifdef __cplusplus
}
#endif
#endif
