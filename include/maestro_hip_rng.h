/* C ABI of libmaestro_hip.so, device-side mask draws: the structural Bernoulli masks and the per-token noise of the masking
 * step that the reference draws from torch's generator in maestro/ssl/mae.py:178-246 (structural masks with their rejection
 * loop 178-226, the rand(B, L) noise and its argsort 228-246), restated on a counter-based generator so that the draws of a
 * step are a pure function of (seed, step, global sample index).
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, device pointers are DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, reads no environment, keeps
 * no global mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 =
 * hipError_t; the message is read with the main header's error call.  No atomics.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them; they then move
 * into maestro_hip.h.
 *
 * THE DRAW FUNCTION.  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds), key = (seed & 0xffffffff, seed >> 32), counter
 *     c0 = i >> 2,   c1 = global row,   c2 = step,   c3 = kind | stream << 4 | attempt << 16
 * and U(seed, step, stream, kind, row, attempt, i) = (float)(word[i & 3] >> 8) * 2^-24: 24 bits in [0, 1), the value set of
 * torch.rand.  kind: 0 noise (i = token, attempt 0), 1 mod (i = 0), 2 bands (i = band-group), 3 dates (i = date slot),
 * 4 loc (i = token of the modality's grid).  A Bernoulli draw is U < p with p as float32.
 */
#ifndef MAESTRO_HIP_RNG_H
#define MAESTRO_HIP_RNG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MH_MASK_KIND_NOISE 0
#define MH_MASK_KIND_MOD 1
#define MH_MASK_KIND_BANDS 2
#define MH_MASK_KIND_DATES 3
#define MH_MASK_KIND_LOC 4
#define MH_MASK_MAX_ATTEMPTS 64   /* the counted rejection loop: a row that is all-masked 64 times is stored all-clear */
#define MH_MASK_MAX_L 8192
#define MH_MASK_MAX_STREAMS 4096  /* stream ids are 12 bits of c3 */

/* One modality (or band-group) inside a group's token row: tokens tok_off ... tok_off + D * L - 1, token (d, l) at d * L + l.
 * mk(d, l) = OR over the active kinds of (U < p): mod at i = 0, bands at i = gi, dates at i = d, loc at i = l, all on `stream`
 * (the modality's index) and the structural row; p < 0 (or 0) = the kind is off (the reference's None). */
typedef struct {
    int tok_off, D, L, gi, G, stream;
    float p_mod, p_bands, p_dates, p_loc;
} MhMaskSeg;

/* One group: noise f32 [Beff, L] and struct u8 [Beff, L] (dense rows; 1 = structurally masked).
 *   structural row of r:  row_base * struct_rpb + r
 *   noise row of r:       row_base * noise_rpb + (r / row_div) * row_mul + row_add + r % row_div
 * (the affine map picks rows (b, draw_g, d) of a [B, draw_G, D] draw: row_div = D, row_mul = draw_G * D, row_add = draw_g * D;
 * 1, 1, 0 = the identity).  *_rpb = rows of the draw tensor per sample.  Segments seg0 ... seg0 + n_segs - 1 of the segment
 * table tile [0, L) in order.  The row kept is that of the first attempt a = 0, 1, ... whose row is not all-masked. */
typedef struct {
    float* noise;
    unsigned char* strct;
    int Beff, L;
    int noise_stream, noise_rpb, struct_rpb;
    int row_div, row_mul, row_add;
    int seg0, n_segs;
} MhMaskJob;

/* All groups of a step in ONE launch (one workgroup per (group, row)).  The tables are given twice: the host copies are
 * checked before the launch (null pointers, 1 <= L <= MH_MASK_MAX_L, segments that do not tile the row, stream ids, row
 * indices that leave 32 bits), the device copies are what the kernel reads.  n_jobs >= 1, 0 <= step <= 2^32 - 1,
 * row_base >= 0; seed, step and row_base are by-value: nothing of a step is baked into a captured graph's table. */
int mh_mask_draw(const MhMaskJob* jobs_host, const MhMaskJob* jobs_device, int n_jobs, const MhMaskSeg* segs_host,
                 const MhMaskSeg* segs_device, int n_segs, uint64_t seed, long long step, long long row_base, void* stream);

#ifdef __cplusplus
}
#endif
#endif
