/* C ABI of libmaestro_hip.so, AdamW with bf16 moments: both Adam moments stored as bf16 with stochastic rounding inside the
 * one fused launch.  The update stream drops from 30 to 22 bytes per parameter (p 8, g 4, m16 4, v16 4, bf16 shadow 2) and
 * the optimizer state from 8 to 4 bytes per parameter.
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, device pointers are DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, reads no environment, keeps
 * no global mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 =
 * hipError_t; the message is read with the main header's error call.  No atomics.
 *
 * ARITHMETIC.  The update is mh_adamw's, one function in the library.  Per element: the stored moments are upcast exactly
 * (bits << 16); the new fp32 moments, the weight decay and the parameter step are computed as mh_adamw computes them -- the
 * parameter therefore moves by the UNROUNDED new moments; each new moment is then stored as bf16 by stochastic rounding.  A
 * launch gives the p / p_bf16 bits of mh_adamw started from the upcast moments.
 *
 * STOCHASTIC ROUNDING, on bits.  u = the fp32 pattern, r = a 16-bit random word:
 *     u inf or NaN:  store u >> 16; a NaN whose surviving mantissa bits are all zero gets the quiet bit (0x0040)
 *     else t = u + r:  t carried into an all-ones exponent -> store u >> 16 (stays finite), else store t >> 16
 * The magnitude goes up with probability low16(u) / 65536: a value representable in bf16 is stored exactly, the expectation
 * of the stored value is the fp32 value, negative values mirror positive ones, v stays non-negative.
 *
 * RANDOM WORDS.  Philox4x32-10 as in maestro_hip_rng.h (same multipliers, key increments and rounds), one call per quad of
 * elements: key = (seed & 0xffffffff, seed >> 32), counter
 *     c0 = (elem_base + i) / 4 (low 32 bits),   c1 = step (low 32 bits),   c2 = 0,   c3 = MH_ADAMW_SR_TAG
 * and element e = (elem_base + i) % 4 of the quad takes
 *     m:  (w[e >> 1] >> 16 * (e & 1)) & 0xffff        v:  (w[2 + (e >> 1)] >> 16 * (e & 1)) & 0xffff
 * elem_base is the offset of p[0] in the caller's flat layout: a split launch, a slice and one whole launch store the same
 * bits.  step is Adam's t after the increment.  MH_ADAMW_SR_TAG differs from every c3 of the mask draws (kind | stream << 4 |
 * attempt << 16 stays below 2^22 there), so no counter of this header is a counter of maestro_hip_rng.h under the same seed.
 *
 * p, g: f32, 16-byte aligned; m16, v16, p_bf16 (may be null): bf16, 8-byte aligned (one 8-byte store per quad each).
 * n > 0, n % 4 == 0, elem_base >= 0, elem_base % 4 == 0 (% 64 in the grouped forms: the map has one byte per 64 elements),
 * step >= 1.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them.
 */
#ifndef MAESTRO_HIP_MOMENTS_H
#define MAESTRO_HIP_MOMENTS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MH_ADAMW_SR_TAG 0x5352424Du /* c3 of every rounding draw ("SRBM") */

/* mh_adamw with bf16 moments. */
int mh_adamw_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed, float lr,
                   float b1, float b2, float eps, float wd, int step, float grad_scale, void* stream);

/* mh_adamw_dev with bf16 moments: hyper = {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active} (mh_adamw_dev's float[5]), step_dev =
 * a device word holding Adam's t (MhGuardState.t, read after mh_grad_guard_finish): its low 32 bits are the counter's step.
 * With hyper[4] == 0 the kernel returns before it touches memory. */
int mh_adamw_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed,
                       float b1, float b2, float eps, float wd, const float* hyper, const long long* step_dev, void* stream);

/* mh_adamw_groups with bf16 moments: group_of, lr_scale, wd as in maestro_hip_optim.h (p starts on a 64-element block of the
 * layout the map was built for, so elem_base % 64 == 0). */
int mh_adamw_groups_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                          const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float lr, float b1,
                          float b2, float eps, int step, float grad_scale, void* stream);

/* mh_adamw_groups_dev with bf16 moments (hyper and step_dev as above). */
int mh_adamw_groups_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                              const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float b1, float b2,
                              float eps, const float* hyper, const long long* step_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
