/* C ABI of libmaestro_hip.so, gradient guard: the global L2 norm of the flat gradient buffer, the clipping coefficient and the
 * non-finite skip, computed on the device and handed to mh_adamw_dev through its five device scalars.
 *
 * What it answers in the reference: the trainer runs precision="16-mixed" (maestro/conf/trainer.py:13), so Lightning's GradScaler
 * skips the optimizer step of maestro/train/model.py:135-140 (AdamW + OneCycleLR) whenever a gradient is inf / NaN, and a
 * Trainer(gradient_clip_val=...) clips by the global norm with torch.nn.utils.clip_grad_norm_, whose coefficient rule
 *     coef = min(1, max_norm / (norm + 1e-6))
 * is restated here.  A skipped step does not advance Adam's step count (GradScaler semantics).
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, device pointers are DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, reads no environment, keeps
 * no global mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 =
 * hipError_t; the message is read with the main header's error call.  No atomics: every sum has ONE order, fixed by the
 * arguments, so the same gradient gives the same bits on every run and on every rank.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them.
 */
#ifndef MAESTRO_HIP_GUARD_H
#define MAESTRO_HIP_GUARD_H
#ifdef __cplusplus
extern "C" {
#endif

/* Elements per workgroup of the first phase (256 threads, 16 float4 loads per lane).  Why 16384: a lane's 16 loads (64 registers)
 * leave before the first is consumed and the kernel, at 72 registers, still runs 7 waves per SIMD; the C3 gradient (176 M elements) gives
 * 10.7 k workgroups = 42 per CU, so the ragged tail of the grid is 2 % of it; and the partials of that buffer (43 KB + 43 KB)
 * are summed by the ONE workgroup of the second phase in 42 strided loads per thread.  A smaller chunk lengthens that serial
 * second phase, a larger one leaves the small trainable spans (probe: a few workgroups) with even fewer.  The partial layout
 * is a function of n alone. */
#define MH_GUARD_CHUNK 16384

/* Caller-owned DEVICE struct, zeroed once; mh_grad_guard_finish reads and writes it. */
typedef struct {
    float norm;          /* |grad_scale| * sqrt(sum g^2) of the last call */
    float coef;          /* clipping coefficient of the last call (1 = not clipped) */
    int finite;          /* 1: the norm is finite and no element was inf / NaN */
    unsigned bad;        /* number of inf / NaN elements (saturating) */
    long long t;         /* Adam's step count: advanced by every APPLIED step */
    long long skipped;   /* number of skipped steps */
} MhGuardState;

/* ceil(n / MH_GUARD_CHUNK): rows of `partial` and `bad` for a gradient of n elements (0 for n <= 0). */
long mh_grad_sumsq_partial_rows(long n);

/* First phase.  Workgroup i: partial[i] = sum of g[j]^2 and bad[i] = number of j whose exponent bits are all ones (inf, NaN),
 * j in [i * MH_GUARD_CHUNK, min(n, (i + 1) * MH_GUARD_CHUNK)); plain stores, every row is written.  g: f32, 16-byte aligned,
 * n > 0, n % 4 == 0.  Order of the additions: lane (of 256) l accumulates acc[c] = fma(g, g, acc[c]) over its float4s
 * k = 0 ... 15 at element 4 * (256 * k + l) + c of the chunk, in k order, c = 0 ... 3; lane sum (acc[0] + acc[1]) + (acc[2] + acc[3]);
 * xor-butterfly over the wave (offsets 32, 16, ... 1); ((w0 + w1) + w2) + w3 over the four waves. */
int mh_grad_sumsq_partial(const float* g, long n, float* partial, unsigned* bad, void* stream);

/* Second phase, one workgroup.  rows = mh_grad_sumsq_partial_rows(n) of the first phase (1 <= rows <= 2^24).
 *   S      = sum of partial[0 ... rows) in double (thread l of 256: rows l, l + 256, ... in order; then a fixed binary tree)
 *   norm   = (float)(|grad_scale| * sqrt(S));   bad = min(sum of bad[i], UINT_MAX)
 *   finite = isfinite(norm) && bad == 0        (a finite gradient whose sum of squares overflows fp32 counts as non-finite)
 *   coef   = (max_norm > 0 && finite) ? min(1, max_norm / (norm + 1e-6f)) : 1
 *   apply  = finite || !skip_nonfinite;  apply ? state->t += 1 : state->skipped += 1
 *   hyper[0 ... 5) = {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale * coef, apply ? 1 : 0}   with t after the increment, the two
 *            correction terms computed in double from the float b1 / b2 and rounded once -- mh_adamw_dev's five scalars.
 * norm, coef, finite, bad are stored in *state.  grad_scale, max_norm, lr finite (max_norm <= 0: no clipping), 0 <= b1, b2 < 1. */
int mh_grad_guard_finish(const float* partial, const unsigned* bad, long rows, float grad_scale, float max_norm,
                         int skip_nonfinite, float lr, float b1, float b2, float* hyper, MhGuardState* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif
