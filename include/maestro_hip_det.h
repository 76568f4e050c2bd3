/* C ABI of libmaestro_hip.so, deterministic mode: an ordered fp32 reduction and the atomic-free first phases of the
 * reductions of the pretraining step ("Deterministic mode").
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, every pointer is DEVICE memory owned by the caller unless
 * its name ends in _host; asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates no device
 * memory, keeps no global mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched),
 * >0 = hipError_t; the message is read with the main header's error call.  No entry point here issues a floating-point atomic:
 * every output element is written by exactly one plain store per launch, so the bits of a result depend on the operands alone
 * and not on the order in which the hardware runs the workgroups.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them; they then move
 * into maestro_hip.h ("Deterministic mode").
 */
#ifndef MAESTRO_HIP_DET_H
#define MAESTRO_HIP_DET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MH_ORDERED_ROWS 16        /* rows per chunk of the ordered reduction */
#define MH_ORDERED_ADD 1          /* MhOrderedJob.flags bit 0: add to the value dst holds (default: overwrite) */
#define MH_COLSUM_PARTIAL_ROWS 256 /* rows per row block of mh_colsum_partial: a constant, so the partial layout depends on M alone */

/* One job of mh_reduce_ordered: src f32 [rows, ld] (cols <= ld), dst f32 [cols]. */
typedef struct MhOrderedJob {
    const float* src;
    float* dst;
    int rows, cols, ld, flags;
} MhOrderedJob;

/* Ordered column sums.  Jobs that share a `dst` are ADJACENT in the table and form a chain (same cols and flags throughout).
 * The result is defined exactly; every operation is an IEEE fp32 round-to-nearest add, nothing is reassociated:
 *   chunk_k[c]    = ((+0 + src[16k][c]) + src[16k+1][c]) + ...          over the chunk's rows (the last chunk may be short)
 *   job_total[c]  = ((+0 + chunk_0[c]) + chunk_1[c]) + ...               in row order
 *   dst[c]        = (ADD ? dst_old[c] : +0) + job_total_0[c] + job_total_1[c] + ...      in table order, left to right
 * Exactly one plain store goes to each dst[c] per launch; no atomics.
 * `blocks_device`: one work item per 256-thread workgroup, (index of the chain's first job) << 32 | column block (256 columns).
 * The table lives in device memory, which the host cannot read without a synchronisation, so the call also takes the table's
 * host copy (`jobs_host`, read during the call only) and checks it before anything is launched: null src / dst, rows or cols
 * <= 0, cols > ld, a chain whose members differ in cols or flags, a chain that is split apart in the table (a dst that returns
 * after another chain), n_jobs or n_blocks <= 0. */
int mh_reduce_ordered(const MhOrderedJob* jobs_host, const MhOrderedJob* jobs_device, int n_jobs, const uint64_t* blocks_device,
                      int n_blocks, void* stream);

/* Column sums, first phase (the arithmetic of the column-sum entry point of maestro_hip.h without its final atomic add):
 * x bf16 or f32 [M, ld] (N <= ld, N % 4 == 0, ld % 4 == 0); partial f32 [mh_colsum_partial_rows(M), N] dense, 16-byte aligned,
 * every element written by a plain store.  Row block i sums rows [256 i, 256 i + 256) of x. */
int mh_colsum_partial_rows(int M);
int mh_colsum_partial(const void* x, int x_is_f32, float* partial, int M, int N, int ld, void* stream);

/* Masked reconstruction loss, first phase.  Operands and `drec` (bit for bit) as the masked-loss entry points of maestro_hip.h;
 * instead of adding to the loss word, workgroup i writes its weighted partial loss to loss_partial[i] (zero is written too;
 * block 0 writes NaN for an empty selection, n_masked == 0).  loss_partial has mh_masked_loss_partial_size(B, Lm) elements; the
 * modality's loss is their ordered sum. */
int mh_masked_loss_partial_size(int B, int Lm);
int mh_masked_loss_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                       float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, void* stream);
int mh_masked_loss_bands_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems, float weight,
                             float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, int tgt_C,
                             int tgt_c0, int n_g, void* stream);

/* Mask-token gradient, first phase.  Operands as the mask-token gradient entry points of maestro_hip.h; workgroup i writes the
 * sum of its rows to partial[i, 0 .. Dd) (f32 [mh_unmask_token_grad_partial_rows(n_rows), Dd] dense, 16-byte aligned; rows
 * without a contributing token are written as zeros).  n_rows = B * (t_hi - t_lo), or B * L for the per-sample form. */
int mh_unmask_token_grad_partial_rows(long n_rows);
int mh_unmask_token_grad_det(const float* dxdec, const uint8_t* mask, const int* tok_slot, float* partial, int B, int L, int Dd,
                             int slot, int t_lo, int t_hi, void* stream);
int mh_unmask_token_grad_per_sample_det(const float* dxdec, const uint8_t* mask, const int* tok_slot_bl, float* partial, int B,
                                        int L, int Dd, int slot, void* stream);

/* GroupNorm backward of the patch embedding.  Operands as the embed-finish backward of maestro_hip.h, but pass 1 writes per
 * workgroup: (S1, S2) to blk_sums [B*D, nblk, 2] and dgamma | dbeta to param_partial [B*D * nblk, 2 E] (dense), with
 * nblk = mh_embed_bwd_partial_rows(1, L).  The per-image sums[B*D, 2] that pass 2 reads are finished inside the call by an
 * ordered reduction of blk_sums (the order of mh_reduce_ordered); the parameter rows are left for mh_reduce_ordered
 * (rows = mh_embed_bwd_partial_rows(B*D, L), cols = E, ld = 2 E; dbeta at column offset E). */
int mh_embed_bwd_partial_rows(int BD, int L);
int mh_embed_finish_bwd_det(const float* dxg, const float* y, const float* stats, const float* gamma, void* dyc,
                            float* param_partial, float* blk_sums, float* sums, int B, int D, int L, int E, int tok_off, int Lgroup,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
