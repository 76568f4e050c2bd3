/* C ABI of libmaestro_hip.so, the ends of the pretraining step's backward (pixelify head, enc_to_dec, patch-embed): producers
 * that leave their bias gradient as partial rows, and the patch-embed backward that reads the encoder gradient through the
 * position map ("Step ends").
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, every pointer is DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates no device memory, keeps no global
 * mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 = hipError_t; the message
 * is read with the main header's error call.
 *
 * "Partial rows": workgroup i of the producer stores the column sums of the rows it wrote to cs_partial[i, 0 .. cols) (f32, dense,
 * plain stores, every element of every row written, zeros included; no atomics).  The sums are of the bf16-ROUNDED values the
 * producer stores -- what a column sum over the stored tensor would read.  One job of the batched column sum of maestro_hip.h
 * (rows = the *_cs_rows() value, cols, ld = cols) finishes them.
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them.
 */
#ifndef MAESTRO_HIP_ENDS_H
#define MAESTRO_HIP_ENDS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Masked reconstruction loss.  Operands, the loss word and `drec` (bit for bit) as the masked-loss entry points of maestro_hip.h
 * (`drec` is required here); cs_partial f32 [mh_masked_loss_cs_rows(B, Lm), PPC] receives the partial rows of colsum(drec).
 * PPC % 4 == 0, PPC <= 1024. */
int mh_masked_loss_cs_rows(int B, int Lm);
int mh_masked_loss_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                      float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                      void* stream);
int mh_masked_loss_bands_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems, float weight,
                            float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                            int tgt_C, int tgt_c0, int n_g, void* stream);

/* dst16[b, j, :] = bf16(src[b, idx[b, j], :]) for j < n_idx: the row gather of maestro_hip.h followed by its bf16 cast, in one
 * pass and without the f32 intermediate (src f32 [B, src_L, dim], idx int32 [B, n_idx], dst16 bf16 [B * n_idx, dim] dense);
 * cs_partial f32 [mh_gather_rows_cs_rows(B * n_idx), dim] receives the partial rows of colsum(dst16).  dim % 4 == 0, dim <= 1024. */
int mh_gather_rows_cs_rows(long rows);
int mh_gather_rows_bf16_cs(const float* src, const int* idx, void* dst16, float* cs_partial, int B, int src_L, int n_idx, int dim,
                           void* stream);

/* GroupNorm backward of the patch embedding, as the embed-finish backward of maestro_hip.h (same operands, same atomically
 * accumulated dgamma / dbeta, same arithmetic per element), with two differences:
 *  - the gradient of the group sequence is read through the position map: dx f32 [B, n_vis, E] holds the gradient of the VISIBLE
 *    rows only and inv int32 [B, Lgroup] maps a group position to its visible row (< 0: masked).  Token (b, d, l) of the modality
 *    sits at group position tok_off + d * L + l; a masked position is a zero gradient whose loads are skipped.  inv == NULL:
 *    dx is the dense [B, Lgroup, E] gradient (n_vis is ignored).
 *  - cs_partial f32 [mh_embed_bwd_cs_rows(B * D * L), E] receives the partial rows of colsum(dyc) (the conv bias gradient).
 * E % 4 == 0, E <= 1024. */
int mh_embed_bwd_cs_rows(long rows);
int mh_embed_finish_bwd_ends(const float* dx, const int* inv, int n_vis, const float* y, const float* stats, const float* gamma,
                             void* dyc, float* dgamma, float* dbeta, float* sums, float* cs_partial, int B, int D, int L, int E,
                             int tok_off, int Lgroup, void* stream);

#ifdef __cplusplus
}
#endif
#endif
