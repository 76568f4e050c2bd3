// C declarations of the nearest-neighbour entry points (knn.hip): row normalisation of exported encoder features, the top-k
// cosine neighbours of bf16 queries in a bf16 feature bank, and the weighted vote over their labels.  They follow every convention
// of include/maestro_hip.h -- no allocation, no synchronisation, the launch goes to `stream`, 0 on success, -1 for a refused
// argument and a hipError_t for a failed launch with the text in mh_last_error(), arguments checked before anything is launched,
// no environment reads -- and live here until they are folded into that header and the guard-band ledger of the tests.
//
// What they compute: the reference trains and scores its models through heads only (maestro/layers/head.py:116-130 gives the
// logits, maestro/train/metric.py the scores) and has no label-free evaluation of a pretrained encoder.  The protocol stated
// here is the weighted k-NN classifier of DINO (Caron et al., "Emerging Properties in Self-Supervised Vision Transformers",
// ICCV 2021, section 4.1, after Wu et al., CVPR 2018): features are L2-normalised with the rule of torch.nn.functional.normalize
// (x / max(||x||_2, eps)), the k bank rows of largest cosine similarity vote for their labels with weight exp(sim / T).
//
// The order rule.  Pairs (similarity, global index) are totally ordered: the larger similarity first, then the smaller index; an
// index below zero (an unfilled slot) comes after every real index, and a NaN similarity is no candidate at all.  Every list
// below is the head of its candidate set under this order, so it does not depend on how the work was cut.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_KNN_MAX_K 128

// The bank-split rule of mh_knn_topk: how many ways the bank is cut across workgroups so that few queries still fill the chip.
// A function of its arguments alone (no device query); 1 <= splits <= the number of 128-row bank tiles.  0 for arguments
// mh_knn_topk would refuse.
int mh_knn_splits(int Nq, int Nb, int E, int k);
// Bytes of the workspace of mh_knn_topk for `splits` splits: splits * Nq * k pairs of (f32, i32).  -1 for refused arguments.
long mh_knn_workspace_bytes(int Nq, int k, int splits);

// y[r, c] = x[r, c] / max(||x[r, :]||_2, eps) for `rows` rows of E columns; x f32 with row pitch ldx, y f32 with pitch ldy (may
// be NULL, may be x itself with ldy == ldx), y16 bf16 with pitch ldy16 (may be NULL; not both): the round-to-nearest-even bf16 of
// the fp32 quotient, bit for bit.  The sum of squares: lane l of a 64-lane wave takes s_l = fma(x_c, x_c, s_l) over its columns
// c = l, l + 64, ... in ascending order, the 64 partial sums are folded by the xor butterfly 32, 16, ... 1, all in fp32: an
// order that depends on E alone.  Then one correctly rounded sqrt, max with eps, and one correctly rounded division per element.
// A zero row gives zeros.  4-byte aligned x and y, 2-byte aligned y16, any pitch >= E.  1 <= E <= 65536, eps >= 0.
int mh_l2_normalize(const float* x, long ldx, float eps, float* y, long ldy, uint16_t* y16, long ldy16, long rows, int E,
                    void* stream);

// The k nearest bank rows of every query.  q bf16 [Nq, E] with pitch ldq, bank bf16 [Nb, E] with pitch ldb; 16-byte aligned
// bases, pitches that are multiples of 8 and at most 2^20, E % 32 == 0, 32 <= E <= 1024, 1 <= k <= MH_KNN_MAX_K.
// The similarity of a pair is the fp32 accumulator of v_mfma_f32_16x16x32_bf16 over the E / 32 blocks of 32 columns in ascending
// order, started from zero: exact bf16 products, one order that depends on E alone -- not on the tile, split, chunk or row the
// pair falls in.
// sims f32 [Nq, k], idx i32 [Nq, k] (4-byte aligned, dense): per query the k first pairs (similarity, index_base + bank row)
// under the order rule, sorted by it; unfilled slots hold (-inf, -1).  accumulate = 1: the incoming sims / idx rows are further
// candidates (entries with idx < 0 or a NaN are none), so that a bank streamed in chunks gives the bits of one call;
// accumulate = 0: they are not read.  Nb = 0 (bank may then be NULL) is accepted with accumulate = 1 only.  index_base >= 0,
// index_base + Nb <= 2^31 - 1.
// `splits` >= 1 cuts the bank's 128-row tiles evenly over that many workgroups per 64-query tile (mh_knn_splits gives the rule's
// value; any value gives the same bits); the partial lists go to `ws` (16-byte aligned, at least
// mh_knn_workspace_bytes(Nq, k, splits) bytes) and a second launch on the same stream merges them.  No [Nq, Nb] buffer exists.
int mh_knn_topk(const uint16_t* q, long ldq, const uint16_t* bank, long ldb, long index_base, float* sims, int* idx, int accumulate,
                void* ws, long ws_bytes, int splits, int Nq, int Nb, int E, int k, void* stream);

// The weighted vote over the first k_eval <= k entries of every sorted list (sims, idx: [Nq, k] as mh_knn_topk leaves them).
//   w_j = sims[j] == sims[0] ? 1 : exp((sims[j] - sims[0]) * inv_T)      (fp32: one subtraction, one product, expf)
//   scores[n, c] = sum over j in ascending order of w_j [labels[idx_j] == c], each sum one fp32 addition, from 0
// An entry with idx < 0, idx >= n_labels, a label equal to missing_val or a label outside [0, C) adds nothing.  labels i32
// [n_labels].  scores f32 [Nq, lds >= C] (pad columns untouched), cls i32 [Nq]: the lowest class among equal maxima of the
// scores just written (the arg-max rule of mh_confusion_ce), -1 when no entry voted.  Either may be NULL, not both.
// 2 <= C <= 1024, inv_T > 0 and finite, 1 <= k_eval <= k <= MH_KNN_MAX_K.
int mh_knn_vote(const float* sims, const int* idx, const int* labels, long n_labels, int missing_val, float inv_T, int k, int k_eval,
                float* scores, long lds, int* cls, int Nq, int C, void* stream);

#ifdef __cplusplus
}
#endif
