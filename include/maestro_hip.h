/* C ABI of libmaestro_hip.so -- the MI355X (gfx950) kernels of MAESTRO's MAE pretraining hot path.
 *
 * The reference (IGNF/MAESTRO) is pure Python with no FFI of its own; the boundary it would bind
 * is therefore one entry point per fused stage of the per-step path.  Each declaration cites the reference
 * lines whose ATen/einops op sequence it replaces (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory owned by the caller unless noted (or its name
 *     ends in _host);
 *   - asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, keeps no
 *     global mutable state, re-entrant across streams/threads; graph-capturable;
 *   - returns 0 on success, <0 for a bad argument (nothing is launched), >0 = hipError_t; mh_last_error() gives a thread-local
 *     message;
 *   - bf16 = raw uint16 bits; "f32" = float; row-major with explicit leading dimensions (in elements).
 *
 * Two terms that several sections use:
 *
 * Deterministic forms (mh_reduce_ordered, mh_colsum_partial, the *_det entry points; DESIGN.md, "Deterministic mode"): an
 * ordered fp32 reduction and the atomic-free first phases of the reductions of the pretraining step.  None of them issues a
 * floating-point atomic: every output element is written by exactly one plain store per launch, so the bits of a result depend on
 * the operands alone and not on the order in which the hardware runs the workgroups.
 *
 * "Partial rows" (the *_cs / *_ends entry points: the ends of the pretraining step's backward -- pixelify head, enc_to_dec,
 * patch-embed; DESIGN.md section 4, "Step ends"): workgroup i of the producer stores the column sums of the rows it wrote to
 * cs_partial[i, 0 .. cols) (f32, dense, plain stores, every element of every row written, zeros included; no atomics).  The sums
 * are of the bf16-ROUNDED values the producer stores -- what a column sum over the stored tensor would read.  One job of
 * mh_colsum_batched (rows = the *_cs_rows() value, cols, ld = cols) finishes them.
 */
#ifndef MAESTRO_HIP_H
#define MAESTRO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* mh_last_error(void);
int mh_version(void);

/* ---------------------------------------------------------------------------------------------- GEMM (MFMA)
 * C[M,N] = op(A) * op(B) (+ epilogue), bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16.
 *   layout 0 "NT": A[M,K] (lda), B[N,K] (ldb)      -- forward of nn.Linear / 1x1 conv / patch-embed conv
 *   layout 1 "NN": A[M,K] (lda), B[K,N] (ldb)      -- dgrad:  dX = dY * W
 *   layout 2 "TN": A[K,M] (lda), B[K,N] (ldb)      -- wgrad:  dW = dY^T * X   (K = tokens)
 * Replaces: vit_pytorch Attention.to_qkv / to_out / FeedForward Linear (call sites maestro/ssl/mae.py:135-174),
 * enc_to_dec Linear (mae.py:145-154), Patchify conv (maestro/layers/embed.py:48-60), Pixelify 1x1 conv
 * (embed.py:139-151) and their autograd transposes.
 * flags: bit0 out_f32 (else bf16) | bit1 +bias[N] | bit2 GELU(erf) (aux_out, if given, receives the bf16
 *        pre-activation) | bit3 += res[M,N] f32 (ldr) | bit4 *= gelu'(aux_in[M,N] bf16) | bit5 atomic accumulate
 *        into C (f32 only; split-K is applied automatically for layout 2).
 * Requirements: K % 8 == 0 (layouts 0/1), lda/ldb % 8 == 0, N % 4 == 0 and ldc % 4 == 0 (f32 out) or % 8 (bf16 out,
 * aux), 16-byte aligned bases; residual needs f32 output, GELU/GELU' need bf16 output. */
#define MH_GEMM_OUT_F32 1
#define MH_GEMM_BIAS 2
#define MH_GEMM_GELU 4
#define MH_GEMM_RESIDUAL 8
#define MH_GEMM_DGELU 16
#define MH_GEMM_ATOMIC 32
#define MH_GEMM_COLSUM 64   /* bf16 output only: colsum[(m / 64), n] = sum over the 64-row block of C[m, n] (f32 values before
                             * rounding); colsum is a [ceil(M / 64), N] workspace, plain stores; reduce it with mh_colsum.
                             * Numerics: the summand is the epilogue's fp32 value (accumulator + bias, times the GELU' / MULAUX
                             * factor), NOT its bf16 rounding that C receives; the 64 terms are added in fp32 (a lane's rows in
                             * order, then a three-step butterfly), so |colsum - exact| <= 64 2^-23 sum |terms| + the terms' own
                             * errors (tests/test_numerics_gpu.py).  Rows at or beyond M contribute nothing. */
#define MH_GEMM_AUX_DGELU 128 /* with MH_GEMM_GELU: aux_out receives GELU'(pre-activation) (bf16) instead of the pre-activation: the
                               * CDF / PDF are already at hand in the forward epilogue, so the backward only multiplies */
#define MH_GEMM_MULAUX 256    /* bf16 output only: C *= aux_in[M, N] (bf16) -- the backward of GELU with the saved derivative */
#define MH_GEMM_AUX_U8 1024   /* the saved GELU derivative (aux_out of MH_GEMM_AUX_DGELU, aux_in of MH_GEMM_MULAUX) is stored as one
                               * BYTE per element, code = round((GELU' + 0.13) * 200): GELU' lies in [-0.129, 1.129], the step of
                               * 0.005 is about what bf16 resolves near 1; halves the derivative's HBM bytes (ldaux in bytes) */
#define MH_GEMM_C8_E5M2 512   /* mh_gemm_fp8 only: the fp8 copy c8 of the output is e5m2 (a gradient: the next dgrad's A operand) */
/* mh_gemm_fp8 only, at most one of them: force a tile / ring form instead of the library's size rule (experiments, tests).
 * The library never reads the environment: every such choice is an argument (maestro_amd/hip.py maps MH_FP8_TILE onto these). */
#define MH_GEMM_FP8_TILE_256 2048    /* 256 x 256, 8 waves */
#define MH_GEMM_FP8_TILE_128 4096    /* 128 x 128, two-stage ring, two workgroups per CU */
#define MH_GEMM_FP8_TILE_128D 8192   /* 128 x 128, four-stage ring */
int mh_gemm_bf16(int layout, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                 int flags, const float* bias, const float* res, int ldr, const void* aux_in, void* aux_out,
                 int ldaux, float* colsum, void* stream);

/* Same contract with an explicit kernel / tile choice (what mh_gemm_bf16 picks by itself with MH_TILE_AUTO):
 *   MH_TILE_REG_128      128x128x64 tile, register-staged double-buffered LDS (gemm.hip): every shape / tail
 *   MH_TILE_DMA_256      256x256x32 tile, 8 waves, 4-stage LDS-DMA ring (gemm_dma.hip)
 *   MH_TILE_DMA_256x128 / MH_TILE_DMA_128x256   4 waves, 3-stage ring;   MH_TILE_DMA_128   128x128, 2 waves, 4-stage ring
 *   MH_TILE_DMA_128x4    128x128, four 64x64 waves, 4-stage ring (the register-staged kernel's geometry, DMA-fed)
 *   MH_TILE_DMA_256_LOCKSTEP   MH_TILE_DMA_256 without the wave-group stagger (A/B experiments; bit-identical results)
 *   MH_TILE_PP_128       persistent workgroups over 128x128x64 tiles with a second accumulator set: the epilogue of tile t runs
 *                        inside the main loop of tile t + 1 (gemm_pp.hip); NT / NN, K %% 64 == 0, K >= 512, N %% 128 == 0, and
 *                        flags one of: 0 | BIAS+GELU+AUX_DGELU+AUX_U8 | MULAUX+AUX_U8+COLSUM | OUT_F32+BIAS+RESIDUAL
 * The DMA tiles return -2 (nothing launched, error string untouched) when the problem does not qualify (K %% 32 != 0 with
 * a K-minor operand, operands beyond the 2 GiB buffer-descriptor range): pick another tile.  The host side times the
 * eligible tiles once per distinct (layout, M, N, K, flags) and remembers the fastest (maestro_amd/hip.py). */
enum { MH_TILE_AUTO = -1, MH_TILE_REG_128 = 0, MH_TILE_DMA_256 = 1, MH_TILE_DMA_256x128 = 2, MH_TILE_DMA_128x256 = 3,
       MH_TILE_DMA_128 = 4, MH_TILE_DMA_128x4 = 5, MH_TILE_DMA_256_LOCKSTEP = 6, MH_TILE_PP_128 = 7,
       /* retired ids, reserved: they named diagnostic builds of MH_TILE_PP_128 whose outputs were NOT the GEMM's (main loop only /
        * epilogue arithmetic without its stores / stores without the GELU arithmetic / other instruction placements: the ablation
        * under profiles/r03_gemm_pp_diag.txt).  No library contains those kernels: every library returns -2 for these ids (nothing
        * launched, output untouched), so no caller of the C ABI can get a wrong-output kernel by passing a tile id. */
       MH_TILE_PP_128_DIAG1 = 8, MH_TILE_PP_128_DIAG2 = 9, MH_TILE_PP_128_DIAG3 = 10,
       MH_TILE_PP_128_DIAG4 = 11, MH_TILE_PP_128_DIAG5 = 12,
       /* MH_TILE_REG_128's kernel with 64 x 128 tiles (three workgroups per CU) / 192 x 128 tiles: for outputs whose 128 x 128
        * tiling fills the chip's workgroup slots badly (N = 512 / 768).  NT / NN without MH_GEMM_COLSUM; otherwise = REG_128. */
       MH_TILE_REG_64 = 13, MH_TILE_REG_192 = 14,
       /* stream-K tiles (gemm_sk.hip; mh_gemm_bf16_sk only -- they need a workspace): 192 x 128 / 256 x 128, one workgroup per CU */
       MH_TILE_SK_192 = 15, MH_TILE_SK_256 = 16,
       MH_TILE_SK_DMA_256 = 17 /* 256 x 256 x 32, eight waves, the LDS-DMA ring of MH_TILE_DMA_256 run by persistent workgroups */ };
int mh_gemm_bf16_tile(int tile, int layout, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                      int ldc, int flags, const float* bias, const float* res, int ldr, const void* aux_in, void* aux_out,
                      int ldaux, float* colsum, void* stream);

/* Which tile mh_gemm_bf16_tile(tile, ...) runs for a problem: the library's one dispatch rule as a query.  Like the size queries
 * it takes no device buffer and no stream and launches nothing; it reads shapes, strides and flags only.  Returns
 *   >= 0  the concrete MH_TILE_* that runs: for MH_TILE_AUTO the rule's choice (REG_128, REG_192, PP_128 or DMA_256); an explicit
 *         tile stands for itself, except MH_TILE_REG_64 / _192 on a TN or MH_GEMM_COLSUM problem, which run as MH_TILE_REG_128;
 *   -2    the explicit DMA / ping-pong tile does not serve the problem (mh_gemm_bf16_tile answers -2 too; error string untouched);
 *   -1    invalid layout / flags / strides / tile (the stream-K ids included: they belong to mh_gemm_bf16_sk), by the same checks
 *         as the GEMM call minus those on its pointers; see mh_last_error.
 * `families`: the kernel families MH_TILE_AUTO may choose besides the 128 x 128 register tile.  MH_GEMM_FAMILY_ALL is the rule
 * mh_gemm_bf16 applies; a subset states an A/B rule without copying it (MH_GEMM_FAMILY_DMA alone: the rule before the ping-pong
 * and 192-row tiles existed).  A family that is left out is never chosen; explicit tiles ignore the mask. */
#define MH_GEMM_FAMILY_DMA 1
#define MH_GEMM_FAMILY_PP 2
#define MH_GEMM_FAMILY_192 4
#define MH_GEMM_FAMILY_ALL 7
int mh_gemm_bf16_resolve_tile(int tile, int families, int layout, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                              int ldaux, int flags);

/* Stream-K GEMM (gemm_sk.hip): C[M, N] = A[M, K] B^T (layout 0, B [N, K]) or A B (layout 1, B [K, N]) with the long-K, narrow-N
 * problems of the transformer blocks in mind (fc2, out-proj, fc1 / qkv / out-proj dgrads: the nn.Linear call sites of
 * vit_pytorch's Attention / FeedForward built at maestro/ssl/mae.py:135-174).  `grid` persistent four-wave workgroups (one per
 * CU: pass the CU count of the device, or of the stream's CU mask) split tiles x (K / 64) units evenly; a tile shared by
 * several workgroups is summed in workgroup order by the one that owns its last K step (deterministic, no atomics on C).
 *   tile   MH_TILE_SK_DMA_256 (256 x 256 x 32, eight waves, LDS-DMA ring: gemm_sk_dma.hip; K %% 32 == 0, K >= 128, N %% 256 == 0) or the
 *          four-wave register-staged MH_TILE_SK_192 (192 x 128 x 64) / MH_TILE_SK_256 (256 x 128 x 64) (K %% 64 == 0, N %% 128 == 0)
 *   flags  0 (bf16 C) or MH_GEMM_OUT_F32 | MH_GEMM_BIAS | MH_GEMM_RESIDUAL (fp32 C = A B + bias + res); anything the tile does not
 *          serve returns -2 (nothing launched, error string untouched): use mh_gemm_bf16
 *   workspace  mh_gemm_sk_workspace(tile, grid) bytes, 16-byte aligned, owned by the caller, ZEROED ONCE before its first use (the
 *          kernel leaves its flag words zero); launches that may run concurrently (different streams) need different workspaces.
 * Same fp32 sums per output element as mh_gemm_bf16 when no tile is shared; a shared tile adds its K ranges in ascending order. */
long mh_gemm_sk_workspace(int tile, int grid);
int mh_gemm_bf16_sk(int tile, int layout, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                    int flags, const float* bias, const float* res, int ldr, void* workspace, long workspace_bytes, int grid,
                    void* stream);

/* Grouped weight-gradient GEMM: ONE launch over the 256x256 tiles of many independent "TN" problems
 * dW_i[M_i, N_i] (f32) = A_i^T B_i with A_i [K_i, M_i] bf16 (= dY_i), B_i [K_i, N_i] bf16 (= X_i), K_i = tokens.
 * Used to issue all wgrads of a backward segment at once (no split-K, whole-chip tile occupancy).  `table` is a DEVICE
 * array of problems; M, N, lda, ldb %% 8 == 0.  accumulate = 0: plain stores (the entry is the only writer of C); 1: fp32
 * atomic adds into a zeroed C (several entries share one C, e.g. one encoder applied to several groups).
 * `tile_queues` is a DEVICE array [8][queue_len] of tile ids (problem << 16 | tile_m << 8 | tile_n, 0xFFFFFFFF = empty
 * slot), one queue per XCD: workgroup b runs entry [b %% 8][b / 8] (the hardware places workgroup b on XCD b %% 8), so the
 * host decides which tiles share an L2: keep the tiles of one problem in one queue (its dY / X panels are then fetched
 * once per XCD instead of once per tile) and balance sum(K) over the queues. */
typedef struct MhGroupedGemm {
    const void* A; const void* B; void* C;
    int M, N, K, lda, ldb, ldc, reserved, accumulate;
} MhGroupedGemm;
int mh_gemm_grouped_tn(const MhGroupedGemm* table_device, int n_problems, const uint32_t* tile_queues, int queue_len,
                       void* stream);

/* fp8 GEMM (BASELINE configs[4], "ViT-Base MAE fp8 MFMA path"): C[M, N] = (*descale_a) (*descale_b) A8[M, K] B8[N, K]^T
 * with the epilogues of mh_gemm_bf16 (flags, bias, res, aux_in / aux_out, colsum: same meaning; no MH_GEMM_ATOMIC).  Both
 * operands are K-minor bytes: B8 = a weight [N, K] in OCP e4m3 (the forward uses the weight as stored, the dgrad its
 * transposed fp8 shadow), A8 = activations in e4m3 or gradients in e5m2 (a_format).  K %% 128 == 0, lda / ldb %% 16 == 0 (bytes).
 * descale_a / descale_b: DEVICE scalars 1 / scale of the per-tensor quantisers below (mh_quant_batched).  Optional c8
 * (bf16-output epilogues only): an e4m3 copy of the output times *c8_scale (the next fp8 GEMM's A operand: fc1 -> fc2),
 * with max |output| folded into the amax row c8_amax (delayed scaling; see MH_FP8_AMAX_PITCH).  Replaces the nn.Linear calls inside vit_pytorch's Attention /
 * FeedForward (call sites maestro/ssl/mae.py:135-174) when the step runs with fp8 operands. */
enum { MH_FP8_E4M3 = 0, MH_FP8_E5M2 = 1 };
int mh_gemm_fp8(int M, int N, int K, const void* A8, int lda, int a_format, const void* B8, int ldb, void* C, int ldc,
                int flags, const float* descale_a, const float* descale_b, const float* bias, const float* res, int ldr,
                const void* aux_in, void* aux_out, int ldaux, float* colsum, void* c8, int ldc8, const float* c8_scale,
                float* c8_amax, void* stream);
/* Per-tensor fp8 quantisation, batched over a job table (DEVICE array): job = one tensor of n elements (n %% 4 == 0), f32 or
 * bf16 source, `slot` = its entry in the scale / amax tables.  items: DEVICE array of work items job << 32 | chunk (chunks of
 * 4096 elements).  mode 0: amax row of slot = max(itself, max |src|) only;  1: dst = fp8(src * scale[slot]) (+ the transposed
 * copy dst_t [cols, rows] of a [rows, cols] tensor when dst_t != NULL, cols %% 4 == 0);  2: cast AND fold max |src| into amax
 * (delayed scaling of activations: this step casts with the previous step's scale).  Values saturate at the format's largest
 * finite number.  mh_fp8_update_scales: scale = 2^(floor(log2(format_max / amax)) - margin_log2) (1 while amax is 0),
 * descale = 1 / scale, amax reset to 0 -- all on the device, capturable.  The floor is the exact one, the largest e with
 * amax 2^e <= format_max, for every finite amax > 0 -- held bit for bit where a float32 evaluation could slip: amax =
 * format_max 2^-k and its fp32 neighbours, fp32 subnormals, the largest fp32 numbers; the exponent after the margin is clamped
 * to [-100, 100]; an inf / NaN amax gives a NaN scale and descale.
 * The cast at EVERY site of this header that writes fp8 bytes (the quantisers, the LayerNorm and GEMM output copies, the AdamW
 * shadow): code = fp8(clamp(x * scale, -max, max)) with the product rounded once to fp32 (subnormal products are kept, not
 * flushed), then round to nearest even; a result that rounds to zero keeps the sign of x; x is the fp32 value the site
 * computed, never its bf16 rounding (the MX copies, which quantise the bf16 output by definition, excepted); the absmax is
 * taken on |x| before the scale (tests/test_fp8_codes_gpu.py holds all of it bit for bit).
 * amax tables: ONE ROW of MH_FP8_AMAX_PITCH floats per slot, not one float -- same-cache-line atomics retire at about one per
 * 10 ns on MI355X (scripts/micro_amax.hip: 18432 LayerNorm rows folding into one word took 217 us instead of 19), so every
 * workgroup folds into sub-slot (its index %% MH_FP8_AMAX_SUBSLOTS) of the row, MH_FP8_AMAX_STRIDE floats (256 bytes) apart; a
 * slot's absmax is the maximum over its row, taken by mh_fp8_update_scales.  Every `amax` pointer of this header (c8_amax,
 * y8_amax, the tables of mh_quant_batched / mh_adamw_fp8) points at such rows. */
#define MH_FP8_AMAX_SUBSLOTS 32
#define MH_FP8_AMAX_STRIDE 64
#define MH_FP8_AMAX_PITCH (MH_FP8_AMAX_SUBSLOTS * MH_FP8_AMAX_STRIDE)
typedef struct MhQuantJob {
    const void* src; void* dst; void* dst_t;
    long n;
    int rows, cols, slot, is_f32, format, reserved;
} MhQuantJob;
int mh_quant_batched(const MhQuantJob* jobs_device, const unsigned long* items_device, int n_items, const float* scale,
                     float* amax, int mode, void* stream);
int mh_fp8_update_scales(float* amax, float* scale, float* descale, int n, float format_max, int margin_log2, void* stream);
/* ---------------------------------------------------------------------------------------------- MX block scaling
 * The second fp8 scaling mode (maestro_amd/fp8.py, `mx`): OCP MX (MXFP8, e4m3 elements) with one E8M0 scale byte per BLOCK of
 * 32 consecutive elements along the GEMM's K dimension (a row of the K-minor byte tensor).  The rule, for every producer below:
 *   scale  e = the smallest integer with amax <= 448 * 2^e (amax = the block's max |value|); stored byte = clamp(127 + e, 0, 254).
 *          An all-zero block gets 127.  A block that holds a NaN or an inf gets 0xFF (E8M0 NaN): every product of the block
 *          is NaN, so the poison reaches the GEMM output -- the MX form of the per-tensor rule (a non-finite amax poisons the
 *          tensor's scale and descale, mh_fp8_update_scales).  Rounding the scale UP means no element ever saturates: the OCP
 *          spec's floor(log2 amax) - 8 puts amax in [256, 512) and clips the top of that binade to 448 (up to 1.75x of the
 *          largest values lost); ceil(log2(amax / 448)) keeps amax in (224, 448], at the cost of at most one binade of e4m3's
 *          17 for the block's smallest values.
 *   elements  e4m3fn(v * 2^-e), round to nearest even (the conversion of the per-tensor quantisers).
 *   source    every MX copy is the MX quantisation of a BF16 tensor (the bf16 operand the bf16 path would use): the producers
 *          that fuse the cast (the LayerNorm, the GEMM's c8 copy) quantise their own bf16-ROUNDED output, so each is bit-equal
 *          to mh_quant_mx_batched applied to that bf16 output.
 *   layout    scales are a row-major byte matrix [rows, K/32] with leading dimension ld (ld %% 4 == 0: one K step of 128 of a row
 *          is one aligned u32).  Weights: one flat byte buffer, a weight [N, K] at parameter offset o has its scales as a
 *          [N, K/32] view at byte o / 32 rounded up to a multiple of 4 (parameters are only 64-element aligned). */
/* C[M, N] = sum_k (A8[m, k] 2^ea(m, k/32)) (B8[n, k] 2^eb(n, k/32)) with the epilogues of mh_gemm_fp8 (same flags, tiles, size
 * rule and MH_GEMM_FP8_TILE_* hints): A8 [M, K] and B8 [N, K] OCP e4m3 bytes (K %% 128 == 0, lda / ldb %% 16 == 0, 16-B bases),
 * sa [M, K/32] / sb [N, K/32] their E8M0 scales (ldsa / ldsb %% 4 == 0, >= K/32, 4-B bases).  No descale factors.  Optional c8
 * (bf16-output epilogues, N %% 32 == 0): the MX copy of the bf16 output C, c8_scales [M, N/32] (ldc8s %% 4 == 0, >= N/32) --
 * the next GEMM's A operand (fc1 -> fc2).  No e5m2 operands. */
int mh_gemm_mx(int M, int N, int K, const void* A8, int lda, const void* sa, int ldsa, const void* B8, int ldb, const void* sb,
               int ldsb, void* C, int ldc, int flags, const float* bias, const float* res, int ldr, const void* aux_in,
               void* aux_out, int ldaux, float* colsum, void* c8, int ldc8, void* c8_scales, int ldc8s, void* stream);
/* MX quantisation, batched (all weight shadows of a step in ONE launch): job = a bf16 source [rows, cols] (row pitch ld_src
 * elements, %% 4, 8-B base) -> dst e4m3 [rows, cols] (pitch ld_dst bytes, %% 4) + scales [rows, cols/32] (pitch ld_s);
 * cols %% 32 == 0.  jobs_host: a host copy of the n_jobs jobs, checked before the launch (the kernel reads jobs_device);
 * items: DEVICE array of job << 32 | chunk (chunks of 128 blocks = 4096 elements, row-major over the job's blocks). */
typedef struct MhQuantMxJob {
    const void* src; void* dst; void* scales;
    int rows, cols, ld_src, ld_dst, ld_s, reserved;
} MhQuantMxJob;
int mh_quant_mx_batched(const MhQuantMxJob* jobs_host, int n_jobs, const MhQuantMxJob* jobs_device, const unsigned long* items_device,
                        int n_items, void* stream);
/* Byte transposes, batched: dst [cols, rows] = src [rows, cols]^T for every job (rows, cols %% 64 == 0, 16-byte aligned) -- the
 * fp8 dgrad C = dY W needs W^T K-minor ([in, out] for an nn.Linear weight [out, in]): the e4m3 weight shadows are transposed
 * once per optimizer step.  items: DEVICE array of job << 32 | tile (64 x 64-byte tiles, row-major over the source). */
typedef struct MhTransposeJob { const void* src; void* dst; int rows, cols; } MhTransposeJob;
int mh_transpose_u8_batched(const MhTransposeJob* jobs_device, const unsigned long* items_device, int n_items, void* stream);

/* ---------------------------------------------------------------------------------------------- LayerNorm
 * y = (x - mean) * rstd * gamma + beta over the last dim; x f32 (residual stream), y bf16 (GEMM operand) or f32.
 * Rows are addressed as row(b, j) = b * L + off + j (j < n) on both sides, so the split / concat of group sequences
 * around the joint encoder (maestro/ssl/mim.py:408-423) and the per-modality ungroup (maestro/layers/utils.py:50-100)
 * are addressing, not copies.  Saves mean/rstd (f32 [B*n]).  Replaces nn.LayerNorm inside vit_pytorch
 * Attention.norm, FeedForward.net[0] and Transformer.norm (call sites maestro/ssl/mae.py:135-174).
 * dim % 4 == 0, dim <= 2048. */
int mh_layernorm_fwd(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L,
                     int y_off, int y_is_f32, float* mean, float* rstd, int B, int n, int dim, float eps, void* stream);
/* The same with a second output for the fp8 path: y8 = OCP e4m3 of (y * *y8_scale) in y's row map (the A operand of the next
 * mh_gemm_fp8), max |y| folded into the amax row y8_amax (optional; delayed scaling).  y is bf16 (the backward's wgrad reads it). */
int mh_layernorm_fwd_fp8(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L,
                         int y_off, float* mean, float* rstd, int B, int n, int dim, float eps, void* y8,
                         const float* y8_scale, float* y8_amax, void* stream);
/* The same with the MX copy (see "MX block scaling"): y8 = e4m3 of the BF16 output y in y's row map, y8_scales [rows, dim/32]
 * in that row map too (row(b, j) * ld_y8s, ld_y8s %% 4 == 0, >= dim/32).  dim %% 32 == 0; y bit-identical to
 * mh_layernorm_fwd's. */
int mh_layernorm_fwd_mx(const float* x, int x_L, int x_off, const float* gamma, const float* beta, void* y, int y_L, int y_off,
                        float* mean, float* rstd, int B, int n, int dim, float eps, void* y8, void* y8_scales, int ld_y8s,
                        void* stream);
/* dx (f32, x's row map) = (dres ? dres : 0) + LN-backward(dy); optional bf16 copy dx_bf16 (operand of the next
 * dgrad/wgrad GEMM).  dgamma/dbeta f32 [dim] are accumulated (+=) through `workspace` (f32,
 * mh_layernorm_bwd_workspace(B*n, dim) floats; per-block partial rows, then a short atomic reduce); dcol f32 [dim]
 * (optional) += column sums of dx = the bias gradient of the Linear whose output fed this residual.  Pass
 * dgamma = dbeta = NULL to skip all three.  dy is bf16 (dy_is_f32 = 0) or f32, addressed with its own row map. */
int mh_layernorm_bwd(const void* dy, int dy_L, int dy_off, int dy_is_f32, const float* x, int x_L, int x_off,
                     const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                     void* dx_bf16, float* dgamma, float* dbeta, float* dcol, float* workspace, int B, int n, int dim,
                     void* stream);
long mh_layernorm_bwd_workspace(int rows, int dim);
/* The same backward with the parameter-gradient reduce left to the caller: only writes the per-block partial rows
 * [mh_layernorm_bwd_workspace / (3 dim)][3 dim] = (dgamma | dbeta | colsum(dx)) into `workspace`; a later
 * mh_colsum_batched over many such workspaces replaces one small reduce launch per LayerNorm. */
int mh_layernorm_bwd_partial(const void* dy, int dy_L, int dy_off, int dy_is_f32, const float* x, int x_L, int x_off,
                             const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                             void* dx_bf16, float* workspace, int B, int n, int dim, void* stream);
/* Batched column sums: for every job, dst[c] += sum over r < rows of src[r * ld + c] (c < cols), all jobs in ONE launch
 * (fp32 atomics: dst must hold the value to add to).  jobs and blocks are device arrays; blocks lists the work items of
 * the launch, one per workgroup: job << 48 | column block (256 columns) << 32 | row chunk (MH_COLSUM_ROWS rows), so that
 * jobs of very different shapes share a dense grid. */
#define MH_COLSUM_ROWS 16
typedef struct {
    const float* src;
    float* dst;
    int rows, cols, ld, reserved;
} MhColsumJob;
int mh_colsum_batched(const MhColsumJob* jobs_device, int n_jobs, const uint64_t* blocks_device, int n_blocks, void* stream);
/* The deterministic form: ordered column sums.  One job: src f32 [rows, ld] (cols <= ld), dst f32 [cols].  Jobs that share a
 * `dst` are ADJACENT in the table and form a chain (same cols and flags throughout).
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
#define MH_ORDERED_ROWS 16        /* rows per chunk of the ordered reduction */
#define MH_ORDERED_ADD 1          /* MhOrderedJob.flags bit 0: add to the value dst holds (default: overwrite) */
typedef struct MhOrderedJob {
    const float* src;
    float* dst;
    int rows, cols, ld, flags;
} MhOrderedJob;
int mh_reduce_ordered(const MhOrderedJob* jobs_host, const MhOrderedJob* jobs_device, int n_jobs, const uint64_t* blocks_device,
                      int n_blocks, void* stream);

/* ---------------------------------------------------------------------------------------------- attention
 * Fused softmax(Q K^T * scale) V, no mask, no dropout (vit_pytorch Attention.forward; call sites mae.py:135-174).
 * qkv: bf16 [B, N, 3, H, D] (= to_qkv output, chunk(3) then 'b n (h d) -> b h n d'); out: bf16 [B, N, H*D];
 * lse: f32 [B, H, N] (natural-log sum-exp of the scaled scores, saved for the backward).  D in {32, 64}. */
int mh_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int D, float scale, void* stream);
/* dqkv bf16 [B,N,3,H,D] from dout bf16 [B,N,H*D]; delta: f32 workspace [B,H,N].  Two kernels: dQ with the query on the MFMA lane
 * (it also computes delta = rowsum(dO * O)), then dK / dV with the key on the lane; S and P are recomputed in both from lse.  The
 * operand that sits in registers (Q resp. K) is multiplied by scale x log2(e) and rounded to bf16 once more, so the recomputed
 * probabilities differ from the forward's by one extra bf16 rounding of that operand (within the kernels' 1.5e-2 parity bound). */
int mh_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                int B, int N, int H, int D, float scale, void* stream);
/* ---------------------------------------------------------------------------------------------- patch embed
 * Patch extraction of one modality (maestro/layers/embed.py:57-60 'b d c (h p1) (w p2)' + the loss target of
 * maestro/train/model.py:211-229): img f32 [BD, Ctot, S, S] ->
 *   cols   bf16 [BD*g*g, Kpad]  im2col rows in (c, p1, p2) order (= Conv2d weight flattening), zero padded;
 *   target f32  [BD*g*g, P*P*Ctot] columns (p1*P+p2)*Ctot + c (optional): patch-group-wise normalised per
 *          norm_bands group (device int array; unbiased variance, eps 1e-6) when normalise != 0, else raw pixels.
 * rescale_elev (maestro/ssl/mim.py:433-436): channels >= 1 become 30*(ch0 - ch) on the fly. */
int mh_patchify(const float* img, void* cols, float* target, int BD, int Ctot, int S, int P, int Kpad,
                const int* norm_bands, int n_norm_groups, int normalise, int rescale_elev, void* stream);
/* The same for ONE band-group of a modality with several (Patchify splits the channel axis by group sizes and gives every
 * group its own PatchifyBands conv, maestro/layers/embed.py:18-34): img f32 [BD, Csrc, S, S], the patch takes channels
 * c0 .. c0 + Ctot - 1; rescale_elev refers to channel 0 of the image.  cols or target may be NULL (the loss target of such a
 * modality is built once over ALL its channels -- the norm_bands groups of maestro/train/model.py:219-229 ignore the band-
 * groups -- with cols == NULL, c0 = 0, Ctot = Csrc). */
int mh_patchify_bands(const float* img, void* cols, float* target, int BD, int Csrc, int c0, int Ctot, int S, int P, int Kpad,
                      const int* norm_bands, int n_norm_groups, int normalise, int rescale_elev, void* stream);

/* GroupNorm(1, E) over the whole (tokens x E) image per (b, d) (embed.py:55,59-61): chunked partials ->
 * stats f32 [BD, 2] = (mean, rstd).  partial: f32 workspace of mh_groupnorm_partial_size() floats.
 * Numerics: every chunk of 8192 values is reduced in two passes (its fp32 sum, then the fp32 sum of (x - chunk mean)^2) and
 * the chunks are merged in fp64, so mean and rstd keep fp32 two-pass accuracy however far the image lies from zero (an image
 * whose mean is 1000 sigma: rstd to ~1e-7 relative; sums of x and x^2 would lose all but two digits there).  A constant image gives
 * variance 0 exactly when its chunk sums are exact in fp32.  tests/test_numerics_gpu.py holds the bounds. */
int mh_groupnorm_stats(const float* y, float* partial, float* stats, int BD, int L, int E, float eps, void* stream);
int mh_groupnorm_partial_size(int BD, int L, int E);
/* normalise + per-channel affine + positional + date encodings (mim.py:232-252, utils.py:103-173), written straight
 * into the group sequence:  xg[b, tok_off + d*L + l, :] = (y - mean)*rstd*gamma + beta + pos[l, :] (+ date[b*D+d, :]
 * on the last 8 channels).  y: f32 [B*D*L, E] conv output incl. bias; pos f32 [L, E]; date f32 [B, date_rows, 8]
 * (row date_off + d belongs to this modality's date d) or NULL. */
int mh_embed_finish(const float* y, const float* stats, const float* gamma, const float* beta, const float* pos,
                    const float* date, int date_rows, int date_off, float* xg, int B, int D, int L, int E, int tok_off,
                    int Lgroup, void* stream);
/* Backward of the above w.r.t. the conv output: dyc bf16 [B*D*L, E] (A operand of the patch-embed wgrad GEMM);
 * dgamma/dbeta atomically accumulated; sums: f32 workspace [B*D, 2].  Sizes positive, E % 4 == 0 (any width; above 1024
 * in column passes), 0 <= tok_off, tok_off + D * L <= Lgroup -- the same checks in the two forms below. */
int mh_embed_finish_bwd(const float* dxg, const float* y, const float* stats, const float* gamma, void* dyc,
                        float* dgamma, float* dbeta, float* sums, int B, int D, int L, int E, int tok_off, int Lgroup,
                        void* stream);
/* GroupNorm backward of the patch embedding, deterministic form.  Operands as mh_embed_finish_bwd, but pass 1 writes per
 * workgroup: (S1, S2) to blk_sums [B*D, nblk, 2] and dgamma | dbeta to param_partial [B*D * nblk, 2 E] (dense), with
 * nblk = mh_embed_bwd_partial_rows(1, L).  The per-image sums[B*D, 2] that pass 2 reads are finished inside the call by an
 * ordered reduction of blk_sums (the order of mh_reduce_ordered); the parameter rows are left for mh_reduce_ordered
 * (rows = mh_embed_bwd_partial_rows(B*D, L), cols = E, ld = 2 E; dbeta at column offset E). */
int mh_embed_bwd_partial_rows(int BD, int L);
int mh_embed_finish_bwd_det(const float* dxg, const float* y, const float* stats, const float* gamma, void* dyc,
                            float* param_partial, float* blk_sums, float* sums, int B, int D, int L, int E, int tok_off, int Lgroup,
                            void* stream);
/* GroupNorm backward of the patch embedding, step-end form: as mh_embed_finish_bwd (same operands, same atomically accumulated dgamma / dbeta, same arithmetic per
 * element), with two differences:
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
/* Date features (maestro/layers/utils.py:128-167): dates int16 [B, D, 3] (year, day-of-year, hour), ref_date int16
 * [B, 1, 3] -> out f32 [B, rows, 8] rows [row_off, row_off + D): fac * [diff x4, sin/cos doy, sin/cos hour]. */
int mh_date_features(const int16_t* dates, const int16_t* ref_date, float* out, int B, int D, int rows, int row_off,
                     float fac, void* stream);
/* Input staging: resize rasters to image_size (maestro/ssl/mim.py:427-432, F.interpolate with align_corners=False).
 * in f32 [planes, Hin, Win] -> out f32 [planes, Hout, Wout]; mode 0 nearest, 1 bilinear, 2 bicubic (PyTorch index maps,
 * cubic convolution with A = -0.75). */
int mh_resize(const float* in, float* out, long planes, int Hin, int Win, int Hout, int Wout, int mode, void* stream);
/* Input staging: per-sample flips / transpose of square rasters (maestro/dataset/dataset.py:224-257: np.flip axis 2, np.flip
 * axis 3, np.swapaxes(2, 3) of the per-sample [D, C, H, W] array, applied in that order).  in/out [B, planes, S, S] of
 * elem_bytes-wide elements (1, 2, 4, 8), out of place; flags[b] bit0 = flip rows, bit1 = flip columns, bit2 = transpose.
 * Pure data movement: bit-exact. */
int mh_dihedral(const void* in, void* out, const uint8_t* flags, int B, long planes, int S, int elem_bytes, void* stream);
/* Input staging: the median-date selection of multi-temporal rasters that the reference does per sample on the CPU in
 * maestro/dataset/dataset.py:188-220 (window cut 188-195, cloud mask 196-200, median and deviation 202-203, random_dates 204-206,
 * mean / nanargmin / gather 208-213, float cast, log and norm_fac 215-220).  No atomics: the same call on the same operands
 * writes the same bytes.
 *
 * One modality of one batch: out[b, j] = the date of window j of sample b that is closest to the window's per-pixel median.
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
/* element type of `raw` */
#define MH_RAW_U8 0
#define MH_RAW_I16 1
#define MH_RAW_U16 2
#define MH_RAW_F32 3
#define MH_SELECT_MAX_WINDOW 64
int mh_select_dates(const void* raw, int raw_code, const unsigned char* mask, int Cm, int mask_floor, const short* dates,
                    const int* t_start, const int* t_win, int w_max, const double* scores, float* out, short* out_dates,
                    int* out_index, int B, int Tmax, int nd, long n_elem, int n_pix, int log_scale, float norm_fac, void* stream);
/* Elevation rescale copy (maestro/ssl/mim.py:433-436): out[:, c>=1] = 30 * (img[:, 0] - img[:, c]); out != img. */
int mh_rescale_elev(const float* img, float* out, int BD, int C, int S, void* stream);
/* Patch layout [BD*g*g, P*P*C] -> image [BD, C, S, S] ('(p1 p2 c) h w -> c (h p1) (w p2)', embed.py:153-160). */
int mh_depatchify(const float* patches, float* img, int BD, int C, int S, int P, void* stream);

/* ---------------------------------------------------------------------------------------------- masking
 * Random-mask token selection with STABLE tie order (maestro/ssl/mae.py:236-259; ties: DESIGN.md): noise f32 [B, L],
 * struct_mask u8 [B, L] or NULL (noise *= 1 - struct), k masked per row.  Outputs: visible_idx int32 [B, L-k]
 * ascending, masked_idx int32 [B, k] ascending, inv int32 [B, L] (position in the visible list or -1),
 * mask u8 [B, L] (1 = masked).  L <= 8192. */
int mh_mask_select(const float* noise, const uint8_t* struct_mask, int* visible_idx, int* masked_idx, int* inv,
                   uint8_t* mask, int B, int L, int k, void* stream);
/* Row gather  dst[b, dst_off + j, :] = src[b, idx[b, j], :]  (f32 rows of `dim`); dst rows live inside a sequence of
 * dst_L rows per sample (x[batch, unmasked_indices], mae.py:261, fused with the joint-encoder concat). */
int mh_gather_rows(const float* src, const int* idx, float* dst, int B, int src_L, int n_idx, int dim, int dst_L,
                   int dst_off, void* stream);
/* dst16[b, j, :] = bf16(src[b, idx[b, j], :]) for j < n_idx: mh_gather_rows followed by its bf16 cast, in one
 * pass and without the f32 intermediate (src f32 [B, src_L, dim], idx int32 [B, n_idx], dst16 bf16 [B * n_idx, dim] dense);
 * cs_partial f32 [mh_gather_rows_cs_rows(B * n_idx), dim] receives the partial rows of colsum(dst16).  dim % 4 == 0, dim <= 1024. */
int mh_gather_rows_cs_rows(long rows);
int mh_gather_rows_bf16_cs(const float* src, const int* idx, void* dst16, float* cs_partial, int B, int src_L, int n_idx, int dim,
                           void* stream);
/* Transpose of mh_gather_rows into a ZEROED dsrc (indices unique per sample -> plain stores). */
int mh_scatter_rows(const float* ddst, const int* idx, float* dsrc, int B, int src_L, int n_idx, int dim, int dst_L,
                    int dst_off, void* stream);
/* The same transpose written as a gather over every destination row: dst[b, t, :] = inv[b, t] >= 0 ? src[b, inv[b, t], :] : 0
 * (inv = mh_mask_select's position map, -1 on masked tokens; src f32 [B, n, dim], dst f32 [B, L, dim]).  Backward of the
 * visible-token gather x[batch, unmasked_indices] (mae.py:261) without a memset of the destination. */
int mh_expand_rows(const float* src, const int* inv, float* dst, int B, int L, int n, int dim, void* stream);
/* Decoder input assembly (mae.py:266-287 + mim.py:254-274):
 *   xdec[b,t,:] = (inv[b,t] < 0 ? mask_token[tok_slot[t]] : y[b, inv[b,t], :]) + pos[t,:] + date[b, date_row[t], :8 tail]
 * y f32 [B, n_vis, Dd]; mask_token f32 [slots, Dd]; pos f32 [L, Dd]; date f32 [B, n_date_rows, 8] or NULL. */
int mh_unmask_assemble(const float* y, const int* inv, const float* mask_token, const int* tok_slot, const float* pos,
                       const float* date, const int* date_row, int n_date_rows, float* xdec, int B, int L, int n_vis,
                       int Dd, void* stream);
/* dmask_token[:] (f32 [Dd], the gradient row of ONE mask token) += sum of dxdec rows of masked tokens t in
 * [t_lo, t_hi) whose tok_slot == slot (atomic). */
int mh_unmask_token_grad(const float* dxdec, const uint8_t* mask, const int* tok_slot, float* dmask_token, int B, int L,
                         int Dd, int slot, int t_lo, int t_hi, void* stream);
/* The same two with a PER-SAMPLE slot map tok_slot_bl int32 [B, L]: masked position t of sample b receives mask token
 * tok_slot_bl[b, t].  Serves the reference's implementation-defined tie order (maestro/ssl/mae.py:274-286:
 * mask_rec.float().argsort(descending=True) orders the masked positions of a sample arbitrarily, so in a group of several
 * modalities a position can receive ANOTHER modality's token); the host builds the map from the same torch call
 * (MAEEngine.tie_order = "torch").  The gradient sums over all masked positions of the group whose map entry == slot. */
int mh_unmask_assemble_per_sample(const float* y, const int* inv, const float* mask_token, const int* tok_slot_bl,
                                  const float* pos, const float* date, const int* date_row, int n_date_rows, float* xdec,
                                  int B, int L, int n_vis, int Dd, void* stream);
int mh_unmask_token_grad_per_sample(const float* dxdec, const uint8_t* mask, const int* tok_slot_bl, float* dmask_token, int B,
                                    int L, int Dd, int slot, void* stream);
/* Mask-token gradient, first phase (the deterministic forms).  Operands as mh_unmask_token_grad / mh_unmask_token_grad_per_sample;
 * workgroup i writes the sum of its rows to partial[i, 0 .. Dd) (f32 [mh_unmask_token_grad_partial_rows(n_rows), Dd] dense,
 * 16-byte aligned; rows without a contributing token are written as zeros).  n_rows = B * (t_hi - t_lo), or B * L for the
 * per-sample form. */
int mh_unmask_token_grad_partial_rows(long n_rows);
int mh_unmask_token_grad_det(const float* dxdec, const uint8_t* mask, const int* tok_slot, float* partial, int B, int L, int Dd,
                             int slot, int t_lo, int t_hi, void* stream);
int mh_unmask_token_grad_per_sample_det(const float* dxdec, const uint8_t* mask, const int* tok_slot_bl, float* partial, int B,
                                        int L, int Dd, int slot, void* stream);
/* out[0] = number of masked tokens of all samples in group positions [t_lo, t_hi) (one modality). */
int mh_count_masked(const uint8_t* mask, int B, int L, int t_lo, int t_hi, int* out, void* stream);
/* out[0] = (accumulate ? out[0] : 0) + mult * that count: the masked ELEMENTS of a modality whose band-groups have different
 * patch sizes in elements (mult = P*P*bands of the group); the denominator of mh_masked_loss_bands. */
int mh_count_masked_elems(const uint8_t* mask, int B, int L, int t_lo, int t_hi, int* out, int mult, int accumulate, void* stream);

/* Device-side mask draws: the structural Bernoulli masks and the per-token noise of the masking step that the reference draws
 * from torch's generator in maestro/ssl/mae.py:178-246 (structural masks with their rejection loop 178-226, the rand(B, L) noise
 * and its argsort 228-246), restated on a counter-based generator so that the draws of a step are a pure function of
 * (seed, step, global sample index).  No atomics.
 *
 * THE DRAW FUNCTION.  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds), key = (seed & 0xffffffff, seed >> 32), counter
 *     c0 = i >> 2,   c1 = global row,   c2 = step,   c3 = kind | stream << 4 | attempt << 16
 * and U(seed, step, stream, kind, row, attempt, i) = (float)(word[i & 3] >> 8) * 2^-24: 24 bits in [0, 1), the value set of
 * torch.rand.  kind: 0 noise (i = token, attempt 0), 1 mod (i = 0), 2 bands (i = band-group), 3 dates (i = date slot),
 * 4 loc (i = token of the modality's grid).  A Bernoulli draw is U < p with p as float32. */
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

/* ---------------------------------------------------------------------------------------------- loss
 * Masked reconstruction loss at patch layout (maestro/train/model.py:195-247) for one modality: rec f32 [B*Lm, PPC]
 * (pixelify GEMM output), target f32 [B*Lm, PPC] (mh_patchify), mask_group u8 [B, Lgroup] (token (b,t) of the modality
 * sits at tok_off + t).  p = 1 (l1*) or 2 (l2*).  With coef = weight / (n_masked[0] * PPC):
 *   acc[0] += coef * sum(e over masked elements)   (weight = w_mod / sum_w  ->  acc accumulates the final loss)
 *   drec (bf16 [B*Lm, PPC], optional) = coef * d e / d rec on masked tokens, 0 elsewhere. */
int mh_masked_loss(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                   float* acc, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, void* stream);
/* One band-group of a modality with several (Pixelify concatenates the groups' reconstructions along the channel axis and
 * the loss is ONE mean over the modality's masked elements, maestro/layers/embed.py:99-127, maestro/train/model.py:241-243):
 * rec f32 [B*Lm, PPC] with PPC = P*P*n_g, columns pixel * n_g + c; target = the MODALITY's rows [B*Lm, P*P*tgt_C], the group
 * reads columns pixel * tgt_C + tgt_c0 + c; coef = weight / n_elems[0] (mh_count_masked_elems over all groups). */
int mh_masked_loss_bands(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems, float weight,
                         float* acc, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, int tgt_C, int tgt_c0,
                         int n_g, void* stream);
/* Masked reconstruction loss, first phase (the deterministic forms).  Operands and `drec` (bit for bit) as mh_masked_loss /
 * mh_masked_loss_bands; instead of adding to the loss word, workgroup i writes its weighted partial loss to loss_partial[i] (zero
 * is written too; block 0 writes NaN for an empty selection, n_masked == 0).  loss_partial has mh_masked_loss_partial_size(B, Lm)
 * elements; the modality's loss is their ordered sum. */
int mh_masked_loss_partial_size(int B, int Lm);
int mh_masked_loss_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                       float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, void* stream);
int mh_masked_loss_bands_det(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems, float weight,
                             float* loss_partial, void* drec, int B, int Lm, int Lgroup, int tok_off, int PPC, int p, int tgt_C,
                             int tgt_c0, int n_g, void* stream);
/* Masked reconstruction loss, step-end forms.  Operands, the loss word and `drec` (bit for bit) as mh_masked_loss /
 * mh_masked_loss_bands (`drec` is required here); cs_partial f32 [mh_masked_loss_cs_rows(B, Lm), PPC] receives the partial rows of
 * colsum(drec).  PPC % 4 == 0, PPC <= 1024. */
int mh_masked_loss_cs_rows(int B, int Lm);
int mh_masked_loss_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_masked, float weight,
                      float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                      void* stream);
int mh_masked_loss_bands_cs(const float* rec, const float* target, const uint8_t* mask_group, const int* n_elems, float weight,
                            float* acc, void* drec, float* cs_partial, int B, int Lm, int Lgroup, int tok_off, int PPC, int p,
                            int tgt_C, int tgt_c0, int n_g, void* stream);

/* ---------------------------------------------------------------------------------------------- probe / finetune heads
 * (maestro/ssl/mim.py:343-394 compute_logits, maestro/layers/head.py, maestro/train/base.py:98-151)
 *
 * Bilinear resize of a channel-last token grid onto the reference grid (mim.py:357-366, F.interpolate bilinear,
 * align_corners=False): rows (b, in_off + d*h*h + y*h + x) of in f32 [B, in_rows, E] -> rows (b, out_off + d*H*H + Y*H + X)
 * of out f32 [B, out_rows, E].  h == H is an exact copy.  The backward is the transposed map written as a gather
 * (deterministic); accumulate = 1 adds to din. */
int mh_token_resize(const float* in, long in_rows, int in_off, float* out, long out_rows, int out_off, int B, int D, int h,
                    int H, int E, void* stream);
int mh_token_resize_bwd(const float* dout, long out_rows, int out_off, float* din, long in_rows, int in_off, int B, int D,
                        int h, int H, int E, int accumulate, void* stream);
/* AttentiveReduce (head.py:28-62) after its LayerNorm + to_kv GEMM: kv bf16 [rows, 2*dim] (k | v); sequence (b, l),
 * b < n_batch, l < Lr, runs over t < T at row (b*T + t)*Lr + l  (PixelifyHead: T = dates, Lr = reference-grid tokens;
 * ClassificationHead: T = all tokens, Lr = 1).  out f32 [n_batch*Lr, dim] = softmax_t(scale * q.k_t) . v per head
 * (heads = 8, dim in {192, 384, 768, 1024}), lse f32 [n_batch*Lr, 8] kept for the backward.
 * Backward: dkv bf16 [rows, 2*dim]; dq_partial f32 [mh_attn_reduce_partial_rows(n_batch*Lr), dim], summed with mh_colsum. */
int mh_attn_reduce_fwd(const void* kv, const float* query, float* out, float* lse, int n_batch, int T, int Lr, int dim,
                       int heads, void* stream);
int mh_attn_reduce_bwd(const void* kv, const float* query, const float* out, const float* lse, const float* dout, void* dkv,
                       float* dq_partial, int n_batch, int T, int Lr, int dim, int heads, void* stream);
long mh_attn_reduce_partial_rows(int n_seq);
/* type_head = "linear": mean over the same token axis (head.py:77-78, 111-112); x f32 [rows, dim] -> out f32 [n_batch*Lr, dim]. */
int mh_mean_reduce_fwd(const float* x, float* out, int n_batch, int T, int Lr, int dim, void* stream);
int mh_mean_reduce_bwd(const float* dout, float* dx, int n_batch, int T, int Lr, int dim, void* stream);
/* ClassificationHead.linear (head.py:83,93), fp32: out[b, c] = bias[c] + x[b, :] . W[c, :]; backward ACCUMULATES dW, db
 * and writes dx (optional). */
int mh_head_linear_fwd(const float* x, const float* W, const float* bias, float* out, int B, int C, int E, void* stream);
int mh_head_linear_bwd(const float* x, const float* W, const float* dout, float* dx, float* dW, float* db, int B, int C, int E,
                       void* stream);
/* loss_pred (base.py:98-151).  count[0] += #targets != missing_val (target_bytes-wide signed integers).
 * mh_ce_loss: target raster [B, S, S] (S = g*P; classification: g = P = 1), logits f32 at PATCH layout [B*g*g, ld >= P*P*C]
 * with columns (p1*P + p2)*C + c (PixelifyBands order, embed.py:153-160); acc[0] += mean over valid pixels of cross entropy,
 * dlogits (bf16 or f32, same layout) = (softmax - onehot) / n_valid, 0 on missing pixels; n_valid = 0 -> loss 0.
 * mh_bce_loss: logits / target f32 [B, C]; rows with any target == missing_val are skipped (base.py:122-123);
 * acc[0] += mean BCE-with-logits, dlogits f32 [B, C]. */
int mh_count_valid(const void* target, int target_bytes, long n, long missing_val, int* count, void* stream);
int mh_ce_loss(const float* logits, const void* target, int target_bytes, long missing_val, const int* n_valid, float* acc,
               void* dlogits, int dlogits_is_f32, int B, int g, int P, int C, int ld, void* stream);
int mh_bce_loss(const float* logits, const float* target, float missing_val, float* acc, float* dlogits, int B, int C,
                void* stream);
/* Prediction metrics: the confusion matrices that maestro/train/metric.py keeps per target and stage (fed on every supervised
 * step from maestro/train/base.py:143-146).  Results are integers: exact, and independent of the launch order (no float
 * atomics; 32-bit LDS counters per workgroup, 64-bit integer atomics into `cm`).
 *
 * Mono-label confusion matrix (maestro/train/metric.py:63-77 "multiclass": argmax over the classes, then
 * torchmetrics.functional.confusion_matrix; the selection of valid entries is maestro/train/base.py:120-138).
 * Operands as mh_ce_loss (csrc/heads.hip): `logits` f32 at patch layout
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
 * 2x2 of "change_detect", metric.py:68-77, with C = 1).  Operands as mh_bce_loss: `logits`, `target` f32 [B, C]
 * dense.  A row is used iff none of its targets equals missing_val (base.py:120-123); for every used (b, l)
 *   cm[l][target > 0.5 ? 1 : 0][logit > logit_threshold ? 1 : 0] += 1,      cm int64 [C, 2, 2], the call ADDS.
 * DEVIATION from the reference, which tests sigmoid(logit) > thr in fp32: the host passes logit_threshold =
 * log(thr / (1 - thr)) (0 for the reference's 0.5).  The two forms differ only where the fp32 sigmoid rounds onto thr, i.e. for
 * |logit - logit_threshold| below about 1e-7.
 * 1 <= C <= 1024. */
int mh_confusion_bce(const float* logits, const float* target, float missing_val, float logit_threshold, long long* cm, int B,
                     int C, void* stream);

/* ---------------------------------------------------------------------------------------------- predictions (predict.hip)
 * The reference has no prediction path; a user of it takes the head's logits [B, 1, C, S, S]
 * (maestro/layers/head.py:116-130), torch.argmax over the class axis (maestro/layers/overlay.py:11-23) and, for a confidence,
 * torch.softmax.  Test-time augmentation undoes the transforms the models are trained under (maestro/dataset/dataset.py:224-257:
 * per sample, flip the rows, flip the columns, swap the two axes, in this order; the flag byte of mh_dihedral).
 *
 * Operands as for mh_ce_loss / mh_confusion_ce: `logits` is f32 in patch layout [B * g * g, ld >= P * P * C], column
 * (p1 * P + p2) * C + c of token row (b * g + ty) * g + tx is class c of pixel (ty * P + p1, tx * P + p2) of the S x S raster,
 * S = g * P; classification heads are g = P = 1.  Any ld and a 4-byte aligned base are accepted, 16-byte loads are used where
 * ld % 4 == 0 and the base is 16-byte aligned, pad columns are never read, every logit is read once. */
#define MH_PREDICT_SOFTMAX 0
#define MH_PREDICT_SIGMOID 1
/* One view of the batch.  `flags` (u8 [B], or NULL = identity) is the mh_dihedral flag byte that produced sample b's view: bit 0
 * flipped the rows, bit 1 the columns, bit 2 then swapped the axes.  Pixel (y, x) of the view is written at its place (y0, x0) of
 * the UNTRANSFORMED raster:  (y0, x0) = bit 2 ? (x, y) : (y, x);  bit 1: x0 = S - 1 - x0;  bit 0: y0 = S - 1 - y0.
 *
 * act = MH_PREDICT_SOFTMAX (2 <= C <= 128), in fp32 with m = max_j l_j:
 *   prob  f32 raster [B, C, S, S] (the layout of the logits a reference user holds):
 *         prob[b, c, y0, x0] = (accumulate ? old : 0) + exp(l_c - m) / sum_j exp(l_j - m) -- a plain read-modify-write by the one
 *         thread that owns the pixel; no atomics
 *   cls   u8 [B, S, S]: torch.argmax of the logits -- the lowest index among equal maxima, a NaN is the maximum and the first NaN
 *         wins (the rule of mh_confusion_ce, one device function)
 *   conf  f32 [B, S, S]: 1 / sum_j exp(l_j - m), the largest class probability
 * act = MH_PREDICT_SIGMOID (1 <= C <= 1024, g = P = 1, flags ignored), `threshold` a LOGIT threshold (the decision of
 * mh_confusion_bce):
 *   prob  f32 [B, C] (+)= 1 / (1 + exp(-l));  cls u8 [B, C] = l > threshold;  conf f32 [B, C] = 1 / (1 + exp(-l))
 * Each of prob, cls and conf may be NULL, not all three.  `threshold` is ignored for the softmax. */
int mh_predict_view(const float* logits, const uint8_t* flags, int act, float threshold, float* prob, int accumulate, uint8_t* cls,
                    float* conf, int B, int g, int P, int C, int ld, void* stream);
/* After 1 / inv_views accumulated views.  `prob` is [B, C, n_pix] (n_pix = S * S, or 1 for classification heads).
 *   softmax: cls[b, pix] = arg-max over c of prob[b, c, pix] under the same rule, conf[b, pix] = max * inv_views
 *   sigmoid: cls[b, c] = prob * inv_views > threshold (`threshold` a PROBABILITY here), conf[b, c] = prob * inv_views (n_pix = 1)
 *   mean (f32, the shape of prob; may be prob itself) = prob * inv_views, the mean probabilities: conf is their largest, bit for bit
 * Each of cls, conf and mean may be NULL, not all three. */
int mh_predict_finish(const float* prob, float inv_views, int act, float threshold, uint8_t* cls, float* conf, float* mean, int B, int C,
                      long n_pix, void* stream);

/* ---------------------------------------------------------------------------------------------- scene prediction (scene.hip)
 * The window cut in front of the prediction path, the weighted accumulation of overlapping windows into a scene canvas behind
 * it, and the canvas finish.  The reference cuts its training crops on the host, every modality at its own pixel scale on one
 * common grid of UNITS (maestro/dataset/dataset.py:86-105, the size_gcd / crop_gcd rule of maestro/conf/dataset/utils.py:99-109),
 * and has no scene inference.  Here a window is W x W units, W the greatest common divisor of the model's raster sizes, and a
 * raster with q pixels per unit shows the window (y0, x0) at pixels [y0 * q, y0 * q + S) x [x0 * q, x0 * q + S), S = W * q.
 *
 * The window table: int32 rows (n, y0, x0, on) -- scene index, window origin in units, 1 for a real window and 0 for a pad slot
 * (pad slots are gathered, so the model sees finite data, and blend nothing).  Every entry point takes the table of the B slots
 * twice, as mh_reduce_ordered takes its job table: `table_host` is checked before the launch, `table_dev` is what the kernel
 * reads.  A row of `table_dev` that names no scene or leaves the raster is skipped on the device, never followed. */
#define MH_SCENE_MAX_SLOTS 1024      /* B of one launch */
#define MH_SCENE_MAX_S 4096          /* window side in pixels of mh_predict_blend (its profile sits in LDS) */
#define MH_SCENE_UNCOVERED 255       /* cls of a canvas pixel no window has reached */
/* out[b, p, y, x] = scene[n_b, p, y0_b * q + y, x0_b * q + x]: `scene` f32 [N, planes, Hs, Ws], `out` f32 [B, planes, S, S],
 * planes = dates * channels.  Pure data movement, bit-exact.  16-byte loads and stores where both bases are 16-byte aligned and
 * Ws, S and every x0 * q are multiples of 4, one float at a time otherwise (4-byte aligned bases).  Refused: a row of
 * `table_host` with n outside 0 .. N - 1 or a window that leaves the scene. */
int mh_window_gather(const float* scene, float* out, const int32_t* table_dev, const int32_t* table_host, int B, int N, int planes,
                     int Hs, int Ws, int S, int q, void* stream);
/* The B windows of one batch onto the canvas.  `prob` f32 [B, C, S, S] (the sum over views mh_predict_view leaves), `profile`
 * f32 [S], `acc` f32 [N, C, Hc, Wc], `wsum` f32 [N, Hc, Wc].  For every canvas pixel (n, Y, X) that at least one `on` slot covers,
 * with b1 < b2 < ... the covering slots and w_b = profile[Y - y0_b * q] * profile[X - x0_b * q]:
 *   wsum[n, Y, X]   = ((wsum + w_b1) + w_b2) ...
 *   acc[n, c, Y, X] = ((acc + (prob[b1, c, ..] * scale) * w_b1) + (prob[b2, c, ..] * scale) * w_b2) ...
 * every product and every sum a separately rounded fp32 operation (nothing is contracted into an FMA).  Pixels that no `on` slot
 * covers are neither read nor written.  No atomics: the thread of the LOWEST covering slot owns the pixel and walks the slots in
 * order, so the canvas bits depend on the order of the windows alone, not on how they are cut into launches.
 * 2 <= C <= 128, B <= MH_SCENE_MAX_SLOTS, S <= MH_SCENE_MAX_S.  Refused: a row of `table_host` as for mh_window_gather. */
int mh_predict_blend(const float* prob, float scale, const float* profile, const int32_t* table_dev, const int32_t* table_host,
                     float* acc, float* wsum, int B, int N, int C, int S, int q, int Hc, int Wc, void* stream);
/* After the last batch.  `acc` f32 [N, C, n_pix], `wsum` f32 [N, n_pix], n_pix = Hc * Wc.
 *   cls  u8  [N, n_pix]: the arg-max over c of acc under the rule of mh_predict_view (one device function: the lowest index among
 *        equal maxima, a NaN is the maximum and the first NaN wins)
 *   conf f32 [N, n_pix]: that maximum / wsum;  mean f32 [N, C, n_pix] (may be `acc` itself) = acc / wsum
 * with correctly rounded divisions; wsum == 0 (no window reached the pixel): cls = MH_SCENE_UNCOVERED, conf = 0, mean = 0.
 * Each of cls, conf and mean may be NULL, not all three.  2 <= C <= 128. */
int mh_predict_blend_finish(const float* acc, const float* wsum, uint8_t* cls, float* conf, float* mean, int N, int C, long n_pix,
                            void* stream);

/* ---------------------------------------------------------------------------------------------- nearest neighbours (knn.hip)
 * Row normalisation of exported encoder features, the top-k cosine neighbours of bf16 queries in a bf16 feature bank, and the
 * weighted vote over their labels.  The reference trains and scores its models through heads only
 * (maestro/layers/head.py:116-130 gives the logits, maestro/train/metric.py the scores) and has no label-free evaluation of a
 * pretrained encoder.  The protocol stated here is the weighted k-NN classifier of DINO (Caron et al., "Emerging Properties in
 * Self-Supervised Vision Transformers", ICCV 2021, section 4.1, after Wu et al., CVPR 2018): features are L2-normalised with the
 * rule of torch.nn.functional.normalize (x / max(||x||_2, eps)), the k bank rows of largest cosine similarity vote for their
 * labels with weight exp(sim / T).
 *
 * The order rule.  Pairs (similarity, global index) are totally ordered: the larger similarity first, then the smaller index; an
 * index below zero (an unfilled slot) comes after every real index, and a NaN similarity is no candidate at all.  Every list
 * below is the head of its candidate set under this order, so it does not depend on how the work was cut. */
#define MH_KNN_MAX_K 128
/* The bank-split rule of mh_knn_topk: how many ways the bank is cut across workgroups so that few queries still fill the chip.
 * A function of its arguments alone (no device query); 1 <= splits <= the number of 128-row bank tiles.  0 for arguments
 * mh_knn_topk would refuse. */
int mh_knn_splits(int Nq, int Nb, int E, int k);
/* Bytes of the workspace of mh_knn_topk for `splits` splits: splits * Nq * k pairs of (f32, i32).  -1 for refused arguments. */
long mh_knn_workspace_bytes(int Nq, int k, int splits);
/* y[r, c] = x[r, c] / max(||x[r, :]||_2, eps) for `rows` rows of E columns; x f32 with row pitch ldx, y f32 with pitch ldy (may
 * be NULL, may be x itself with ldy == ldx), y16 bf16 with pitch ldy16 (may be NULL; not both): the round-to-nearest-even bf16 of
 * the fp32 quotient, bit for bit.  The sum of squares: lane l of a 64-lane wave takes s_l = fma(x_c, x_c, s_l) over its columns
 * c = l, l + 64, ... in ascending order, the 64 partial sums are folded by the xor butterfly 32, 16, ... 1, all in fp32: an
 * order that depends on E alone.  Then one correctly rounded sqrt, max with eps, and one correctly rounded division per element.
 * A zero row gives zeros.  4-byte aligned x and y, 2-byte aligned y16, any pitch >= E.  1 <= E <= 65536, eps >= 0. */
int mh_l2_normalize(const float* x, long ldx, float eps, float* y, long ldy, uint16_t* y16, long ldy16, long rows, int E,
                    void* stream);
/* The k nearest bank rows of every query.  q bf16 [Nq, E] with pitch ldq, bank bf16 [Nb, E] with pitch ldb; 16-byte aligned
 * bases, pitches that are multiples of 8 and at most 2^20, E % 32 == 0, 32 <= E <= 1024, 1 <= k <= MH_KNN_MAX_K.
 * The similarity of a pair is the fp32 accumulator of v_mfma_f32_16x16x32_bf16 over the E / 32 blocks of 32 columns in ascending
 * order, started from zero: exact bf16 products, one order that depends on E alone -- not on the tile, split, chunk or row the
 * pair falls in.
 * sims f32 [Nq, k], idx i32 [Nq, k] (4-byte aligned, dense): per query the k first pairs (similarity, index_base + bank row)
 * under the order rule, sorted by it; unfilled slots hold (-inf, -1).  accumulate = 1: the incoming sims / idx rows are further
 * candidates (entries with idx < 0 or a NaN are none), so that a bank streamed in chunks gives the bits of one call;
 * accumulate = 0: they are not read.  Nb = 0 (bank may then be NULL) is accepted with accumulate = 1 only.  index_base >= 0,
 * index_base + Nb <= 2^31 - 1.
 * `splits` >= 1 cuts the bank's 128-row tiles evenly over that many workgroups per 64-query tile (mh_knn_splits gives the rule's
 * value; any value gives the same bits); the partial lists go to `ws` (16-byte aligned, at least
 * mh_knn_workspace_bytes(Nq, k, splits) bytes) and a second launch on the same stream merges them.  No [Nq, Nb] buffer exists. */
int mh_knn_topk(const uint16_t* q, long ldq, const uint16_t* bank, long ldb, long index_base, float* sims, int* idx, int accumulate,
                void* ws, long ws_bytes, int splits, int Nq, int Nb, int E, int k, void* stream);
/* The weighted vote over the first k_eval <= k entries of every sorted list (sims, idx: [Nq, k] as mh_knn_topk leaves them).
 *   w_j = sims[j] == sims[0] ? 1 : exp((sims[j] - sims[0]) * inv_T)      (fp32: one subtraction, one product, expf)
 *   scores[n, c] = sum over j in ascending order of w_j [labels[idx_j] == c], each sum one fp32 addition, from 0
 * An entry with idx < 0, idx >= n_labels, a label equal to missing_val or a label outside [0, C) adds nothing.  labels i32
 * [n_labels].  scores f32 [Nq, lds >= C] (pad columns untouched), cls i32 [Nq]: the lowest class among equal maxima of the
 * scores just written (the arg-max rule of mh_confusion_ce), -1 when no entry voted.  Either may be NULL, not both.
 * 2 <= C <= 1024, inv_T > 0 and finite, 1 <= k_eval <= k <= MH_KNN_MAX_K. */
int mh_knn_vote(const float* sims, const int* idx, const int* labels, long n_labels, int missing_val, float inv_T, int k, int k_eval,
                float* scores, long lds, int* cls, int Nq, int C, void* stream);

/* ---------------------------------------------------------------------------------------------- misc
 * column sums: out[n] += sum_m x[m, n]  (bias gradients); x bf16 or f32; atomically accumulated. */
int mh_colsum(const void* x, int x_is_f32, float* out, int M, int N, int ld, void* stream);
/* Column sums, first phase (the deterministic form: the arithmetic of mh_colsum without its final atomic add):
 * x bf16 or f32 [M, ld] (N <= ld, N % 4 == 0, ld % 4 == 0); partial f32 [mh_colsum_partial_rows(M), N] dense, 16-byte aligned,
 * every element written by a plain store.  Row block i sums rows [256 i, 256 i + 256) of x. */
#define MH_COLSUM_PARTIAL_ROWS 256 /* rows per row block of mh_colsum_partial: a constant, so the partial layout depends on M alone */
int mh_colsum_partial_rows(int M);
int mh_colsum_partial(const void* x, int x_is_f32, float* partial, int M, int N, int ld, void* stream);
/* Zero n_spans (offset, length) float ranges of one buffer (spans: device array of 2*n_spans longs; max_len = longest span).
 * Used to clear only the atomically accumulated gradient slots when the weight gradients are stored by the grouped GEMM. */
int mh_zero_spans(float* base, const long* spans_device, int n_spans, long max_len, void* stream);
/* x[0..n) *= *scale with the scalar read on the device; a no-op when it equals 1 (the autograd bridge of the Lightning
 * surface, maestro/train/base.py:242-247: loss.backward() hands over d loss as a device tensor). */
int mh_scale_dev(float* x, long n, const float* scale, void* stream);
/* f32 -> bf16 cast of a flat buffer (weight shadow copies). */
int mh_cast_bf16(const float* src, void* dst, long n, void* stream);
/* f32 [E, K] -> bf16 [E, Kpad] (zero padded rows: patch-embed conv weight [E, C*P*P]) and the transpose for grads:
 * dst f32 [E, K] += src f32 [E, Kpad][:, :K]. */
int mh_pack_rows_bf16(const float* w, void* dst, int E, int K, int Kpad, void* stream);
int mh_unpack_rows_add(const float* src, float* dst, int E, int K, int Kpad, void* stream);
/* Fused AdamW over a flat parameter buffer (torch.optim.AdamW semantics, maestro/train/model.py:135-140): decoupled
 * weight decay, bias correction, grads pre-multiplied by grad_scale; refreshes the bf16 shadow copy (optional).
 * n % 4 == 0, step >= 1. */
int mh_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float lr, float b1, float b2,
             float eps, float wd, int step, float grad_scale, void* stream);
/* The same update that also refreshes the OCP e4m3 weight shadows of the fp8 path: p_fp8 = flat uint8 buffer with the
 * parameters' offsets (same n), slot_map[i / 64] = scale slot of element i's weight or -1 (short; parameters are 64-element
 * aligned), cast with scale[slot] (derived from the previous step's absmax by mh_fp8_update_scales), |new value| folded into
 * amax row `slot`.  The slices passed must start at a multiple of 64 elements of the flat buffer the map was built for. */
int mh_adamw_fp8(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_fp8, const short* slot_map,
                 const float* scale, float* amax, long n, float lr, float b1, float b2, float eps, float wd, int step,
                 float grad_scale, void* stream);
/* The same update with the per-step scalars read from DEVICE memory, so that the launch can sit inside a captured hipGraph
 * (the optimizer step overlapped with the next forward): hyper = f32 [5] = {lr, 1 - b1^step, sqrt(1 - b2^step), grad_scale,
 * active}; active == 0 makes the launch a no-op (no update pending). */
int mh_adamw_dev(float* p, const float* g, float* m, float* v, void* p_bf16, long n, float b1, float b2, float eps,
                 float wd, const float* hyper, void* stream);

/* AdamW parameter groups: per-group learning-rate scale and weight decay inside the one fused launch over the flat parameter
 * buffer.
 *
 * What it answers in the reference: the finetune configuration's layer-wise learning-rate decay.  OptFinetuneConfig.lw_decay
 * (maestro/conf/opt.py:51) is handed on by SSLTrainer (maestro/train/trainer.py:43-52); maestro/train/baseline.py:110-131 turns it
 * into AdamW parameter groups and a per-group OneCycleLR(max_lr=[...]); the groups are geometric in depth
 * (maestro/baselines/dinov2.py:312-373): patch_embed at rate^(depth + 1), block i at rate^(depth - i), heads at the base rate.
 * OneCycleLR is linear in max_lr, so a per-group rate is the scalar schedule times a constant scale: that scale is what the
 * table below holds.  The other use of parameter groups, no weight decay on 1-d parameters, is the second table.
 *
 * The update arithmetic is mh_adamw's, one function in the library: a launch of mh_adamw_groups gives, on every span of one
 * group, the bits of mh_adamw over that span with lr = fmul_rn(lr, lr_scale[g]) and wd = wd[g]. */
/* Elements per byte of the group map (the alignment of every parameter in the flat layout) and the length of both tables. */
#define MH_ADAMW_GROUP_BLOCK 64
#define MH_ADAMW_GROUP_TABLE 256
/* mh_adamw with per-group learning-rate scale and weight decay.  group_of[i / 64] = group of element i (parameters are
 * 64-element aligned; p must start on a 64-element block of the layout the map was built for, the caller offsets the map
 * pointer for a slice): ceil(n / 64) bytes are read.  lr_scale and wd are DEVICE float[256] tables (always 256 long, so any
 * byte of the map indexes inside them); element i is updated with lr_g = fmul_rn(lr, lr_scale[g]) and wd[g].  p, g, m, v: f32,
 * 16-byte aligned; p_bf16 (may be null): the bf16 shadow of p, 8-byte aligned.  n > 0, n % 4 == 0, step >= 1. */
int mh_adamw_groups(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                    const float* lr_scale, const float* wd, long n, float lr, float b1, float b2, float eps, int step,
                    float grad_scale, void* stream);
/* The same with {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active} from device memory (mh_adamw_dev's hyper[5]): with
 * hyper[4] == 0 the kernel returns before it touches memory. */
int mh_adamw_groups_dev(float* p, const float* g, float* m, float* v, void* p_bf16, const unsigned char* group_of,
                        const float* lr_scale, const float* wd, long n, float b1, float b2, float eps,
                        const float* hyper, void* stream);

/* AdamW with bf16 moments: both Adam moments stored as bf16 with stochastic rounding inside the one fused launch.  The update
 * stream drops from 30 to 22 bytes per parameter (p 8, g 4, m16 4, v16 4, bf16 shadow 2) and the optimizer state from 8 to 4
 * bytes per parameter.  No atomics.
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
 * RANDOM WORDS.  Philox4x32-10 as for the mask draws (mh_mask_draw: same multipliers, key increments and rounds), one call per
 * quad of elements: key = (seed & 0xffffffff, seed >> 32), counter
 *     c0 = (elem_base + i) / 4 (low 32 bits),   c1 = step (low 32 bits),   c2 = 0,   c3 = MH_ADAMW_SR_TAG
 * and element e = (elem_base + i) % 4 of the quad takes
 *     m:  (w[e >> 1] >> 16 * (e & 1)) & 0xffff        v:  (w[2 + (e >> 1)] >> 16 * (e & 1)) & 0xffff
 * elem_base is the offset of p[0] in the caller's flat layout: a split launch, a slice and one whole launch store the same
 * bits.  step is Adam's t after the increment.  MH_ADAMW_SR_TAG differs from every c3 of the mask draws (kind | stream << 4 |
 * attempt << 16 stays below 2^22 there), so no counter of the rounding draws is a counter of a mask draw under the same seed.
 *
 * p, g: f32, 16-byte aligned; m16, v16, p_bf16 (may be null): bf16, 8-byte aligned (one 8-byte store per quad each).
 * n > 0, n % 4 == 0, elem_base >= 0, elem_base % 4 == 0 (% 64 in the grouped forms: the map has one byte per 64 elements),
 * step >= 1. */
#define MH_ADAMW_SR_TAG 0x5352424Du /* c3 of every rounding draw ("SRBM") */
/* mh_adamw with bf16 moments. */
int mh_adamw_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed, float lr,
                   float b1, float b2, float eps, float wd, int step, float grad_scale, void* stream);
/* mh_adamw_dev with bf16 moments: hyper = {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale, active} (mh_adamw_dev's float[5]), step_dev =
 * a device word holding Adam's t (MhGuardState.t, read after mh_grad_guard_finish): its low 32 bits are the counter's step.
 * With hyper[4] == 0 the kernel returns before it touches memory. */
int mh_adamw_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, long n, long elem_base, uint64_t seed,
                       float b1, float b2, float eps, float wd, const float* hyper, const long long* step_dev, void* stream);
/* mh_adamw_groups with bf16 moments: group_of, lr_scale, wd as in mh_adamw_groups (p starts on a 64-element block of the
 * layout the map was built for, so elem_base % 64 == 0). */
int mh_adamw_groups_bf16m(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                          const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float lr, float b1,
                          float b2, float eps, int step, float grad_scale, void* stream);
/* mh_adamw_groups_dev with bf16 moments (hyper and step_dev as above). */
int mh_adamw_groups_bf16m_dev(float* p, const float* g, void* m16, void* v16, void* p_bf16, const unsigned char* group_of,
                              const float* lr_scale, const float* wd, long n, long elem_base, uint64_t seed, float b1, float b2,
                              float eps, const float* hyper, const long long* step_dev, void* stream);

/* ---------------------------------------------------------------------------------------------- gradient guard
 * The global L2 norm of the flat gradient buffer, the clipping coefficient and the non-finite skip, computed on the device and
 * handed to mh_adamw_dev through its five device scalars.
 *
 * What it answers in the reference: the trainer runs precision="16-mixed" (maestro/conf/trainer.py:13), so Lightning's GradScaler
 * skips the optimizer step of maestro/train/model.py:135-140 (AdamW + OneCycleLR) whenever a gradient is inf / NaN, and a
 * Trainer(gradient_clip_val=...) clips by the global norm with torch.nn.utils.clip_grad_norm_, whose coefficient rule
 *     coef = min(1, max_norm / (norm + 1e-6))
 * is restated here.  A skipped step does not advance Adam's step count (GradScaler semantics).
 *
 * No atomics: every sum has ONE order, fixed by the arguments, so the same gradient gives the same bits on every run and on
 * every rank. */
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
