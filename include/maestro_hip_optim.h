/* C ABI of libmaestro_hip.so, AdamW parameter groups: per-group learning-rate scale and weight decay inside the one fused
 * launch over the flat parameter buffer.
 *
 * What it answers in the reference: the finetune configuration's layer-wise learning-rate decay.  OptFinetuneConfig.lw_decay
 * (maestro/conf/opt.py:51) is handed on by SSLTrainer (maestro/train/trainer.py:43-52); maestro/train/baseline.py:110-131 turns it
 * into AdamW parameter groups and a per-group OneCycleLR(max_lr=[...]); the groups are geometric in depth
 * (maestro/baselines/dinov2.py:312-373): patch_embed at rate^(depth + 1), block i at rate^(depth - i), heads at the base rate.
 * OneCycleLR is linear in max_lr, so a per-group rate is the scalar schedule times a constant scale: that scale is what the
 * table below holds.  The other use of parameter groups, no weight decay on 1-d parameters, is the second table.
 *
 * The conventions are those of maestro_hip.h: plain pointers + sizes, device pointers are DEVICE memory owned by the caller;
 * asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, allocates nothing, reads no environment, keeps
 * no global mutable state, graph-capturable; returns 0 on success, -1 for a bad argument (nothing is launched), >0 =
 * hipError_t; the message is read with the main header's error call.
 *
 * The update arithmetic is mh_adamw's, one function in the library: a launch of mh_adamw_groups gives, on every span of one
 * group, the bits of mh_adamw over that span with lr = fmul_rn(lr, lr_scale[g]) and wd = wd[g].
 *
 * These declarations live in a header of their own until the guard-band ledger of the test suite lists them.
 */
#ifndef MAESTRO_HIP_OPTIM_H
#define MAESTRO_HIP_OPTIM_H
#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
