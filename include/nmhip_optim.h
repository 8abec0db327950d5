/* libnmhip -- C ABI of the optimizer family beyond Adam and Adadelta (csrc/nm_optim.hip), a companion of nmhip.h
 * with the same conventions: every function returns 0 on success, <0 on error with the text in nm_last_error(); tensor
 * pointers are DEVICE pointers owned by the caller (fp32 / int32 / int64 tables); `stream` is a hipStream_t passed as
 * void*; sizes are int64_t element counts.  Arguments are checked before anything is launched.  No kernel here uses
 * atomics: two runs are bit-equal.
 *
 * Reference: trainers/generic_trainer.py:64 takes any tf.train.Optimizer; these are TF 1.12's ApplyGradientDescent,
 * ApplyMomentum, ApplyAdagrad and ApplyRMSProp (core/kernels/training_ops.cc) as pass 3 of the flat optimizer: the chunk
 * and segment tables, the workspace (nm_optim_workspace_bytes) and the squared gradient norms in it are those of
 * nm_optim_partials / nm_optim_segments in nmhip.h, which run first.  One kernel template serves all six kinds; kinds 0
 * (Adam) and 1 (Adadelta) are launched through nm_optim_apply, which keeps its own argument checks. */
#ifndef NMHIP_OPTIM_H
#define NMHIP_OPTIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_OPTIM_SGD 2        /* tf.train.GradientDescentOptimizer: no slot        p0 = lr */
#define NM_OPTIM_MOMENTUM 3   /* tf.train.MomentumOptimizer: slot0 accum           p0 = lr, p1 = momentum, p2 != 0 Nesterov */
#define NM_OPTIM_ADAGRAD 4    /* tf.train.AdagradOptimizer: slot0 accum            p0 = lr */
#define NM_OPTIM_RMSPROP 5    /* tf.train.RMSPropOptimizer: slot0 ms, slot1 mom    p0 = lr, p1 = decay, p2 = momentum, p3 = epsilon */

/* Per-tensor clip + update over the chunks [chunk_begin, chunk_end), one workgroup of 256 per chunk.  With
 * g = grad * clip_norm / max(||grad||, clip_norm) per variable (clip_norm <= 0: g = grad), in fp32 and in this order:
 *   NM_OPTIM_SGD       var -= lr*g
 *   NM_OPTIM_MOMENTUM  accum = accum*momentum + g;  var -= lr*accum      (Nesterov: var -= g*lr + accum*momentum*lr)
 *   NM_OPTIM_ADAGRAD   accum += g*g;  var -= g*lr*rsqrt(accum)           (no epsilon)
 *   NM_OPTIM_RMSPROP   ms += (g*g - ms)*(1 - decay);  mom = mom*momentum + (g*lr)/sqrt(ms + epsilon);  var -= mom
 * Variables whose seg_flags lack bit 1 (not trainable) and the padding between variables are not touched.  A kind reads
 * and writes only the streams it has; a slot it does not have may be NULL and is never dereferenced.  skip_word (may be
 * NULL): a device word that, when not zero, turns the launch into a no-op.
 * Refused: a kind outside 2..5, a null theta, grad, workspace or table, a slot the kind needs missing, nchunk or
 * nseg < 1, a range outside [0, nchunk], a workspace smaller than nm_optim_workspace_bytes(nchunk, nseg).  An empty
 * range is a no-op. */
int nm_optim_update(void* stream, int32_t kind, float* theta, const float* grad, float* slot0, float* slot1,
                    const int64_t* chunk_start, const int32_t* chunk_len, const int32_t* chunk_seg,
                    const int32_t* seg_first, const int32_t* seg_count, const int32_t* seg_flags, int64_t nchunk,
                    int64_t nseg, float clip_norm, float p0, float p1, float p2, float p3, int64_t chunk_begin,
                    int64_t chunk_end, const int32_t* skip_word, void* workspace, int64_t workspace_bytes);

/* The same over a LIST of chunks (a device array of `count` chunk indices, each < nchunk, in any order, none twice):
 * everything a rank of the sharded optimizer owns in one launch.  Refused as above, plus count < 0, count > nchunk, or a
 * null list with count > 0.  count == 0 is a no-op. */
int nm_optim_update_list(void* stream, int32_t kind, float* theta, const float* grad, float* slot0, float* slot1,
                         const int64_t* chunk_start, const int32_t* chunk_len, const int32_t* chunk_seg,
                         const int32_t* seg_first, const int32_t* seg_count, const int32_t* seg_flags, int64_t nchunk,
                         int64_t nseg, float clip_norm, float p0, float p1, float p2, float p3,
                         const int32_t* chunk_list, int64_t count, const int32_t* skip_word, void* workspace,
                         int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
