/* libnmhip -- C ABI of the sequence splitter (the entry point lives beside the sentence-level heads in
 * csrc/nm_pool.hip), a companion of nmhip.h with the same conventions: every function returns 0 on success, <0 on error
 * with the text in nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32); `stream` is a
 * hipStream_t passed as void*; sizes are int64_t element counts.  Arguments are checked before anything is launched.
 *
 * Reference: neuralmonkey/model/sequence_split.py.  The split of the states themselves is a reshape of contiguous
 * memory and needs no kernel; what does is the mask of the longer sequence (sequence_split.py:60-66: every entry of the
 * parent's mask `factor` times) and its lengths (model/stateful.py:55-62: int32 row sums of the mask). */
#ifndef NMHIP_SPLIT_H
#define NMHIP_SPLIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* mask [B, T] float 0/1, contiguous -> out_mask [B, T*factor], out_mask[b*T*factor + t*factor + j] = mask[b*T + t] for
 * j < factor, and lengths[b] = (int32) sum_t mask[b*T + t] * factor, in one launch.
 * Refused: B, T, factor < 1; T or factor of 2^24 and more (the row sum is taken in fp32), T*factor or B of 2^31 and more;
 * a null pointer; out_mask overlapping mask. */
int nm_split_mask(void* stream, const float* mask, int64_t B, int64_t T, int64_t factor, float* out_mask,
                  int32_t* lengths);

#ifdef __cplusplus
}
#endif
#endif
