/* libnmhip -- the GRU cluster time loops with their inputs and outputs in the callers' layouts (csrc/nm_gru_cluster.hip),
 * a companion of nmhip.h with the same conventions: every function returns 0 on success, <0 on error with the text in
 * nm_last_error(); tensor pointers are DEVICE pointers owned by the caller (fp32 / int32); `stream` is a hipStream_t
 * passed as void*; sizes and strides are int64_t element counts.  Arguments are checked before anything is launched. */
#ifndef NMHIP_GRU_SEQ_H
#define NMHIP_GRU_SEQ_H
#include "nmhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* nm_gru_seq_fwd / nm_gru_seq_bwd (nmhip.h) with the passes their callers launched around them done by the loop
 * kernels, which hold every one of these values in registers anyway.  Each member of `io` is optional (null / 0: off); `io` itself is required and
 * steps >= 1.  Everything else as nm_gru_seq_fwd / nm_gru_seq_bwd, which are these calls with nothing switched on.
 *   fwd_ex  e->h_in may be null: h_0 = 0                                  (replaces the zero fill of the state buffer);
 *           zero_padded: positions t >= lengths[row] of `out` get zeros   (replaces the zero fill of `out`);
 *           final_state[row * final_row + d * final_dir + col] = the state after the row's last valid step
 *                                                                         (replaces one nm_copy_cols per direction);
 *           hprev_seq / rh_seq (both or neither; element strides seq_dir, seq_row, seq_time as for `out`): at every
 *           valid position the h_{t-1} the step used and r * h_{t-1}, zeros at padded positions -- with h_0 = 0 what
 *           nm_gru_seq_shift and nm_gru_rh_seq compute from `out` and the saved gates (replaces both);
 *           h0_out [ndir][R][H]: a copy of the initial state              (replaces the copy of s_0 in front of the
 *                                                                          decoder's state sequence).
 *   bwd_ex  dL/dh after the last step is d_final[row * dfinal_row + d * dfinal_dir + col], zero when d_final is null;
 *           e->dh is only written (dL/dh_0)                (replaces the zero fill of dh and one nm_copy_cols per direction);
 *           zero_padded: positions t >= lengths[row] of dxp get zeros     (replaces the zero fill of dxp).
 * The zero stores and the final state are issued behind the last hand-off of the loop, never between two steps. */
typedef struct nm_gru_seq_io {
    int32_t zero_padded, reserved;
    float* final_state; int64_t final_row, final_dir;
    float* hprev_seq; float* rh_seq; int64_t seq_dir, seq_row, seq_time;
    float* h0_out;
    const float* d_final; int64_t dfinal_row, dfinal_dir;
} nm_gru_seq_io;
int nm_gru_seq_fwd_ex(void* stream, const nm_gru_epilogue* e, const nm_gru_seq_io* io, int32_t steps, int64_t h_step,
                      int64_t ru_step, int64_t rh_step, int64_t c_step, const float* wgh, int64_t ld_g,
                      int64_t stride_g, const float* wch, int64_t ld_c, int64_t stride_c, void* workspace,
                      int64_t workspace_bytes, uint32_t* sticky_error);
int nm_gru_seq_bwd_ex(void* stream, const nm_gru_epilogue* e, const nm_gru_seq_io* io, int32_t steps, int64_t ru_step,
                      int64_t c_step, const float* wgh, int64_t ld_g, int64_t stride_g, const float* wch,
                      int64_t ld_c, int64_t stride_c, void* workspace, int64_t workspace_bytes,
                      uint32_t* sticky_error);

#ifdef __cplusplus
}
#endif
#endif
