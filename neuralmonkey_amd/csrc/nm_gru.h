// Operands of one GRU time step as the fused epilogues see them (nm_gemm.hip: the per-step launches;
// nm_gru_cluster.hip: the whole time loop in one launch).  TF GRUCell (nn/ortho_gru_cell.py:44-53) under
// dynamic_rnn's length masking and reverse_sequence (encoders/recurrent.py:86-102).
#pragma once
#include "nm_common.h"
#include "../../include/nmhip.h"      // nm_gru_epilogue: what the callers hand over, GruEpi is its device-side form

struct GruEpi {
    int mode;
    const int* lengths;
    int t, rev_mask, H;
    long R;
    // forward
    const float* xp; long x_dir, x_row, x_time;
    const float* h_in; float* h_out; float* ru; float* rh; float* c_save;
    float* out; long o_dir, o_row, o_time;
    // backward
    float* dh; const float* dout; long do_dir, do_row, do_time;
    const float* c; const float* h0; const float* hseq; long hs_dir, hs_row, hs_time;
    float* dxp; long dx_dir, dx_row, dx_time;
    float* dgpre; float* dcpre;
};

// The length / reversal rule of a GRU step (the fused epilogues here and the pointwise backward kernels of
// nm_backward.hip; gru_pos of nm_elementwise.hip states its forward half again: calling this from there changes that
// file's device code): at step t, row r of direction d stands at sequence position ``pos`` -- tf.reverse_sequence
// indexing when the direction's bit of rev_mask is set -- and stood at ``ppos`` one step earlier; false: the row has
// ended (t >= its length).
__device__ __forceinline__ bool gru_step_pos(const int* lengths, int rev_mask, int r, int d, int t, int& pos, int& ppos) {
    pos = t;
    const bool rev = (rev_mask >> d) & 1;
    if (lengths) {
        const int len = lengths[r];
        if (t >= len) return false;
        if (rev) pos = len - 1 - t;
    }
    ppos = rev ? pos + 1 : pos - 1;
    return true;
}

__device__ __forceinline__ bool gru_epi_pos(const GruEpi& e, int r, int d, int t, int& pos, int& ppos) {
    return gru_step_pos(e.lengths, e.rev_mask, r, d, t, pos, ppos);
}

__device__ __forceinline__ float gru_epi_hprev(const GruEpi& e, long ro, int d, int r, int t, int ppos,
                                               int col) {
    if (t == 0) return e.h0 ? e.h0[ro * e.H + col] : 0.0f;
    return e.hseq[d * e.hs_dir + (long)r * e.hs_row + (long)ppos * e.hs_time + col];
}
