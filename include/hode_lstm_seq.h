/* C ABI of libhode_lstm_seq.so: the masked single-layer LSTM of hode.h (hode_lstm_fwd / hode_lstm_bwd) with the hidden state
 * of EVERY step as its output, gfx950 -- a sequence-to-sequence LSTM (reference model.py:322-380 LSTMBaseline, and
 * EncoderLSTMReal(output_all=True), model.py:236-237).  libhode.so's kernels keep h on chip and emit the final state only;
 * these are the same kernel bodies (csrc/hode_lstm_kernels.hpp) under their all-steps policy, launched by the same host
 * code (csrc/hode_lstm.hip, csrc/hode_lstm_tpw.hip compiled a second time).
 *
 * Every entry takes hode.h's hode_lstm_desc and has the signature and the contract of its hode_lstm_* namesake there --
 * the same sizes (hidden_dim <= 160), the same refusals and codes, the same workspace layout, c_out, grad_gates, h_prev,
 * reverse, save_tape and patient_tiles -- except for two fields, which are read differently:
 *
 *     h_out       [T][B][H]  out: row t is the hidden state after the step that consumed input row t, whichever way the
 *                            window is walked (reverse = 1: row 0 is the state after all T steps)
 *     grad_h_out  [T][B][H]  in (hode_lstm_seq_bwd): the cotangent of every row of h_out
 *
 * c_out stays [B][H], the cell state after the last processed step.  hode_lstm_seq_last_error_string() holds the message
 * of this library's last failed call on the calling thread; > 0 is a hipError_t from a launch. */
#ifndef HODE_LSTM_SEQ_H_
#define HODE_LSTM_SEQ_H_

#include "hode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_LSTM_SEQ_ABI_VERSION 1

int hode_lstm_seq_version(void);
const char* hode_lstm_seq_last_error_string(void);
/* 0 outside the domain (hode_lstm_seq_fwd then says why) */
size_t hode_lstm_seq_workspace_bytes(const hode_lstm_desc* desc);
int hode_lstm_seq_fwd(const hode_lstm_desc* desc, void* hip_stream);
int hode_lstm_seq_bwd(const hode_lstm_desc* desc, void* hip_stream);
/* as hode_lstm_fill_operand: the x * mask columns of the weight-gradient operand rows of the hode_lstm_seq_bwd call */
int hode_lstm_seq_fill_operand(const hode_lstm_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_LSTM_SEQ_H_ */
