// libhode_lstm_seq.so (include/hode_lstm_seq.h): the LSTM window kernels under their all-steps policy.  This unit holds what
// the library needs beside ../hode_lstm.hip and ../hode_lstm_tpw.hip (both compiled with -DHODE_LSTM_SEQ_UNIT): the error
// state and the two entries that describe the library.  This library exists because libhode.so's set of kernel symbols is
// pinned.
#include <hip/hip_runtime.h>

#include "../../../include/hode_lstm_seq.h"
#include "../hode_error_state.hpp"  // hode::fail / hip_fail for this library's units: defined here, once

extern "C" int hode_lstm_seq_version(void) { return HODE_LSTM_SEQ_ABI_VERSION; }
extern "C" const char* hode_lstm_seq_last_error_string(void) { return hode::g_err; }
