// The error state of a library that spans several translation units (libhode.so, libhode_neural_odd.so and the like): the thread-local
// message its *_last_error_string returns, and the definitions of hode::fail / hode::hip_fail that hode_host.hpp declares
// for every unit.  The two functions have external linkage, so this header is included by exactly ONE unit per library
// (hode_api.hip, neural_odd/hode_neural_odd.hip, roche_dims/hode_roche_dims.hip, real_dims/hode_real_dims.hip); each library thereby keeps a message of its own.  The single-unit side
// libraries use hode_side_error.hpp, whose copy has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>

#include "hode_host.hpp"

namespace hode {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

}  // namespace hode
