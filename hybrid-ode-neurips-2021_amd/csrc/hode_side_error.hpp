// Host-side error reporting of the single-translation-unit side libraries (libhode_flow.so, libhode_mix.so,
// libhode_blend.so): the thread-local message their hode_*_last_error_string returns, and the two ways to set it.
// Everything here has internal linkage (unnamed namespace), so each library gets a private copy: no state and no symbol
// is shared between them or with libhode.so, whose hode::fail / hip_fail (hode_api.hip) span many units and stay apart.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>

namespace hode_side {
namespace {

thread_local char g_err[512] = "";

// records the printf-style message and returns `code`, so that an entry point can `return fail(...)`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// 0 for hipSuccess; otherwise records "<what>: <HIP's text>" and returns the HIP error as the code
int launch_fail(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  return fail((int)e, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace
}  // namespace hode_side
