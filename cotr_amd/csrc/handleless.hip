// The per-thread error message of the handle-less entry points (handleless.h) and the exported call that reads it.
#include <stdio.h>

#include "handleless.h"

namespace {
thread_local char g_error[256];   // the message of the last failed handle-less call on this thread
}  // namespace

namespace cotr_detail {
int handleless_fail(int code, const char* msg) {
  snprintf(g_error, sizeof g_error, "%s", msg);
  return code;
}

int arg_fail(const char* fn, const char* what, const char* note) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s%s", fn, what, note);
  return handleless_fail(COTR_ERR_ARG, msg);
}
}  // namespace cotr_detail

extern "C" const char* cotr_raster_last_error(void) { return g_error; }
