// Error plumbing for the C-ABI: thread-local last-error string, no exceptions cross the boundary.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

static thread_local char g_last_error[1024] = "";
static thread_local char g_last_kernel[160] = "";

void pso_note_kernel(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_kernel, sizeof(g_last_kernel), fmt, ap);
  va_end(ap);
}

void pso_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
}

int pso_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    pso_set_error("%s: %s", what, hipGetErrorString(e));
    return PSO_ERR_HIP;
  }
  return PSO_OK;
}

bool pso_dtype_ok(int code, const char* who) {
  if (code == PSO_F32 || code == PSO_ELEM) return true;
  if (code == PSO_BF16 || code == PSO_F16)
    pso_set_error("%s: this library's 16-bit element type is " PSO_ELEM_NAME " (dtype code %d); %s tensors need %s "
                  "(PSO_LIB=%s)", who, PSO_ELEM, code == PSO_F16 ? "fp16" : "bf16",
                  code == PSO_F16 ? "libpso_amd_f16.so" : "libpso_amd.so", code == PSO_F16 ? "f16" : "unset");
  else
    pso_set_error("%s: bad dtype code %d", who, code);
  return false;
}

extern "C" {
const char* pso_last_error(void) { return g_last_error; }
const char* pso_last_kernel(void) { return g_last_kernel; }
int pso_abi_version(void) { return PSO_ABI_VERSION; }
int pso_elem_dtype(void) { return PSO_ELEM; }
}
