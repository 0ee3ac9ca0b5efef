// zs_api.hip -- error state, version and kernel-selection knobs of libzs_amd.so (see include/zs_amd.h).
#include <stdarg.h>

#include "zs_common.h"

static thread_local char g_err[512] = "";

void zs_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

Knob* g_knobs = nullptr;

extern "C" int zs_set_option(const char* key, int value) {
  for (Knob* k = g_knobs; key && k; k = k->next)
    if (!strcmp(k->key, key)) return k->set(value);
  zs_set_error("zs_set_option: unknown key %s", key ? key : "(null)");
  return ZS_EINVAL;
}

extern "C" int zs_get_option(const char* key) {
  for (Knob* k = g_knobs; key && k; k = k->next)
    if (!strcmp(k->key, key)) return k->get();
  zs_set_error("zs_get_option: unknown key %s", key ? key : "(null)");
  return ZS_EINVAL;
}

int zs_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    zs_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return ZS_ELAUNCH;
  }
  return ZS_OK;
}

extern "C" int zs_abi_version(void) { return ZS_ABI_VERSION; }
extern "C" const char* zs_last_error(void) { return g_err; }
