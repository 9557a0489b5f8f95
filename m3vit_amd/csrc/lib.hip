// Host-side plumbing of libm3vit_hip.so: error text, version, device query.
#include <stdarg.h>
#include <stdlib.h>

#include "common.h"

namespace m3 {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return M3_ERR_LAUNCH;
  }
  return M3_OK;
}

// m3_set_cache_hints' mask; < 0: the next launch reads M3_CACHE_HINTS (unset: the families that measured faster)
static int g_cache_hints = -1;
int cache_hints() {
  if (g_cache_hints < 0) {
    const char *e = getenv("M3_CACHE_HINTS");
    g_cache_hints = (e ? atoi(e) : M3_HINT_DEFAULT) & M3_HINT_ALL;
  }
  return g_cache_hints;
}

}  // namespace m3

extern "C" int m3_set_cache_hints(int mask) {
  M3_REQUIRE(mask >= -1 && mask <= M3_HINT_ALL, "m3_set_cache_hints: mask %d out of range", mask);
  m3::g_cache_hints = mask;
  return M3_OK;
}

extern "C" int m3_version(void) { return 100; }   // 0.1.0

extern "C" const char *m3_last_error(void) { return m3::g_err; }

extern "C" int m3_device_query(char *name, int len) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { m3::set_error("m3_device_query: no HIP device"); return M3_ERR_LAUNCH; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { m3::set_error("m3_device_query: hipGetDeviceProperties failed"); return M3_ERR_LAUNCH; }
  if (name && len > 0) {
    strncpy(name, prop.gcnArchName, (size_t)len - 1);
    name[len - 1] = 0;
  }
  return prop.multiProcessorCount;
}
