// Host-side helpers of every translation unit of the C ABI: the error state (one thread-local
// message, defined in lif_layers.hip, read back by snnflow_last_error), the two early-return macros
// of the exported functions and the load-time environment switches.
#pragma once

#include <cstdlib>

#include <hip/hip_runtime.h>

int snnflow_set_error(int code, const char* msg);

#define SNN_FAIL(code, msg) return snnflow_set_error((code), (msg))
#define SNN_CHECK_LAUNCH()                                                        \
    do {                                                                          \
        hipError_t e_ = hipGetLastError();                                        \
        if (e_ != hipSuccess) return snnflow_set_error((int)e_, hipGetErrorString(e_)); \
    } while (0)

// Integer environment switch (SNNFLOW_*), read once at load time by the unit that owns it.
inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
