// The state behind the C ABI (abi_common.hpp): the per-thread error message and the per-device cache, one copy for the whole
// library whichever translation unit an entry point lives in.  Host code only; no kernel is defined or launched here.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "abi_common.hpp"

namespace msim_abi {

namespace {

thread_local char g_err[512] = "";

// once-initialised per-device cache (with g_err the only mutable state shared between the translation units)
DeviceInfo g_dev[kMaxDevices];
std::atomic<int> g_dev_ready[kMaxDevices];

}  // namespace

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int launch_failed(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "%s launch: %s", what, hipGetErrorString(e));
    return MSIM_OK;
}

int device_info(const DeviceInfo **out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "hipGetDevice: %s", hipGetErrorString(e));
    if (dev < 0 || dev >= kMaxDevices) return fail(MSIM_ELAUNCH, "device ordinal %d out of range", dev);
    if (!g_dev_ready[dev].load(std::memory_order_acquire)) {
        hipDeviceProp_t p;
        e = hipGetDeviceProperties(&p, dev);
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "hipGetDeviceProperties: %s", hipGetErrorString(e));
        if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
            return fail(MSIM_EUNSUPPORTED, "libmaxsim_gfx950 is built for gfx950 (MI355X) only; device %d is %s", dev,
                        p.gcnArchName);
        g_dev[dev].cus = p.multiProcessorCount;
        g_dev[dev].lds_per_cu = 160 * 1024;
        g_dev_ready[dev].store(1, std::memory_order_release);
    }
    *out = &g_dev[dev];
    return MSIM_OK;
}

}  // namespace msim_abi

extern "C" {

int msim_abi_version(void) { return MSIM_ABI_VERSION; }

const char *msim_last_error(void) { return msim_abi::g_err; }

}  // extern "C"
