// What the translation units behind the C ABI (maxsim_abi.hip and abi_*.hip; see include/maxsim.h) share: the error buffer, the per-device
// cache and a few one-line helpers.  Host-only declarations; the state itself lives in abi_core.cpp.  Everything here has hidden visibility:
// the library exports the msim_* entry points and nothing of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstddef>
#include <cstdlib>

#include "../../include/maxsim.h"

#pragma GCC visibility push(hidden)
namespace msim_abi {

// formats the calling thread's msim_last_error() message and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// MSIM_OK, or the pending launch error as "<what> launch: <hip error>" and MSIM_ELAUNCH
int launch_failed(const char *what);

// an integer A/B knob from the environment -- measurement builds only (maxsim_common.hpp: kAbBuild); the shipped library returns
// the default without looking (inline, so that a shipped build does not even keep the knobs' names)
inline int ab_env(const char *name, int dflt) {
#if defined(MSIM_AB) || defined(MSIM_TRACE)
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

struct DeviceInfo {
    int cus = 0;
    int lds_per_cu = 0;
};

constexpr int kMaxDevices = 64;

// the current device's entry of the once-initialised per-device cache
int device_info(const DeviceInfo **out);

// kernels that ask for more than 64 KiB of dynamic LDS need the attribute raised once per (kernel, device)
template <class Kern>
int allow_lds(Kern kern, int bytes, std::atomic<int> *configured) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!configured[dev].load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "hipFuncSetAttribute(%d B LDS): %s", bytes, hipGetErrorString(e));
        configured[dev].store(1, std::memory_order_release);
    }
    return MSIM_OK;
}

// the second row width msim_fwd_candidates_wide and msim_align_candidates take (ColQwen3): 3 panels, 4 k-steps of 16 in the last
constexpr int kCandWideDim = 320;

inline int elem_bytes(int dtype) { return dtype == MSIM_DTYPE_F32 ? 4 : 2; }

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace msim_abi
#pragma GCC visibility pop
