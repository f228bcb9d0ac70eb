// pv_host.h -- host helpers of every translation unit of libpvvote.so: HIP
// status to the C ABI's return code, and the device's CU count.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pvvote.h"

namespace pvv __attribute__((visibility("hidden"))) {

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
// the status of the launches since the last check
inline int last() { return rc(hipGetLastError()); }

// CUs of the current device (256 if it cannot be asked), asked once: caller
// threads may race here, and a function-local static is initialised by one
inline int cu_count() {
    static const int n = [] {
        int dev = 0, cus = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        return cus > 0 ? cus : 256;
    }();
    return n;
}

}  // namespace pvv
