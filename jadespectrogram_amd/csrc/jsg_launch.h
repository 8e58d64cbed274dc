// Launching a kernel that asks for more dynamic LDS than a kernel gets without asking: what the launchers of libjsg.so (jsg_internal.h)
// and of libjsgx.so (jsgx_internal.h) share.  Templates and a class without a static member: each library keeps its own OncePerDevice
// objects in its own units, and the two share this text, no object code and no state.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>

namespace jsg {

// What has been said once per device, a bit per path of a unit.  A device index outside 0..63 has no slot: there every call is the
// first.  done() after the step has succeeded, so that a failed first attempt is made again.
class OncePerDevice {
public:
    bool first(int dev, unsigned bit) const { return dev < 0 || dev >= 64 || !(told_[dev].load(std::memory_order_acquire) & bit); }
    void done(int dev, unsigned bit) {
        if (dev >= 0 && dev < 64) told_[dev].fetch_or(bit, std::memory_order_release);
    }

private:
    std::atomic<unsigned> told_[64] = {};
};

// Launches a kernel with lds_bytes of dynamic LDS, up to lds_max.  The runtime has to be told lds_max once per device and kernel
// before the first such launch there; `once` and the path's bit remember it, so it is told at the first launch of a path on a device.
// Telling is no stream operation, so a first launch under capture works.
template <class Args>
hipError_t launch_large_lds(OncePerDevice& once, int dev, unsigned bit, void (*kernel)(Args), int lds_max, dim3 grid, dim3 block, size_t lds_bytes,
                            hipStream_t s, const Args& k) {
    const bool first = once.first(dev, bit);
    if (first) {
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (err != hipSuccess) return err;
    }
    void* args[] = {const_cast<Args*>(&k)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, args, lds_bytes, s);
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess && first) once.done(dev, bit);
    return err;
}

}  // namespace jsg
