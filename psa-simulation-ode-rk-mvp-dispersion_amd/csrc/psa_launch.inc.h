// psa_launch.inc.h -- the host half of every sweep launch, once: runtime values to template arguments (with_int, with_bool)
// and the launch of a picked kernel over `lanes` lanes (launch_lanes).  The numbers are the functions of psa_launch_rules.h.
#pragma once
#include <type_traits>

#include "psa_internal.h"

namespace psa {

// f(std::integral_constant<int, V>{}) for the V equal to v -- the last one when none is
template <int V, int... Vs, typename F>
static hipError_t with_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : with_int<Vs...>(v, f);
}
template <typename F>
static hipError_t with_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// One launch on s of `kernel` (its one argument the struct a, by value) over `lanes` lanes in workgroups of `block` threads
// with lds_bytes of dynamic LDS; nothing for an empty sweep.  By the kernel's address: a <<< >>> call through a pointer is lost
// in the host-sanitizer build.  Above the 64 KiB a launch gets by default (the float32 comb alone) the kernel's limit is raised
// first.  The attribute belongs to the function ON THE CURRENT DEVICE, and a sweep split over devices launches from one thread
// per device: it is set at every such launch (a host call without a device round trip) rather than remembered per kernel and device.
template <typename Args>
static hipError_t launch_lanes(const void *kernel, long long lanes, int block, size_t lds_bytes, const Args &a, hipStream_t s) {
    if (lanes == 0) return hipSuccess;
    if (lds_limit_raised(lds_bytes)) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    void *args[] = {const_cast<Args *>(&a)};
    (void)hipLaunchKernel(kernel, dim3(grid_blocks(lanes, block)), dim3(block), args, lds_bytes, s);
    return hipGetLastError();
}

}  // namespace psa
