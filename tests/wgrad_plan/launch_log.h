// Forced-include shim of the weight-gradient launch-plan recorder (wgrad_plan.hip, `hipcc --cuda-host-only -include launch_log.h`):
// after hip/hip_runtime.h, hipLaunchKernelGGL no longer launches but reports the kernel's full name, grid, dynamic LDS bytes and the
// all_csum field of its argument to the recorder.  The name comes from the compiler, not from a table: the type name of a tag
// instantiated on the kernel's address (__PRETTY_FUNCTION__ of such a helper leaves the kernel's template arguments out).
#pragma once
#include <hip/hip_runtime.h>
#include <typeinfo>

namespace regt { struct WgradArgs; }
namespace wgrad_plan {
void log_launch(const std::type_info& tag, dim3 grid, dim3 block, size_t lds_bytes, int all_csum);
int all_csum_of(const regt::WgradArgs& a);
template <class A> int all_csum_of(const A&) { return -1; }        // (the slab reduction's arguments have no such field)
template <auto K> struct KernelTag {};
}  // namespace wgrad_plan

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
    wgrad_plan::log_launch(typeid(wgrad_plan::KernelTag<(kernel)>), grid, block, lds_bytes, wgrad_plan::all_csum_of(__VA_ARGS__))
