// Forced-include shim of the aggregation launch-plan recorder (spmm_plan.hip, `hipcc --cuda-host-only -include launch_log.h`):
// after hip/hip_runtime.h, hipLaunchKernelGGL no longer launches but reports the kernel's full name (the type name of a tag
// instantiated on the kernel's address, as tests/wgrad_plan/launch_log.h does), grid, block, dynamic LDS bytes and every argument of
// the launch in order: integers by value, pointers as <fake buffer>+<byte offset> (spmm_plan.hip names the buffers).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <typeinfo>

namespace spmm_plan {
void log_launch(const std::type_info& tag, dim3 grid, dim3 block, size_t lds_bytes, const std::string& args);
std::string ptr_text(const void* p);
template <auto K> struct KernelTag {};
template <class T> void put_arg(std::string& s, const T& v) {
    if (!s.empty()) s += ",";
    if constexpr (std::is_pointer_v<T> || std::is_null_pointer_v<T>) s += ptr_text(v);
    else if constexpr (std::is_signed_v<T>) s += std::to_string((long long)v);
    else s += std::to_string((unsigned long long)v);
}
template <class... A> std::string args_text(const A&... a) {
    std::string s;
    (put_arg(s, a), ...);
    return s;
}
}  // namespace spmm_plan

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ...) \
    spmm_plan::log_launch(typeid(spmm_plan::KernelTag<(kernel)>), grid, block, lds_bytes, spmm_plan::args_text(__VA_ARGS__))
