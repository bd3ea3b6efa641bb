// Runtime value -> template argument, once: iod_dispatch<3, 5, 7>(k, [&](auto ks) { return launch_x<ks>(args); }) calls the
// closure with std::integral_constant<int, V> for the V equal to k, so the argument list is written once.  A value outside the
// list is an error (hipErrorInvalidValue), never a silent default, and the closure is not called.
// Included through launch.h; needs only hipError_t declared before it, so a host-only test can include it with a stand-in.
#pragma once
#include <type_traits>

template <int... Vs, class F>
inline hipError_t iod_dispatch(int v, F&& f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return e;
}
template <class F>
inline hipError_t iod_dispatch_bool(bool v, F&& f)
{
    return v ? f(std::true_type{}) : f(std::false_type{});
}
