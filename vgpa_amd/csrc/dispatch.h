// Host-side dispatch: run-time values as template arguments, and the launch that opts in to large dynamic LDS.  Every launcher in csrc/
// selects its kernel through these.  Host code only: a generic lambda handed to with_* receives the value as a
// std::integral_constant (or std::true_type / std::false_type) and reads it back with decltype(v)::value.  A combination that has no kernel
// is refused inside the lambda with `if constexpr`, so that the helper instantiates nothing the site did not instantiate by hand.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "../../include/vgpa_hip.h"

namespace vgpa {

// a run-time flag as a compile-time one: f(std::true_type) or f(std::false_type)
template <class F>
hipError_t with_flag(bool on, F f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

namespace detail {
template <int Lo, class R, class F, int... I>
R with_int_seq(int v, F& f, R miss, std::integer_sequence<int, I...>) {
  R r = miss;      // (the fold stops at the one I with Lo + I == v; none: `miss`)
  (void)(... || (v == Lo + I && ((void)(r = f(std::integral_constant<int, Lo + I>{})), true)));
  return r;
}
}  // namespace detail

// A run-time integer in [Lo, Hi] as a compile-time one: f(std::integral_constant<int, v>).  Outside the range: `miss`, and f is not called.
template <int Lo, int Hi, class F, class R = decltype(std::declval<F&>()(std::integral_constant<int, Lo>{}))>
R with_int(int v, F f, R miss = hipErrorInvalidValue) {
  static_assert(Lo <= Hi, "with_int: empty range");
  return detail::with_int_seq<Lo>(v, f, miss, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

// The stepper (VGPA_ODE_*) and the model (VGPA_MODEL_OU / DW / L63: what the lane sweep takes; a site with fewer models refuses the rest in
// its lambda, and L96 has launchers of its own) as compile-time integers.  Any other value: `miss`.
static_assert(VGPA_ODE_EULER == 0 && VGPA_ODE_HEUN == 1 && VGPA_ODE_RK2 == 2 && VGPA_ODE_RK4 == 3, "with_method: the four steppers are 0..3");
static_assert(VGPA_MODEL_OU == 0 && VGPA_MODEL_DW == 1 && VGPA_MODEL_L63 == 2, "with_model: the three lane models are 0..2");
template <class F, class R = decltype(std::declval<F&>()(std::integral_constant<int, 0>{}))>
R with_method(int method, F f, R miss = hipErrorInvalidValue) { return with_int<VGPA_ODE_EULER, VGPA_ODE_RK4>(method, f, miss); }
template <class F, class R = decltype(std::declval<F&>()(std::integral_constant<int, 0>{}))>
R with_model(int model, F f, R miss = hipErrorInvalidValue) { return with_int<VGPA_MODEL_OU, VGPA_MODEL_L63>(model, f, miss); }

// Dynamic LDS a kernel may be launched with before it has been granted more.  48 KiB is the limit HIP inherits from the CUDA programming
// model and the lowest any ROCm release has enforced (others allow 64 KiB); asking from the lower figure on is harmless, since the call is
// idempotent, and a launch above the real limit without it fails.  The device has 160 KiB per workgroup.
constexpr size_t kLdsOptInBytes = 48 * 1024;

// Launch `kern` with `lds` bytes of dynamic LDS: above kLdsOptInBytes the limit of this kernel is raised first, and a failure to raise it is
// returned without launching.  Nothing is remembered between calls: the attribute belongs to the current device, and the sharded driver and
// the vgpa_device_* entry points run on several.
template <class... KA, class... A>
hipError_t launch_lds(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
  if (lds > kLdsOptInBytes)
    if (hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, lds, st, std::forward<A>(args)...);
  return hipGetLastError();
}

}  // namespace vgpa
