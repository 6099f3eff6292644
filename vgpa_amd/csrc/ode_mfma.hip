// Dispatcher of the symmetric fp64-MFMA stepping kernels (kernels: ode_mfma_impl.h, one TU per stepper).
#include "ode_mfma_impl.h"

namespace vgpa {

bool ode_mfma_supported(int method, bool, int D) {
  if (D < 1) return false;
  const int nb = (D + 3) / 4;
  if (nb > sym::kMaxNB) return false;   // D <= 64
  return with_method(method, [&](auto m) { return mfma_method_supported<decltype(m)::value>(nb); }, false);
}

bool sym_stores_q(int method, int D) { return sym::stores_q(method, D); }
bool sym_fuses_grad(int method, int D) { return sym::fuses_grad(method, D); }

hipError_t launch_ode_mfma(int method, bool fwd, const OdeArgs& a, int helper_roles, hipStream_t st) {
  return with_method(method, [&](auto m) { return mfma_method_launch<decltype(m)::value>(fwd, a, helper_roles, st); });
}

}  // namespace vgpa
