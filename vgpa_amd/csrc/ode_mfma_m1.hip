// Instantiations of the symmetric fp64-MFMA stepping kernels for stepper 1: D <= 44 on the role-specialised kernels of
// ode_mfma_impl.h or the symmetric-unit ones, as OdeArgs::sym_units says, 44 < D <= 64 on the symmetric-unit kernels of
// ode_sym_impl.h.
#include "ode_sym_impl.h"
namespace vgpa {
template bool mfma_method_supported<1>(int nb);
template hipError_t mfma_method_launch<1>(bool fwd, const OdeArgs& a, int helper_roles, hipStream_t st);
}  // namespace vgpa
