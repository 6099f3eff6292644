// Device helpers the samplers (sample.hip) and the backward smoother (particle_smooth.hip) share: the Philox counters and the normals drawn
// from them, the model drifts of the lane kernels, the wave reductions, a problem's observation at a grid index.  Device code only; every
// function is internal to the translation unit that includes it.
#pragma once
#include "vgpa_internal.h"

namespace vgpa {
namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* r) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ double unit_open(uint32_t hi, uint32_t lo) {
  const double u = (((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) + 0.5) * 0x1.0p-53;
  return fmin(u, 0x1.fffffffffffffp-1);     // (2^53 - 1 + 0.5 rounds to 2^53 in fp64: the one value that would reach 1)
}

// the pair (xi_2j, xi_2j+1) of grid index k, path `path`, problem p
__device__ __forceinline__ void normal_pair(uint32_t k0, uint32_t k1, uint32_t k, uint32_t path, uint32_t p, uint32_t j, double* z0, double* z1) {
  uint32_t r[4];
  philox4x32_10(k, path, p, j, k0, k1, r);
  const double u1 = unit_open(r[0], r[1]), u2 = unit_open(r[2], r[3]);
  const double rho = sqrt(-2.0 * log(u1));
  double s, c;
  sincos(6.283185307179586 * u2, &s, &c);
  *z0 = rho * c; *z1 = rho * s;
}

// ---- D <= 4: one lane per (problem, path) -----------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void model_drift(int model, const double* th, const double* x, double* f) {
  if (model == VGPA_MODEL_OU) { f[0] = -th[0] * x[0]; }
  else if (model == VGPA_MODEL_DW) { f[0] = 4.0 * x[0] * (th[0] - x[0] * x[0]); }
  else if (model == VGPA_MODEL_L63) {
    if constexpr (D == 3) {
      f[0] = th[0] * (x[1] - x[0]);
      f[1] = (th[1] - x[2]) * x[0] - x[1];
      f[2] = x[0] * x[1] - th[2] * x[2];
    }
  } else {
#pragma unroll
    for (int i = 0; i < D; i++) f[i] = (x[(i + 1) % D] - x[(i + D - 2) % D]) * x[(i + D - 1) % D] - x[i] + th[0];
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// pf_obs_at: the problem's observation at grid index a.k, or -1
__device__ __forceinline__ int pf_obs_at(const PfArgs& a, int p) {
  const int64_t* t = a.obs_t + (size_t)p * a.obs_t_stride;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  int j = -1;
  for (int m = 0; m < cnt; m++) if (t[m] == (int64_t)a.k) j = m;
  return j;
}

// The Lorenz-96 transition mean of one candidate on its own column of an LDS tile [D][ld] (component d at col[d ld]), circular, in place
// behind three rolling registers: col[d ld] <- x_d + dt ((x_{d+1} - x_{d-2}) x_{d-1} - x_d + theta) (k_pf_backward and the backward smoother)
__device__ __forceinline__ void l96_mean_in_place(double* col, int ld, int D, double dt, double th0) {
  const double x_first = col[0];
  double om2 = col[(D - 2) * ld], om1 = col[(D - 1) * ld], cur = x_first;
  for (int d = 0; d < D; d++) {
    const double nxt = d + 1 < D ? col[(d + 1) * ld] : x_first;
    const double fd = (nxt - om2) * om1 - cur + th0;
    col[d * ld] = cur + dt * fd;
    om2 = om1; om1 = cur; cur = nxt;
  }
}

}  // namespace
}  // namespace vgpa
