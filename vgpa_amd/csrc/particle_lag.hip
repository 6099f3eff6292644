// Weighted cross moments of stored trajectories between every kept grid index and a set of anchor rows (vgpa_particle_lag_covariance,
// vgpa_path_cross_moments): with paths X [B][n][n_keep][D], weights W [B][n] and anchor rows r_q into the kept axis,
//   mean[p][k][a]        = sum_i W_i X_i(k)[a]
//   cross[p][q][k][a][b] = sum_i W_i X_i(k)[a] X_i(r_q)[b]
// a contraction over the path index i alone.  Every term is fma(X_i(k)[a], W_i X_i(r_q)[b], .): the weight goes to the anchor's side, rounded
// once, and the product into the sum unrounded.
//
// Two kernels:
//   k_path_cross_lane   D <= 4: one thread per (problem, anchor, kept row, a, b), the paths in increasing order
//   k_path_cross_mfma   5 <= D <= 64: one wave per (problem, anchor, kept row) on v_mfma_f64_16x16x4_f64 with the path index as the K
//                       dimension, four paths per product, D padded to NT = 16, 32, 48 or 64.  All MT x MT tiles (MT = NT / 16): the
//                       product is not symmetric for k != r_q.  Lane l gives A[a = l & 15][path l >> 4] = X_i(k)[16 mt + a] and
//                       B[path l >> 4][b = l & 15] = W_i X_i(r_q)[16 nt + b], and holds C[(l >> 4) + 4 r][l & 15] in r = 0..3 (the fp64
//                       accumulator map).  Rows >= D and paths >= n give zeros on both sides.  A workgroup is four waves on four
//                       consecutive kept rows of one anchor: they read the same anchor rows, which so come from HBM once per workgroup.
//                       The operands go from global memory straight to the registers the product reads -- a half wave reads 16
//                       consecutive doubles of one path, 128 bytes -- so there is no LDS and no bank to conflict on.
// Order of addition.  A wave (a thread) owns its output tile and runs over all paths of the problem in increasing order, the four paths of
// one product in the order the matrix core adds them; nothing is split over waves or workgroups, there are no atomics and no scratch.  The
// mean's four partial sums over the paths i = l >> 4 mod 4 are added in index order.  So a result does not depend on the batch, on
// n_anchor, on the other anchors or on n_keep.  The mean is written by the workgroups of anchor 0.
#include "vgpa_internal.h"
#include "dispatch.h"

namespace vgpa {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kCrossThreads = 256;
constexpr int kCrossRows = kCrossThreads / 64;      // kept rows per workgroup of the matrix-core kernel: one per wave

__global__ void __launch_bounds__(kCrossThreads) k_path_cross_lane(PathMomentArgs g) {
  const int D = g.D, DD = D * D, n = g.n_paths, n_keep = g.n_keep;
  const size_t e = (size_t)blockIdx.x * kCrossThreads + threadIdx.x;
  if (e >= (size_t)n_keep * DD) return;
  const int q = blockIdx.y, p = blockIdx.z;
  const size_t k = e / DD;
  const int ab = (int)(e - k * DD), a = ab / D, b = ab - a * D;
  const size_t row = (size_t)n_keep * D;      // one path
  const double* __restrict__ xt = g.paths + (size_t)p * n * row + k * D + a;
  const double* __restrict__ xs = g.paths + (size_t)p * n * row + (size_t)g.anchor_rows[q] * D + b;
  const double* __restrict__ W = g.weights ? g.weights + (size_t)p * n : nullptr;
  const double equal = 1.0 / (double)n;
  double acc = 0.0, m = 0.0;
  for (int i = 0; i < n; i++) {
    const double w = W ? W[i] : equal, xa = xt[(size_t)i * row];
    acc = fma(xa, w * xs[(size_t)i * row], acc);
    m = fma(w, xa, m);
  }
  g.cross[((size_t)p * g.n_anchor + q) * n_keep * DD + e] = acc;
  if (q == 0 && b == 0) g.mean[((size_t)p * n_keep + k) * D + a] = m;
}

template <int NT>
__global__ void __launch_bounds__(kCrossThreads) k_path_cross_mfma(PathMomentArgs g) {
  constexpr int MT = NT / 16;
  const int D = g.D, n = g.n_paths, n_keep = g.n_keep;
  const int lane = threadIdx.x & 63, kk = lane >> 4, j16 = lane & 15;
  const int k = (int)blockIdx.x * kCrossRows + (threadIdx.x >> 6);      // (wave-uniform)
  if (k >= n_keep) return;                                              // (no barrier below)
  const int q = blockIdx.y, p = blockIdx.z;
  const size_t row = (size_t)n_keep * D;
  const double* __restrict__ X = g.paths + (size_t)p * n * row;
  const double* __restrict__ W = g.weights ? g.weights + (size_t)p * n : nullptr;
  const size_t off_t = (size_t)k * D, off_s = (size_t)g.anchor_rows[q] * D;
  const double equal = 1.0 / (double)n;
  d4 acc[MT][MT];
  double m[MT];
#pragma unroll
  for (int mt = 0; mt < MT; mt++) {
    m[mt] = 0.0;
#pragma unroll
    for (int nt = 0; nt < MT; nt++) acc[mt][nt] = d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int i0 = 0; i0 < n; i0 += 4) {
    const int i = i0 + kk;
    const bool path = i < n;
    const double* __restrict__ xi = X + (size_t)(path ? i : 0) * row;
    const double w = path ? (W ? W[i] : equal) : 0.0;
    double av[MT], bv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
      const int c = 16 * mt + j16;
      const bool in = path && c < D;
      av[mt] = in ? xi[off_t + c] : 0.0;
      bv[mt] = in ? w * xi[off_s + c] : 0.0;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
      m[mt] = fma(w, av[mt], m[mt]);
#pragma unroll
      for (int nt = 0; nt < MT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
    }
  }
  double* __restrict__ out = g.cross + (((size_t)p * g.n_anchor + q) * n_keep + k) * D * D;
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int nt = 0; nt < MT; nt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int a = 16 * mt + 4 * r + kk, b = 16 * nt + j16;
        if (a < D && b < D) out[a * D + b] = acc[mt][nt][r];
      }
  if (q != 0) return;      // (uniform over the workgroup)
#pragma unroll
  for (int mt = 0; mt < MT; mt++) {
    const double s = ((__shfl(m[mt], j16) + __shfl(m[mt], j16 + 16)) + __shfl(m[mt], j16 + 32)) + __shfl(m[mt], j16 + 48);
    const int a = 16 * mt + j16;
    if (kk == 0 && a < D) g.mean[((size_t)p * n_keep + k) * D + a] = s;
  }
}

}  // namespace

bool path_moments_grid_fits(int D, int batch, int n_keep, int n_anchor) {
  const size_t x = D <= kMaxLaneD ? ((size_t)n_keep * D * D + kCrossThreads - 1) / kCrossThreads : ((size_t)n_keep + kCrossRows - 1) / kCrossRows;
  return x <= 2147483647u && n_anchor <= kMaxGridY && batch <= kMaxGridY;
}

hipError_t launch_path_cross_moments(const PathMomentArgs& g, hipStream_t st) {
  if (!g.paths || !g.anchor_rows || !g.mean || !g.cross || g.D < 1 || g.D > kMaxSmallD || g.batch < 1 || g.n_paths < 1 || g.n_keep < 1 || g.n_anchor < 1 ||
      !path_moments_grid_fits(g.D, g.batch, g.n_keep, g.n_anchor))
    return hipErrorInvalidValue;
  if (g.D <= kMaxLaneD) {
    const size_t x = ((size_t)g.n_keep * g.D * g.D + kCrossThreads - 1) / kCrossThreads;
    hipLaunchKernelGGL(k_path_cross_lane, dim3((unsigned)x, g.n_anchor, g.batch), dim3(kCrossThreads), 0, st, g);
    return hipGetLastError();
  }
  return with_int<1, 4>((g.D + 15) / 16, [&](auto tiles) {      // D padded to 16, 32, 48 or 64
    constexpr int NT = 16 * decltype(tiles)::value;
    hipLaunchKernelGGL(k_path_cross_mfma<NT>, dim3((unsigned)((g.n_keep + kCrossRows - 1) / kCrossRows), g.n_anchor, g.batch), dim3(kCrossThreads), 0, st, g);
    return hipGetLastError();
  });
}

}  // namespace vgpa
