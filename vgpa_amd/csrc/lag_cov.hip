// Two-time covariance of the posterior process (vgpa_lag_covariance): for an anchor s and every grid index k >= s,
//   C_s = S_s (covariance) or I (propagator),   C_{k+1} = step_k(C_k),
// step_k the context's scheme for the MEAN equation dm/dt = -A_t m applied to every column of C (b = 0; the mean branch has no quirk):
//   euler  C + (-(A_k C)) dt
//   heun   p = -(A_k C), c = -(A_{k+1} (C + p dt)):  C + h (p + c)
//   rk2    C + dt (-(A_mid (C + h (-(A_k C)))))
//   rk4    k1 = -(A_k C), k2 = -(A_mid (C + h k1)), k3 = -(A_mid (C + h k2)), k4 = -(A_{k+1} (C + dt k3)):  C + dt (k1 + 2 (k2 + k3) + k4) / 6
// with h = dt / 2 and A_mid = (A_k + A_{k+1}) / 2.  So K(k, s) = Phi(k, s) S_s is what the recursion of the library propagates, not the
// matrix exponential it approximates.
//
// Three kernels:
//   k_lag_start   the n_anchor starting matrices of every problem, [B][n_anchor][D][D], from S_t in the layout it is resident in (whole
//                 matrices, packed lower triangles, the lane path's time-major array) or the identity: copies, so that row k = s of the
//                 result is the fetched S_s bit for bit
//   k_lag_lane    D <= 4: one lane per (problem, anchor), C and A_k in registers
//   k_lag_mfma    5 <= D <= 64: one workgroup of 4 waves per (problem, anchor) on v_mfma_f64_16x16x4_f64; wave w owns the columns
//                 16 w .. 16 w + 15 of C (a wave whose columns lie beyond D only helps to stage A_t)
// A workgroup (a lane) starts at its anchor's step and reads nothing but A_t of its own problem and its own start: the result of an anchor
// does not depend on the other anchors of the call, nor on the batch around the problem.
//
// The matrix-core step.  Lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds C[(l >> 4) + 4 r][l & 15] in
// r = 0..3.  With the columns of C on the N side, register r of row tile mt of an accumulator holds row 16 mt + 4 r + (l >> 4) -- which is
// what the B operand of k-step kk = 4 mt + r wants from this lane.  So a stage's state goes from the accumulators straight into the next
// product: no LDS round trip, no lane movement.  Only A_t comes from LDS: [NT][LDA] row-major, zero beyond D, LDA = 2 mod 32 doubles (the
// 16 rows x 2 columns a half wave reads fall into 32 different bank pairs), three images: A_k and A_{k+1} alternate, A_mid is formed as
// A_{k+1} is written.  A thread carries its NPF elements of A_{k+2} in registers across the step's products (the HBM latency is behind them).
#include "vgpa_internal.h"
#include "dispatch.h"

namespace vgpa {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kLagThreads = 256;

__global__ void __launch_bounds__(kLagThreads) k_lag_start(LagStartArgs a) {
  const size_t DD = (size_t)a.D * a.D, n = (size_t)a.batch * a.n_anchor * DD;
  const size_t gid = (size_t)blockIdx.x * kLagThreads + threadIdx.x;
  if (gid >= n) return;
  const int e = (int)(gid % DD), r = e / a.D, c = e % a.D;
  const size_t pa = gid / DD;
  const int ai = (int)(pa % a.n_anchor), p = (int)(pa / a.n_anchor);
  const int s = a.anchors[ai];
  double v;
  if (a.layout == LagStartArgs::Identity) v = r == c ? 1.0 : 0.0;
  else if (a.layout == LagStartArgs::Whole) v = a.S[((size_t)p * a.Np + s) * DD + e];
  else if (a.layout == LagStartArgs::Packed) v = a.S[((size_t)p * a.Np + s) * tri_off(a.D) + tri_idx(r, c)];
  else v = a.S[((size_t)s * (tri_off(a.D) + a.D) + tri_idx(r, c)) * a.bpad + p];      // (OdeArgs::msT)
  a.start[gid] = v;
}

// ---- D <= 4 ---------------------------------------------------------------------------------------------------------------------------
// w = -(a x), the sum over k in increasing order
template <int D>
__device__ __forceinline__ void neg_prod(const double* a, const double* x, double* w) {
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      double s = a[i * D] * x[j];
#pragma unroll
      for (int k = 1; k < D; k++) s += a[i * D + k] * x[k * D + j];
      w[i * D + j] = -s;
    }
}

template <int D, int METHOD>
__global__ void __launch_bounds__(kLagThreads) k_lag_lane(LagArgs a) {
  constexpr int DD = D * D;
  const size_t gid = (size_t)blockIdx.x * kLagThreads + threadIdx.x;      // the problem fastest: a wave's lanes share their anchor
  if (gid >= (size_t)a.batch * a.n_anchor) return;
  const int p = (int)(gid % a.batch), ai = (int)(gid / a.batch);
  const int s = a.anchors[ai], Np = a.Np, stride = a.stride;
  const double dt = a.dt, h = 0.5 * a.dt;
  const double* __restrict__ Ap = a.A + (size_t)p * a.stride_x;
  const size_t pa = (size_t)p * a.n_anchor + ai;
  double* __restrict__ outp = a.out + pa * (size_t)a.n_keep * DD;
  const double* __restrict__ st = a.start + pa * DD;
  double C[DD], Ak[DD], An[DD], Am[DD], X[DD], k1[DD], k2[DD], k3[DD], k4[DD];
  const int first = (s + stride - 1) / stride;      // the first kept index at or behind the anchor
  for (int kk = 0; kk < first; kk++)
#pragma unroll
    for (int e = 0; e < DD; e++) outp[(size_t)kk * DD + e] = 0.0;
#pragma unroll
  for (int e = 0; e < DD; e++) { C[e] = st[e]; Ak[e] = Ap[(size_t)s * DD + e]; }
  if (s % stride == 0)
#pragma unroll
    for (int e = 0; e < DD; e++) outp[(size_t)(s / stride) * DD + e] = C[e];
  for (int k = s; k < Np - 1; k++) {
#pragma unroll
    for (int e = 0; e < DD; e++) { An[e] = Ap[(size_t)(k + 1) * DD + e]; Am[e] = 0.5 * (Ak[e] + An[e]); }
    neg_prod<D>(Ak, C, k1);
    if constexpr (METHOD == VGPA_ODE_EULER) {
#pragma unroll
      for (int e = 0; e < DD; e++) C[e] = C[e] + k1[e] * dt;
    } else if constexpr (METHOD == VGPA_ODE_HEUN) {
#pragma unroll
      for (int e = 0; e < DD; e++) X[e] = C[e] + k1[e] * dt;
      neg_prod<D>(An, X, k2);
#pragma unroll
      for (int e = 0; e < DD; e++) C[e] = C[e] + h * (k1[e] + k2[e]);
    } else if constexpr (METHOD == VGPA_ODE_RK2) {
#pragma unroll
      for (int e = 0; e < DD; e++) X[e] = C[e] + h * k1[e];
      neg_prod<D>(Am, X, k2);
#pragma unroll
      for (int e = 0; e < DD; e++) C[e] = C[e] + dt * k2[e];
    } else {
#pragma unroll
      for (int e = 0; e < DD; e++) X[e] = C[e] + h * k1[e];
      neg_prod<D>(Am, X, k2);
#pragma unroll
      for (int e = 0; e < DD; e++) X[e] = C[e] + h * k2[e];
      neg_prod<D>(Am, X, k3);
#pragma unroll
      for (int e = 0; e < DD; e++) X[e] = C[e] + dt * k3[e];
      neg_prod<D>(An, X, k4);
#pragma unroll
      for (int e = 0; e < DD; e++) C[e] = C[e] + dt * (k1[e] + 2.0 * (k2[e] + k3[e]) + k4[e]) / 6.0;
    }
    if ((k + 1) % stride == 0)
#pragma unroll
      for (int e = 0; e < DD; e++) outp[(size_t)((k + 1) / stride) * DD + e] = C[e];
#pragma unroll
    for (int e = 0; e < DD; e++) Ak[e] = An[e];
  }
}

// ---- 5 <= D <= 64 ---------------------------------------------------------------------------------------------------------------------
template <int NT> struct LagShape {
  static constexpr int LDA = NT <= 32 ? 34 : 66;
  static constexpr int MT = NT / 16, KT = NT / 4;
  static constexpr int NPF = (NT * NT + kLagThreads - 1) / kLagThreads;
  static constexpr size_t lds_bytes = (size_t)3 * NT * LDA * sizeof(double);
};

// w = As x over the padded NT x 16 slice: x in the accumulator layout, which is the B operand's (see the head of the file)
template <int NT>
__device__ __forceinline__ void lag_prod(const double* __restrict__ As, int q, int j16, const d4 (&x)[LagShape<NT>::MT], d4 (&w)[LagShape<NT>::MT]) {
  using G = LagShape<NT>;
#pragma unroll
  for (int mt = 0; mt < G::MT; mt++) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    const double* ar = As + (mt * 16 + j16) * G::LDA + q;
#pragma unroll
    for (int kk = 0; kk < G::KT; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[4 * kk], x[kk >> 2][kk & 3], acc, 0, 0, 0);
    w[mt] = acc;
  }
}

template <int NT, int METHOD>
__global__ void __launch_bounds__(kLagThreads) k_lag_mfma(LagArgs a) {
  using G = LagShape<NT>;
  constexpr int LDA = G::LDA, MT = G::MT, NPF = G::NPF;
  extern __shared__ double lag_lds[];
  double* Acur = lag_lds;
  double* Anxt = lag_lds + NT * LDA;
  double* const Amid = lag_lds + 2 * NT * LDA;
  const int D = a.D, DD = D * D, Np = a.Np, stride = a.stride;
  // the problem fastest: consecutive workgroups go to consecutive XCDs, so with the anchor fastest and 8 anchors every workgroup of one
  // anchor -- one length of recursion -- lands on one XCD and the call takes as long as 8 times its longest anchor (measured: 93 ms for
  // 8 spread anchors, the time of 8 anchors at 0).  This way every XCD sees every anchor, the longest recursions first
  const int p = (int)(blockIdx.x % (unsigned)a.batch), ai = (int)(blockIdx.x / (unsigned)a.batch);
  const int s = a.anchors[ai];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j16 = lane & 15;
  const int col = wave * 16 + j16;
  const bool active = wave * 16 < D;      // wave-uniform
  const double dt = a.dt, h = 0.5 * a.dt;
  const double* __restrict__ Ap = a.A + (size_t)p * a.stride_x;
  const size_t pa = (size_t)p * a.n_anchor + ai;
  double* __restrict__ outp = a.out + pa * (size_t)a.n_keep * DD;
  const double* __restrict__ st = a.start + pa * DD;

  // this thread's elements of an A_t image: e = tid + 256 i -> (row, column) = (e / NT, e % NT); zero beyond D
  double pf[NPF];
  auto fetch = [&](int k) {
    const double* __restrict__ At = Ap + (size_t)k * DD;
#pragma unroll
    for (int i = 0; i < NPF; i++) {
      const int e = tid + kLagThreads * i, r = e / NT, c = e % NT;
      pf[i] = (r < D && c < D) ? At[r * D + c] : 0.0;      // (r < D implies e < NT * NT)
    }
  };
  // one kept row: the D x 16 slice of this wave
  auto store = [&](int k, const d4 (&c)[MT]) {
    double* __restrict__ o = outp + (size_t)(k / stride) * DD;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + 4 * r + q;
        if (row < D && col < D) o[row * D + col] = c[mt][r];
      }
  };

  // the kept rows before the anchor
  const int first = (s + stride - 1) / stride;
  for (size_t e = tid; e < (size_t)first * DD; e += kLagThreads) outp[e] = 0.0;

  d4 C[MT];
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = mt * 16 + 4 * r + q;
      C[mt][r] = (row < D && col < D) ? st[row * D + col] : 0.0;
    }
  if (active && s % stride == 0) store(s, C);

  fetch(s);
#pragma unroll
  for (int i = 0; i < NPF; i++) {
    const int e = tid + kLagThreads * i, r = e / NT, c = e % NT;
    if (e < NT * NT) Acur[r * LDA + c] = pf[i];
  }
  if (s + 1 < Np) fetch(s + 1);

  for (int k = s; k < Np - 1; k++) {
    // A_{k+1} and A_mid beside the A_k this thread wrote itself: no barrier between the two
#pragma unroll
    for (int i = 0; i < NPF; i++) {
      const int e = tid + kLagThreads * i, r = e / NT, c = e % NT;
      if (e < NT * NT) {
        Anxt[r * LDA + c] = pf[i];
        if constexpr (METHOD == VGPA_ODE_RK2 || METHOD == VGPA_ODE_RK4) Amid[r * LDA + c] = 0.5 * (Acur[r * LDA + c] + pf[i]);
      }
    }
    __syncthreads();
    if (k + 2 < Np) fetch(k + 2);
    if (active) {
      d4 X[MT], k1[MT], k2[MT];
      lag_prod<NT>(Acur, q, j16, C, k1);
      if constexpr (METHOD == VGPA_ODE_EULER) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) C[mt] = C[mt] + (-k1[mt]) * dt;
      } else if constexpr (METHOD == VGPA_ODE_HEUN) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) X[mt] = C[mt] + (-k1[mt]) * dt;
        lag_prod<NT>(Anxt, q, j16, X, k2);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) C[mt] = C[mt] + h * ((-k1[mt]) + (-k2[mt]));
      } else if constexpr (METHOD == VGPA_ODE_RK2) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) X[mt] = C[mt] + h * (-k1[mt]);
        lag_prod<NT>(Amid, q, j16, X, k2);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) C[mt] = C[mt] + dt * (-k2[mt]);
      } else {
        d4 acc[MT];      // k1 + 2 (k2 + k3) + k4 of the negated products, built as the stages arrive
#pragma unroll
        for (int mt = 0; mt < MT; mt++) X[mt] = C[mt] + h * (-k1[mt]);
        lag_prod<NT>(Amid, q, j16, X, k2);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) X[mt] = C[mt] + h * (-k2[mt]);
        lag_prod<NT>(Amid, q, j16, X, acc);      // k3
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
          X[mt] = C[mt] + dt * (-acc[mt]);
          acc[mt] = (-k1[mt]) + 2.0 * ((-k2[mt]) + (-acc[mt]));
        }
        lag_prod<NT>(Anxt, q, j16, X, k2);       // k4
#pragma unroll
        for (int mt = 0; mt < MT; mt++) C[mt] = C[mt] + dt * (acc[mt] + (-k2[mt])) / 6.0;
      }
      if ((k + 1) % stride == 0) store(k + 1, C);
    }
    __syncthreads();      // every wave is done with A_k: the next step writes A_{k+2} over it
    double* t = Acur; Acur = Anxt; Anxt = t;
  }
}

}  // namespace

bool lag_grid_fits(int D, int batch, int n_anchor) {
  const size_t n = (size_t)batch * n_anchor;
  return (D <= kMaxLaneD ? (n + kLagThreads - 1) / kLagThreads : n) <= 2147483647u;
}

hipError_t launch_lag_start(const LagStartArgs& a, hipStream_t st) {
  if (!a.start || !a.anchors || (a.layout != LagStartArgs::Identity && !a.S) || a.D < 1 || a.batch < 1 || a.n_anchor < 1) return hipErrorInvalidValue;
  const size_t n = (size_t)a.batch * a.n_anchor * a.D * a.D, blocks = (n + kLagThreads - 1) / kLagThreads;
  if (blocks > 2147483647u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lag_start, dim3((unsigned)blocks), dim3(kLagThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_lag(const LagArgs& a, hipStream_t st) {
  if (!a.A || !a.start || !a.anchors || !a.out || a.D < 1 || a.D > kMaxSmallD || a.Np < 1 || a.batch < 1 || a.n_anchor < 1 || a.stride < 1 ||
      a.n_keep != (a.Np - 1) / a.stride + 1 || !lag_grid_fits(a.D, a.batch, a.n_anchor))
    return hipErrorInvalidValue;
  const size_t n = (size_t)a.batch * a.n_anchor;
  return with_method(a.method, [&](auto m) {
    constexpr int METHOD = decltype(m)::value;
    if (a.D <= kMaxLaneD)      // one lane per anchor
      return with_int<1, kMaxLaneD>(a.D, [&](auto d) {
        hipLaunchKernelGGL((k_lag_lane<decltype(d)::value, METHOD>), dim3((unsigned)((n + kLagThreads - 1) / kLagThreads)), dim3(kLagThreads), 0, st, a);
        return hipGetLastError();
      });
    return with_int<1, 4>((a.D + 15) / 16, [&](auto tiles) {      // one workgroup per anchor, D padded to 16, 32, 48 or 64
      constexpr int NT = 16 * decltype(tiles)::value;
      return launch_lds(k_lag_mfma<NT, METHOD>, dim3((unsigned)n), dim3(kLagThreads), LagShape<NT>::lds_bytes, st, a);
    });
  });
}

}  // namespace vgpa
