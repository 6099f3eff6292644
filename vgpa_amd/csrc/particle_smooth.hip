// The marginal backward smoother (vgpa_particle_backward_moments): the smoothing weights of every stretch from all n
// particles of the cloud behind it, the expectation of the draw k_pf_backward (sample.hip) makes.  With the filter's histories of problem p
// -- clouds_j, anc_j, hlw_j, the flags -- and W^{j+1} the weights of stretch j + 1, at a cut j whose cloud was resampled (k = t_j):
//   x~_s    = (z + dt (b_k - A_k z)) + R_dd xi, z = clouds_j[anc_j[s]], xi the sampler's normals of counter (k + 1, s, p, .): slot s's
//             state one step behind the cut, in plain fp64 as k_pf_backward forms it
//   b_{s,i} = hlw_j[i] - 1/2 sum_d ((x~_{s,d} - mu_{i,d}) (1 / R_dd))^2, mu_i = clouds_j[i] + dt f(clouds_j[i]; theta_p)
//   P_{s,i} = exp(b_{s,i} - max_i b_{s,i}) / sum_i exp(b_{s,i} - max_i b_{s,i})
//   W^j_i   = sum_s W^{j+1}_s P_{s,i}
// and W^j = W^{j+1} where the cloud was carried on.  The host walks the union of the batch's cuts backwards; at grid index k every problem
// looks up its own observation there (none: nothing to do) and decides from its own flag whether it copies or recurses.
//
// The kernels, the problem in grid.x (D <= 4: k_ps_rows and k_ps_columns; Lorenz-96 with D >= 5: k_ps_centre and the two _mfma kernels,
// the same passes with the scores' cross term on the fp64 matrix cores, described where they stand):
//   k_ps_successors  one thread per (slot, component): x~ [B][n][D]
//   k_ps_rows<DC>    workgroup (p, blk) owns kSmoothRowBlock successors and streams the n candidates through LDS 256 at a time with
//                    k_pf_backward's tile -- 256 D consecutive doubles loaded in that order, written component-major with a row stride of
//                    257 doubles, a thread's own column read without conflict --; thread t owns candidate base + t, forms its transition mean
//                    once per tile (DC = 1, 3: model_drift<DC> in registers; DC = 0: Lorenz-96 of any D in place on the column) and the
//                    block's scores side by side, and keeps a running (max, sum of exp(b - max)) per successor: one exp per score.  The 256
//                    pairs of a successor are merged by a butterfly over the wave and in wave order through LDS.  Writes rmax, rsum [B][n]
//   k_ps_columns<DC> workgroup (p, blk) owns kSmoothColBlock = 64 candidates, one per lane, all four waves the same ones: the transition
//                    means once (registers, or the columns of an LDS tile [D][65]), then the n successors through LDS 64 at a time, x~ and
//                    c_s = W^{j+1}_s / rsum_s and rmax_s read at wave-uniform addresses.  Wave w takes the successors 16 w .. 16 w + 15 of
//                    every tile, eight scores side by side, and adds c_s exp(b_{s,i} - rmax_s) in increasing s; the four waves' sums are
//                    added as (w0 + w1) + (w2 + w3).  Writes row j of the table and the workgroup's sum of W^2 in a fixed order.  Where the
//                    cloud was carried on it copies row j + 1
//   k_ps_ess         one thread per problem: less[j] = 1 / (the workgroups' sums of W^2 in block order), less[j + 1] at a carried cut
// No atomics and no order that depends on the launch: a weight is the sum of n terms in an order n alone fixes, so two calls give the same
// bits and a problem's rows do not depend on the batch around it.
// Up to D = 4 the scores are differences on the vector ALU; from D = 5 on they are (|a|^2 + |m|^2) - 2 <a, m> with the cross term on the
// matrix cores, the form tests/test_particle_backward_moments_cpu.py::test_gram_form_holds_the_bound holds to the rounding bound.
#include "vgpa_internal.h"
#include "dispatch.h"
#include "pf_device.h"

namespace vgpa {
namespace {

constexpr int kRowTile = 256, kRowLd = kRowTile + 1;      // candidates per LDS tile of the row pass, its row stride in doubles
constexpr int kColTile = 64, kColLd = kColTile + 1;       // successors per LDS tile of the column pass (16 per wave); the stride of the means' tile

struct Cut {      // what a workgroup of problem p finds at grid index f.k
  int j;                   // the problem's observation there, or -1
  bool resampled;
  size_t hj;               // its row of the histories
};
__device__ __forceinline__ Cut cut_of(const PfArgs& f, uint32_t p) {
  Cut c;
  c.j = pf_obs_at(f, (int)p);
  c.hj = (size_t)p * f.M + (c.j < 0 ? 0 : c.j);
  c.resampled = c.j >= 0 && f.h_flag[c.hj] != 0;
  return c;
}

__global__ __launch_bounds__(256) void k_ps_successors(PfArgs f, SampleArgs a, SmoothArgs sm) {
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (!c.resampled) return;      // (uniform over the workgroup)
  const int n = f.n_paths, D = a.D, k = f.k;
  const size_t e = (size_t)blockIdx.y * 256 + threadIdx.x;
  if (e >= (size_t)n * D) return;
  const uint32_t s = (uint32_t)(e / D);
  const int d = (int)(e - (size_t)s * D);
  const uint32_t k0 = (uint32_t)(f.seed & 0xffffffffu), k1 = (uint32_t)(f.seed >> 32);
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const double* Ak = a.A + (size_t)p * a.stride_x + (size_t)k * D * D;
  const double* bk = a.b + (size_t)p * a.stride_x + (size_t)k * D;
  const double* z = f.h_clouds + (c.hj * n + (size_t)f.h_anc[c.hj * n + s]) * D;
  double sum = 0.0, z0, z1;
  for (int q = 0; q < D; q++) sum += Ak[d * D + q] * z[q];
  normal_pair(k0, k1, (uint32_t)k + 1u, s, p, (uint32_t)(d >> 1), &z0, &z1);
  sm.xt[(size_t)p * n * D + e] = (z[d] + a.dt * (bk[d] - sum)) + Rp[d * D + d] * ((d & 1) ? z1 : z0);
}

// (m, s) <- the pair of the union of two sets of scores, s = sum of exp(b - m) over the set, m its maximum; an empty set is (-inf, 0)
__device__ __forceinline__ void merge_pairs(double& m, double& s, double om, double os) {
  const double top = fmax(m, om);
  const double a = m == -INFINITY ? 0.0 : s * exp(m - top), b = om == -INFINITY ? 0.0 : os * exp(om - top);
  m = top; s = a + b;
}

template <int DC>
__global__ __launch_bounds__(256) void k_ps_rows(PfArgs f, SampleArgs a, SmoothArgs sm) {
  constexpr int TS = kSmoothRowBlock, LD = kRowLd;
  extern __shared__ double lds[];
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (!c.resampled) return;      // (uniform over the workgroup)
  const int D = DC > 0 ? DC : a.D;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = f.n_paths;
  double* tile = lds;                          // [D][LD]
  double* xt = tile + (size_t)D * LD;          // [TS][D]
  double* ir = xt + TS * D;                    // [D] 1 / R_dd
  double* wm = ir + D;                         // [4 waves][TS]
  double* ws = wm + 4 * TS;                    // [4 waves][TS]
  const double* Rp = a.R + (size_t)p * a.R_stride;
  double th[kMaxTheta];
#pragma unroll
  for (int i = 0; i < kMaxTheta; i++) th[i] = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta + i] : a.theta[i];
  const int s0 = blockIdx.y * TS;
  const double* cloud = f.h_clouds + c.hj * n * D;
  const double* hlw = f.h_lw + c.hj * n;
  const double* xsrc = sm.xt + (size_t)p * n * D;
  for (int e = tid; e < TS * D; e += 256) {      // (a successor behind the last one is the last one again and stores nothing)
    const int ss = e / D, s = s0 + ss < n ? s0 + ss : n - 1;
    xt[e] = xsrc[(size_t)s * D + (e - ss * D)];
  }
  if (tid < D) ir[tid] = 1.0 / Rp[tid * D + tid];
  double m[TS], sum[TS];
#pragma unroll
  for (int ss = 0; ss < TS; ss++) { m[ss] = -INFINITY; sum[ss] = 0.0; }
  for (int base = 0; base < n; base += kRowTile) {
    __syncthreads();      // (x~ is written; the columns of the tile before have been read)
    const int nt = n - base < kRowTile ? n - base : kRowTile;
    const double* src = cloud + (size_t)base * D;
    for (int e = tid; e < nt * D; e += 256) { const int cnd = e / D; tile[(e - cnd * D) * LD + cnd] = src[e]; }
    __syncthreads();
    const int i = base + tid;
    const bool mine = i < n;
    double* col = tile + tid;
    double mu[DC > 0 ? DC : 1];
    if constexpr (DC > 0) {
      double xc[DC], fc[DC];
#pragma unroll
      for (int d = 0; d < DC; d++) xc[d] = mine ? col[d * LD] : 0.0;      // (a lane behind the last candidate: no stale LDS into the drift)
      model_drift<DC>(a.model, th, xc, fc);
#pragma unroll
      for (int d = 0; d < DC; d++) mu[d] = xc[d] + a.dt * fc[d];
    } else if (mine) {
      l96_mean_in_place(col, LD, D, a.dt, th[0]);
    }
    if (!mine) continue;      // (no barrier below in this pass; the next pass begins with one every thread reaches)
    double acc[TS];
#pragma unroll
    for (int ss = 0; ss < TS; ss++) acc[ss] = 0.0;
    for (int d = 0; d < D; d++) {
      double md;
      if constexpr (DC > 0) md = mu[d]; else md = col[d * LD];
      const double ird = ir[d];
#pragma unroll
      for (int ss = 0; ss < TS; ss++) { const double v = (xt[ss * D + d] - md) * ird; acc[ss] += v * v; }
    }
    const double lwi = hlw[i];
#pragma unroll
    for (int ss = 0; ss < TS; ss++) {
      const double b = lwi - 0.5 * acc[ss];
      if (b != -INFINITY) {      // (a candidate of weight zero adds nothing; a NaN goes through)
        const double e = exp(-fabs(b - m[ss]));
        if (b > m[ss]) { sum[ss] = sum[ss] * e + 1.0; m[ss] = b; } else sum[ss] += e;
      }
    }
  }
#pragma unroll
  for (int ss = 0; ss < TS; ss++) {
    double mv = m[ss], sv = sum[ss];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double om = __shfl_xor(mv, o), os = __shfl_xor(sv, o);
      merge_pairs(mv, sv, om, os);
    }
    if (lane == 0) { wm[w * TS + ss] = mv; ws[w * TS + ss] = sv; }
  }
  __syncthreads();
  if (tid < TS && s0 + tid < n) {
    double mv = wm[tid], sv = ws[tid];
    for (int q = 1; q < 4; q++) merge_pairs(mv, sv, wm[q * TS + tid], ws[q * TS + tid]);
    sm.rmax[(size_t)p * n + s0 + tid] = mv;
    sm.rsum[(size_t)p * n + s0 + tid] = sv;
  }
}

template <int DC>
__global__ __launch_bounds__(256) void k_ps_columns(PfArgs f, SampleArgs a, SmoothArgs sm) {
  constexpr int CB = kSmoothColBlock, ST = kColTile, LD = kColLd, G = 8;
  static_assert(CB == 64 && ST == 64, "one candidate per lane, 16 successors of a tile per wave");
  extern __shared__ double lds[];
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (c.j < 0) return;      // (uniform over the workgroup)
  const int D = DC > 0 ? DC : a.D;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = f.n_paths;
  const int i = blockIdx.y * CB + lane;
  const bool mine = i < n;
  double* row = sm.wtab + ((size_t)p * sm.rows + c.j) * n;
  const double* next = row + n;
  if (!c.resampled) {      // the cloud was carried on: the weights of the stretch behind it
    if (w == 0 && mine) row[i] = next[i];
    return;
  }
  double* mut = lds;                           // [D][LD] the candidates' transition means
  double* xs = mut + (size_t)D * LD;           // [ST][D]
  double* cf = xs + ST * D;                    // [ST] W^{j+1}_s / rsum_s
  double* mx = cf + ST;                        // [ST] rmax_s
  double* ir = mx + ST;                        // [D]
  double* red = ir + D;                        // [4 waves][CB]
  const double* Rp = a.R + (size_t)p * a.R_stride;
  double th[kMaxTheta];
#pragma unroll
  for (int q = 0; q < kMaxTheta; q++) th[q] = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta + q] : a.theta[q];
  const double* hlw = f.h_lw + c.hj * n;
  const double* xsrc = sm.xt + (size_t)p * n * D;
  const double* rmax = sm.rmax + (size_t)p * n;
  const double* rsum = sm.rsum + (size_t)p * n;
  {
    const int i0 = blockIdx.y * CB, nt = n - i0 < CB ? n - i0 : CB;
    const double* src = f.h_clouds + (c.hj * n + (size_t)i0) * D;
    for (int e = tid; e < CB * D; e += 256) { const int cnd = e / D; mut[(e - cnd * D) * LD + cnd] = e < nt * D ? src[e] : 0.0; }
  }
  if (tid < D) ir[tid] = 1.0 / Rp[tid * D + tid];
  __syncthreads();
  double* col = mut + lane;
  double mu[DC > 0 ? DC : 1];
  if constexpr (DC > 0) {
    double xc[DC], fc[DC];
#pragma unroll
    for (int d = 0; d < DC; d++) xc[d] = col[d * LD];
    model_drift<DC>(a.model, th, xc, fc);
#pragma unroll
    for (int d = 0; d < DC; d++) mu[d] = xc[d] + a.dt * fc[d];
  } else {
    if (w == 0) l96_mean_in_place(col, LD, D, a.dt, th[0]);
  }
  const double lwi = mine ? hlw[i] : 0.0;
  double acc = 0.0;
  for (int sb = 0; sb < n; sb += ST) {
    __syncthreads();      // (the means are written; the tile before has been read)
    const int nt = n - sb < ST ? n - sb : ST;
    for (int e = tid; e < ST * D; e += 256) xs[e] = e < nt * D ? xsrc[(size_t)sb * D + e] : 0.0;
    if (tid < ST) {
      const bool in = tid < nt;
      cf[tid] = in ? next[sb + tid] / rsum[sb + tid] : 0.0;
      mx[tid] = in ? rmax[sb + tid] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < ST / 4; g += G) {
      const int u0 = w * (ST / 4) + g;      // (wave-uniform)
      if (u0 >= nt) break;
      double q[G];
#pragma unroll
      for (int u = 0; u < G; u++) q[u] = 0.0;
      for (int d = 0; d < D; d++) {
        double md;
        if constexpr (DC > 0) md = mu[d]; else md = col[d * LD];
        const double ird = ir[d];
#pragma unroll
        for (int u = 0; u < G; u++) { const double v = (xs[(u0 + u) * D + d] - md) * ird; q[u] += v * v; }
      }
#pragma unroll
      for (int u = 0; u < G; u++) {
        const double b = lwi - 0.5 * q[u];
        if (u0 + u < nt) acc += cf[u0 + u] * exp(b - mx[u0 + u]);      // (a successor behind the last one adds nothing)
      }
    }
  }
  red[w * CB + lane] = acc;
  __syncthreads();
  if (w != 0) return;
  const double wi = mine ? (red[lane] + red[CB + lane]) + (red[2 * CB + lane] + red[3 * CB + lane]) : 0.0;
  if (mine) row[i] = wi;
  const double s2 = wave_sum(wi * wi);
  if (lane == 0) sm.part[((size_t)p * sm.rows + c.j) * gridDim.y + blockIdx.y] = s2;
}

// ---- D >= 5 (Lorenz-96): the cross term of the scores on the fp64 matrix cores ---------------------------------------------------------------
// With c the mean of the cut's cloud (k_ps_centre), a_s = (x~_s - c) (1 / R) and m_i = (mu_i - c) (1 / R), component by component,
//   q_{s,i} = sum_d ((x~_{s,d} - mu_{i,d}) (1 / R_dd))^2 = (|a_s|^2 + |m_i|^2) - 2 <a_s, m_i>
// and <a_s, m_i> is a 16 x 16 x 4 product of v_mfma_f64_16x16x4_f64 per four components: the successors are the rows, the candidates the
// columns, D padded with zeros to DP = 16 NT.  Lane l gives A[s = l & 15][d = 4 kc + (l >> 4)] and B[d = 4 kc + (l >> 4)][i = l & 15] and holds
// C[s = (l >> 4) + 4 r][i = l & 15] in r = 0..3.  Centred and scaled, the three terms are of the size of the cloud's squared radius in
// transition widths, which the rounding bound of the scores covers on every case the tests run.
typedef double d4 __attribute__((ext_vector_type(4)));

// centre [B][kMaxSmallD]: the mean of the cut's cloud, component by component, the particles added in an order n and D fix
__global__ __launch_bounds__(256) void k_ps_centre(PfArgs f, SmoothArgs sm) {
  __shared__ double part[256];
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (!c.resampled) return;      // (uniform over the workgroup)
  const int n = f.n_paths, D = f.D, tid = threadIdx.x, G = 256 / D, g = tid / D, d = tid - g * D;
  const double* cloud = f.h_clouds + c.hj * n * D;
  double s = 0.0;
  if (g < G)
    for (int i = g; i < n; i += G) s += cloud[(size_t)i * D + d];
  part[tid] = s;
  __syncthreads();
  if (tid < D) {
    double t = 0.0;
    for (int v = 0; v < G; v++) t += part[v * D + tid];
    sm.centre[(size_t)p * kMaxSmallD + tid] = t / (double)n;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void k_ps_rows_mfma(PfArgs f, SampleArgs a, SmoothArgs sm) {
  constexpr int TS = kSmoothRowBlock, LD = kRowLd, DP = 16 * NT, NK = 4 * NT, XS = DP + 1;
  static_assert(TS == 16, "the successors of a workgroup are the 16 rows of the product");
  extern __shared__ double lds[];
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (!c.resampled) return;      // (uniform over the workgroup)
  const int D = a.D, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = f.n_paths, j16 = lane & 15, kk = lane >> 4;
  double* tile = lds;                          // [DP][LD]: rows >= D stay zero
  double* at = tile + (size_t)DP * LD;         // [TS][XS] a_s, zero behind D
  double* ir = at + TS * XS;                   // [DP]
  double* cen = ir + DP;                       // [DP]
  double* na = cen + DP;                       // [TS] |a_s|^2
  double* nrm = na + TS;                       // [kRowTile] |m_i|^2 of the tile's candidates
  double* wm = nrm + kRowTile;                 // [4 waves][TS]
  double* ws = wm + 4 * TS;                    // [4 waves][TS]
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const double th0 = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta] : a.theta[0];
  const int s0 = blockIdx.y * TS;
  const double* cloud = f.h_clouds + c.hj * n * D;
  const double* hlw = f.h_lw + c.hj * n;
  const double* xsrc = sm.xt + (size_t)p * n * D;
  if (tid < DP) {
    ir[tid] = tid < D ? 1.0 / Rp[tid * D + tid] : 0.0;
    cen[tid] = tid < D ? sm.centre[(size_t)p * kMaxSmallD + tid] : 0.0;
  }
  for (int e = tid; e < (DP - D) * LD; e += 256) tile[(size_t)D * LD + e] = 0.0;
  __syncthreads();
  for (int e = tid; e < TS * DP; e += 256) {      // (a successor behind the last one is the last one again and stores nothing)
    const int ss = e / DP, d = e - ss * DP, s = s0 + ss < n ? s0 + ss : n - 1;
    at[ss * XS + d] = d < D ? (xsrc[(size_t)s * D + d] - cen[d]) * ir[d] : 0.0;
  }
  __syncthreads();
  if (tid < TS) {
    double t = 0.0;
    for (int d = 0; d < D; d++) { const double v = at[tid * XS + d]; t += v * v; }
    na[tid] = t;
  }
  double areg[NK];
#pragma unroll
  for (int kc = 0; kc < NK; kc++) areg[kc] = at[j16 * XS + 4 * kc + kk];
  double m[4], sum[4];
#pragma unroll
  for (int r = 0; r < 4; r++) { m[r] = -INFINITY; sum[r] = 0.0; }
  for (int base = 0; base < n; base += kRowTile) {
    __syncthreads();      // (na is written; the columns of the tile before have been read)
    const int nt = n - base < kRowTile ? n - base : kRowTile;
    const double* src = cloud + (size_t)base * D;
    for (int e = tid; e < nt * D; e += 256) { const int cnd = e / D; tile[(e - cnd * D) * LD + cnd] = src[e]; }
    __syncthreads();
    if (tid < nt) {
      double* col = tile + tid;
      l96_mean_in_place(col, LD, D, a.dt, th0);
      double t = 0.0;
      for (int d = 0; d < D; d++) { const double v = (col[d * LD] - cen[d]) * ir[d]; col[d * LD] = v; t += v * v; }
      nrm[tid] = t;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int first = w * 64 + q * 16;      // (wave-uniform)
      if (first >= nt) break;
      const int cl = first + j16, i = base + cl;
      d4 C = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kc = 0; kc < NK; kc++) C = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[kc], tile[(4 * kc + kk) * LD + cl], C, 0, 0, 0);
      if (cl < nt) {
        const double lwi = hlw[i], nmi = nrm[cl];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double b = lwi - 0.5 * ((na[kk + 4 * r] + nmi) - 2.0 * C[r]);
          if (b != -INFINITY) {
            const double e = exp(-fabs(b - m[r]));
            if (b > m[r]) { sum[r] = sum[r] * e + 1.0; m[r] = b; } else sum[r] += e;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    double mv = m[r], sv = sum[r];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {      // the 16 lanes of a successor
      const double om = __shfl_xor(mv, o), os = __shfl_xor(sv, o);
      merge_pairs(mv, sv, om, os);
    }
    if (j16 == 0) { wm[w * TS + kk + 4 * r] = mv; ws[w * TS + kk + 4 * r] = sv; }
  }
  __syncthreads();
  if (tid < TS && s0 + tid < n) {
    double mv = wm[tid], sv = ws[tid];
    for (int q = 1; q < 4; q++) merge_pairs(mv, sv, wm[q * TS + tid], ws[q * TS + tid]);
    sm.rmax[(size_t)p * n + s0 + tid] = mv;
    sm.rsum[(size_t)p * n + s0 + tid] = sv;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void k_ps_columns_mfma(PfArgs f, SampleArgs a, SmoothArgs sm) {
  constexpr int CB = kSmoothColBlock, ST = kColTile, LD = kColLd, DP = 16 * NT, NK = 4 * NT, XS = DP + 1;
  static_assert(CB == 64 && ST == 64, "four column tiles of 16 candidates, 16 successors of a tile per wave");
  extern __shared__ double lds[];
  const uint32_t p = blockIdx.x;
  const Cut c = cut_of(f, p);
  if (c.j < 0) return;      // (uniform over the workgroup)
  const int D = a.D, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = f.n_paths, j16 = lane & 15, kk = lane >> 4;
  const int i0 = blockIdx.y * CB;
  double* row = sm.wtab + ((size_t)p * sm.rows + c.j) * n;
  const double* next = row + n;
  if (!c.resampled) {      // the cloud was carried on: the weights of the stretch behind it
    if (w == 0 && i0 + lane < n) row[i0 + lane] = next[i0 + lane];
    return;
  }
  double* mut = lds;                           // [DP][LD] m_i, zero behind D
  double* xs = mut + (size_t)DP * LD;          // [ST][XS] a_s of the tile, zero behind D and behind the last successor
  double* cf = xs + ST * XS;                   // [ST] W^{j+1}_s / rsum_s
  double* mx = cf + ST;                        // [ST] rmax_s
  double* nas = mx + ST;                       // [ST] |a_s|^2
  double* ir = nas + ST;                       // [DP]
  double* cen = ir + DP;                       // [DP]
  double* nrm = cen + DP;                      // [CB] |m_i|^2
  double* red = nrm + CB;                      // [4 waves][CB]
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const double th0 = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta] : a.theta[0];
  const double* hlw = f.h_lw + c.hj * n;
  const double* xsrc = sm.xt + (size_t)p * n * D;
  const double* rmax = sm.rmax + (size_t)p * n;
  const double* rsum = sm.rsum + (size_t)p * n;
  if (tid < DP) {
    ir[tid] = tid < D ? 1.0 / Rp[tid * D + tid] : 0.0;
    cen[tid] = tid < D ? sm.centre[(size_t)p * kMaxSmallD + tid] : 0.0;
  }
  {
    const int nt = n - i0 < CB ? n - i0 : CB;
    const double* src = f.h_clouds + (c.hj * n + (size_t)i0) * D;
    for (int e = tid; e < CB * D; e += 256) { const int cnd = e / D; mut[(e - cnd * D) * LD + cnd] = e < nt * D ? src[e] : 0.0; }
    for (int e = tid; e < (DP - D) * LD; e += 256) mut[(size_t)D * LD + e] = 0.0;
  }
  __syncthreads();
  if (w == 0) {
    double* col = mut + lane;
    l96_mean_in_place(col, LD, D, a.dt, th0);
    double t = 0.0;
    for (int d = 0; d < D; d++) { const double v = (col[d * LD] - cen[d]) * ir[d]; col[d * LD] = v; t += v * v; }
    nrm[lane] = t;
  }
  __syncthreads();
  double lw[4], nm[4], acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = i0 + 16 * q + j16;
    lw[q] = i < n ? hlw[i] : 0.0; nm[q] = nrm[16 * q + j16]; acc[q] = 0.0;
  }
  for (int sb = 0; sb < n; sb += ST) {
    __syncthreads();      // (the tile before has been read)
    const int nt = n - sb < ST ? n - sb : ST;
    for (int e = tid; e < ST * DP; e += 256) {
      const int ss = e / DP, d = e - ss * DP;
      xs[ss * XS + d] = ss < nt && d < D ? (xsrc[(size_t)(sb + ss) * D + d] - cen[d]) * ir[d] : 0.0;
    }
    if (tid < ST) {
      const bool in = tid < nt;
      cf[tid] = in ? next[sb + tid] / rsum[sb + tid] : 0.0;
      mx[tid] = in ? rmax[sb + tid] : 0.0;
    }
    __syncthreads();
    if (tid < ST) {
      double t = 0.0;
      for (int d = 0; d < D; d++) { const double v = xs[tid * XS + d]; t += v * v; }
      nas[tid] = t;
    }
    __syncthreads();
    if (16 * w >= nt) continue;      // (wave-uniform; the next pass begins with a barrier every wave reaches)
    double areg[NK];
#pragma unroll
    for (int kc = 0; kc < NK; kc++) areg[kc] = xs[(16 * w + j16) * XS + 4 * kc + kk];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      d4 C = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kc = 0; kc < NK; kc++) C = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[kc], mut[(4 * kc + kk) * LD + 16 * q + j16], C, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int u = 16 * w + kk + 4 * r;
        const double b = lw[q] - 0.5 * ((nas[u] + nm[q]) - 2.0 * C[r]);
        if (u < nt) acc[q] += cf[u] * exp(b - mx[u]);      // (a successor behind the last one adds nothing)
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {      // the four lanes of a candidate, then the four waves
    double v = acc[q];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (kk == 0) red[w * CB + 16 * q + j16] = v;
  }
  __syncthreads();
  if (w != 0) return;
  const bool mine = i0 + lane < n;
  const double wi = mine ? (red[lane] + red[CB + lane]) + (red[2 * CB + lane] + red[3 * CB + lane]) : 0.0;
  if (mine) row[i0 + lane] = wi;
  const double s2 = wave_sum(wi * wi);
  if (lane == 0) sm.part[((size_t)p * sm.rows + c.j) * gridDim.y + blockIdx.y] = s2;
}

__global__ __launch_bounds__(256) void k_ps_ess(PfArgs f, SmoothArgs sm, int n_blocks) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)f.batch) return;
  const int cnt = f.n_obs_v ? f.n_obs_v[p] : f.n_obs;
  double* less = sm.less + p * sm.rows;
  for (int j = cnt - 1; j >= 0; j--) {
    if (!f.h_flag[p * f.M + j]) { less[j] = less[j + 1]; continue; }
    const double* part = sm.part + (p * sm.rows + j) * n_blocks;
    double s2 = 0.0;
    for (int blk = 0; blk < n_blocks; blk++) s2 += part[blk];
    less[j] = 1.0 / s2;
  }
}

// the kernels' compile-time D: 1 (OU, double well), 3 (Lorenz-63), 0 (Lorenz-96 of any D >= 3), or -1: no kernel
int smooth_dc(const SampleArgs& a) {
  return a.model == VGPA_MODEL_L96 && a.D >= 3                                ? 0
         : a.D == 1 && (a.model == VGPA_MODEL_OU || a.model == VGPA_MODEL_DW) ? 1
         : a.D == 3 && a.model == VGPA_MODEL_L63                              ? 3
                                                                              : -1;
}

bool smooth_args_fit(const PfArgs& f, const SampleArgs& a, const SmoothArgs& sm) {
  return f.batch >= 1 && f.n_paths >= 1 && f.M >= 1 && sm.rows >= f.M + 1 && f.h_flag && f.h_anc && f.h_clouds && f.h_lw && f.obs_t && sm.xt && sm.rmax &&
         sm.rsum && sm.centre && sm.wtab && sm.part && sm.less && a.D >= 1 && a.D <= kMaxSmallD && a.D == f.D && a.A && a.b && a.R && a.R_diag && f.k >= 0 &&
         smooth_grid_fits(a.D, f.n_paths) && smooth_dc(a) >= 0;
}

}  // namespace

int smooth_column_blocks(int n_paths) { return (n_paths + kSmoothColBlock - 1) / kSmoothColBlock; }

bool smooth_grid_fits(int D, int n_paths) {
  return ((size_t)n_paths * D + 255) / 256 <= (size_t)kMaxGridY && (n_paths + kSmoothRowBlock - 1) / kSmoothRowBlock <= kMaxGridY;
}

hipError_t launch_smooth_cut(const PfArgs& f, const SampleArgs& a, const SmoothArgs& sm, hipStream_t st) {
  if (!smooth_args_fit(f, a, sm)) return hipErrorInvalidValue;
  const int n = f.n_paths, D = a.D;
  hipLaunchKernelGGL(k_ps_successors, dim3(f.batch, (unsigned)(((size_t)n * D + 255) / 256)), dim3(256), 0, st, f, a, sm);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const size_t row_lds = ((size_t)D * kRowLd + (size_t)kSmoothRowBlock * D + D + 8 * kSmoothRowBlock) * sizeof(double);
  const size_t col_lds = ((size_t)D * kColLd + (size_t)kColTile * D + 2 * kColTile + D + 4 * kSmoothColBlock) * sizeof(double);
  const dim3 row_grid(f.batch, (n + kSmoothRowBlock - 1) / kSmoothRowBlock), col_grid(f.batch, smooth_column_blocks(n));
  if (a.model == VGPA_MODEL_L96 && D >= 5) {      // the cross term on the matrix cores, D padded to 16, 32, 48 or 64
    hipLaunchKernelGGL(k_ps_centre, dim3(f.batch), dim3(256), 0, st, f, sm);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return with_int<1, 4>((D + 15) / 16, [&](auto tiles) {
      constexpr int NT = decltype(tiles)::value, DP = 16 * NT;
      const size_t rows_lds = ((size_t)DP * kRowLd + (size_t)kSmoothRowBlock * (DP + 1) + 2 * DP + kSmoothRowBlock + kRowTile + 8 * kSmoothRowBlock) * sizeof(double);
      const size_t cols_lds = ((size_t)DP * kColLd + (size_t)kColTile * (DP + 1) + 3 * kColTile + 2 * DP + 5 * kSmoothColBlock) * sizeof(double);
      if (hipError_t e = launch_lds(k_ps_rows_mfma<NT>, row_grid, dim3(256), rows_lds, st, f, a, sm); e != hipSuccess) return e;
      return launch_lds(k_ps_columns_mfma<NT>, col_grid, dim3(256), cols_lds, st, f, a, sm);
    });
  }
  return with_int<0, 3>(smooth_dc(a), [&](auto dc) {
    constexpr int DC = decltype(dc)::value;
    if constexpr (DC == 2) return hipErrorInvalidValue;
    else {
      if (hipError_t e = launch_lds(k_ps_rows<DC>, row_grid, dim3(256), row_lds, st, f, a, sm); e != hipSuccess) return e;
      return launch_lds(k_ps_columns<DC>, col_grid, dim3(256), col_lds, st, f, a, sm);
    }
  });
}

hipError_t launch_smooth_ess(const PfArgs& f, const SmoothArgs& sm, hipStream_t st) {
  if (f.batch < 1 || f.n_paths < 1 || f.M < 1 || sm.rows < f.M + 1 || !f.h_flag || !sm.part || !sm.less) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ps_ess, dim3((unsigned)((f.batch + 255) / 256)), dim3(256), 0, st, f, sm, smooth_column_blocks(f.n_paths));
  return hipGetLastError();
}

}  // namespace vgpa
