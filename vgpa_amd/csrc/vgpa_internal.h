// Internal declarations shared by the translation units of libvgpa_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/vgpa_hip.h"

namespace vgpa {

#ifdef __HIPCC__
// A wave-uniform int from read-only global memory as a SCALAR load (s_load_dword -> SGPR, counted by lgkmcnt).  Behind the first
// global store of a kernel the compiler no longer proves such a load unclobbered and emits a vector load + s_waitcnt vmcnt(0) +
// v_readfirstlane on the spot -- i.e. it waits for every HBM prefetch the step has just issued (round 3: this was the backward
// steppers' observation-index lookup, one exposed memory round trip per time step).
__device__ __forceinline__ int ldu(const int32_t* p, int i) {
  typedef const int32_t __attribute__((address_space(4))) * cptr;
  return ((cptr)p)[i];
}
// ... and a wave-uniform double (constant matrices read once per kernel: they stay in SGPRs)
__device__ __forceinline__ double lds_const(const double* p, int i) {
  typedef const double __attribute__((address_space(4))) * cptr;
  return ((cptr)p)[i];
}
#endif

#ifdef __HIPCC__
// packed lower triangles (OdeArgs::s_packed): element (r, c), c <= r, at tri_off(r) + c; tri_row(e) = the row of flat index e
__host__ __device__ __forceinline__ int tri_off(int r) { return r * (r + 1) / 2; }
__device__ __forceinline__ int tri_row(int e) {                     // e < 2^20
  int i = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  i += (tri_off(i + 1) <= e) ? 1 : 0;
  i -= (tri_off(i) > e) ? 1 : 0;
  return i;
}
__host__ __device__ __forceinline__ int tri_idx(int r, int c) { return r >= c ? tri_off(r) + c : tri_off(c) + r; }
#endif

constexpr int kMaxSmallD = 64;   // single-workgroup (LDS resident) stepping kernels
constexpr int kMaxLaneD = 4;     // one-lane-per-problem stepping kernels (ode_small.hip)
constexpr int kMaxTheta = 4;

// Arguments of the time-stepping kernels (fwd: moments, bwd: Lagrange multipliers).
struct OdeArgs {
  int D, Np, batch;
  int sym_units;            // D <= 44: symmetric-unit kernels instead of the role-specialised ones (the context's plan says which)
  size_t strideA, strideB;  // elements between consecutive problems in A / b (x layout: len_x for both)
  double dt;
  // forward
  const double* A;       // [B][Np][D][D]
  const double* b;       // [B][Np][D]
  const double* m0;      // [D], or [B][D] with m0_stride = D (per-problem data, vgpa_set_problem_data)
  const double* S0;      // [D][D], or [B][D][D] with S0_stride = D*D
  const double* Sigma;   // [D][D]
  double* m;             // [B][Np][D]
  double* S;             // [B][Np][D][D]
  // backward
  const double* dEm;     // [B][Np][D]
  const double* dEs;     // [B][Np][D][D]
  const double* jm_dense;  // [B][Np][D]      or nullptr (then the sparse form is used)
  const double* js_dense;  // [B][Np][D][D]   or nullptr
  const int32_t* obs_idx;  // [Np] -> observation counter n, or -1; [B][Np] with obs_idx_stride = Np (per-problem times)
  const double* jm_sparse; // [B][M][D]
  const double* js_const;  // [D][D]
  int n_obs;
  double* lam;           // [B][Np][D]
  double* psi;           // [B][Np][D][D]
  // fused sweeps of the batched symmetric-unit kernels (sym::stores_q) with Sigma = sigma^2 I: q_on = 1 and q_scale = 1 / sigma^2, and
  // `psi` receives Q''_t = q_scale A_t - 2 Psi_t (what the gradient assembly needs of A_t and Psi_t) instead of Psi_t
  int q_on;
  double q_scale;
  // lane-per-problem kernels of the fused small-D sweep (ode_small.hip): the moments in a layout the context owns, TIME-major with the
  // problem fastest -- entry e (the packed lower triangle of S_t, then m_t: W = D (D + 1) / 2 + D entries) of grid point t of problem p at msT[(t * W + e) * bpad + p] -- so that a
  // wave's 64 lanes read / write 512 contiguous bytes per entry straight from / into registers; nullptr: the [B][Np] arrays m / S
  double* msT;
  int bpad;
  // fused batched sweeps of the fragment-cover kernels (33 <= D <= 40): S_t leaves the forward kernel as its packed LOWER triangle,
  // row-major -- element (r, c), c <= r, of grid point t of problem p at S[(p * Np + t) * D (D + 1) / 2 + r (r + 1) / 2 + c] -- which is
  // all the energy kernel factorises and half of what the gradient assembly streams (vgpa_fetch unpacks it on demand)
  int s_packed;
  int ds_packed;            // dEs holds packed lower triangles (EnergyArgs::ds_packed): symmetric-unit cover kernels, backward
  const double* jmT;     // sparse vector jumps in the same spirit: entry i of observation n of problem p at jmT[(n * D + i) * bpad + p]
  // backward kernel with the gradient assembly on its helper waves (sym::fuses_grad: fragment-cover kernels, RK4, Sigma = sigma^2 I,
  // Lorenz-96, packed S_t): grad_on = 1, q_on = 1; the kernel reads S (packed), m, b, Ef, Am of every grid point beside its own
  // streams and writes g = dt [gLa | gLb] (variational.py:263-288) -- Psi_t / Q''_t are NOT stored, lam_t is
  int grad_on;
  const double* Ef;      // [B][Np][D] <f>_t            (energy kernel)
  const double* Am;      // [B][Np][D] A_t m_t          (energy kernel)
  double* g;             // [B][strideA]: problem p's [Np][D][D] gLa, then [Np][D] gLb (the caller's x layout)
  // per-problem data (vgpa_set_problem_data), last so that the kernel-argument offsets of everything above stay where they were
  size_t m0_stride, S0_stride;   // elements between consecutive problems' m0 / S0; 0: shared by the batch
  int obs_idx_stride;            // Np: obs_idx is [B][Np]; 0: the observation times are shared by the batch
  // per-problem parameters (vgpa_set_problem_params), last for the same reason
  size_t Sigma_stride;           // D*D: Sigma is [B][D][D]; 0: shared by the batch
  const double* q_scale_v;       // [B] 1 / sigma_p^2 instead of q_scale, or nullptr
  // per-problem observation model (vgpa_set_problem_obs_model), last for the same reason
  size_t js_const_stride;        // D*D: js_const is [B][D][D] (packed copy: the first D (D + 1) / 2 of each row); 0: shared by the batch
};

// Fused lane-per-problem pass of the models with closed-form moments (OU, double well, Lorenz-63; ode_small.hip::k_sweep_lane):
// E_sde terms of every grid point re-evaluated in registers, backward recursion, gradient assembly, F -- from (A, b, m, S) alone.
struct LaneSweepArgs {
  OdeArgs o;               // A, b (x layout), m, S, dt, batch, Np, D, sparse jumps (obs_idx, jm_sparse, js_const, n_obs)
  int model;
  int want_grad;           // 0: F only (no recursion); 1: F and the gradient
  double theta[kMaxTheta];
  double sigma1;           // 1-D models: sigma
  double isg[4];           // diagonal of Sigma^-1
  double isig[16];         // Sigma^-1 [D][D]
  double e0, pre, div;     // F = e0 + pre * trapz(E_sde(t)) / div + E_obs
  const double* eobs;      // [B]
  double* esde;            // [B]
  double* f;               // [B]
  double* g;               // [B][Np*D*D + Np*D] (want_grad)
  const double* e0v;       // [B] per-problem e0 instead of e0, or nullptr (last: the offsets above stay where they were)
  // per-problem parameters (vgpa_set_problem_params): all three set or all nullptr; each lane loads its own row before the time loop
  const double* theta_v;   // [B][kMaxTheta]
  const double* sigma1_v;  // [B] 1-D models: sigma (also the divisor of E_sde)
  const double* isig_v;    // [B][D][D] Sigma^-1
};

struct EnergyArgs {
  int model, D, Np, batch;
  double dt;
  double theta[kMaxTheta];
  double sigma1;            // 1-D models: sigma
  const double* isg;        // [D] diagonal of Sigma^-1
  size_t strideA, strideB;  // elements between consecutive problems in A / b
  const double* A;          // [B][Np][D][D] (problem stride strideA)
  const double* b;          // [B][Np][D]    (problem stride strideB)
  const double* m;          // [B][Np][D]
  const double* S;          // [B][Np][D][D]
  double* e_t;              // [B][Np] integrand of E_sde
  double* Ef;               // [B][Np][D]
  double* Edf;              // [B][Np][D][D] or nullptr
  double* dEm;              // [B][Np][D]
  double* dEs;              // [B][Np][D][D]
  int s_packed;             // S holds packed lower triangles (OdeArgs::s_packed)
  int ds_upper;             // L96, D <= 64: write only the upper triangle of dEs (row <= col) -- the consumer is a symmetric-unit backward
                            // kernel, which reads nothing else (fused sweeps; VGPA_FETCH_DESDE_DS mirrors it on the way out)
  int ds_packed;            // ... as PACKED lower triangles (element (r, c), c <= r, of the symmetric matrix at tri_off(r) + c; matrix
                            // stride tri_off(D)): k_energy_l96_r with the cover kernels behind it (OdeArgs::ds_packed)
  double* hyp;              // [B][Np][H] per-grid-point integrands of dEsde/dtheta, dEsde/dSigma (nullptr: skipped)
  double* Am;               // [B][Np][D] A_t m_t, a by-product the gradient assembly reuses (L96 kernel; may be nullptr)
  int32_t* status;          // [B] device status word (bit0: S_t not positive definite)
  // per-problem parameters (vgpa_set_problem_params), last so that the offsets above stay where they were
  const double* theta_v;    // [B][kMaxTheta] instead of theta, or nullptr
  const double* sigma1_v;   // [B] instead of sigma1, or nullptr
  size_t isg_stride;        // D: isg is [B][D]; 0: shared by the batch
  // dF/dtheta from the resident state (vgpa_theta_gradient), last for the same reason
  double* tg;               // L96, D <= 64: [B][Np] integrand sum_i isg_i UT-mean(f_i(chi) + (A chi)_i - b_i); set: k_energy_l96_r computes this and
                            // NOTHING else (no other array is written).  nullptr: skipped
  int hyp_only;             // 1-D models, Lorenz-63: write `hyp` and nothing else (the cached energy arrays stay as they are)
};

// dF/dtheta integrands of the lane-per-problem contexts (ode_small.hip::k_theta_lane): x and the time-major moments in, [B][H] out
struct ThetaLaneArgs {
  int model, D, Np, batch, bpad;
  double dt;
  size_t stride_x;          // elements between consecutive problems in A / b (len_x)
  const double* A;          // [B][Np][D][D]
  const double* b;          // [B][Np][D]
  const double* msT;        // OdeArgs::msT
  double theta[kMaxTheta];
  const double* theta_v;    // [B][kMaxTheta] instead of theta, or nullptr
  double* out;              // [B][H] trapezoids of the integrands, H = 1 (OU, double well) or 3 (Lorenz-63); unscaled (vgpa_theta_gradient)
};

struct ObsArgs {
  int D, Np, batch, n_obs, single;
  const int64_t* obs_t;     // [M]     ([B][M] with obs_t_stride = M: per-problem times)
  const double* obs_y;      // [M][D]  ([B][M][D] with obs_y_stride = M*D: per-problem values)
  const double* Q;          // [D][D]  H R^-1 H^T     (1-D: 1/r)
  const double* K;          // [D][D]  H^T R^-1 H^T   (1-D: H/r ... see obs kernel)
  const double* rinv_diag;  // [D]     diag(R^-1)
  double obs_const;         // M*(d*log(2pi) + logdet R)
  const double* m;          // [B][Np][D]
  const double* S;          // [B][Np][D][D]
  double* jm_sparse;        // [B][M][D]
  double* eobs;             // [B]
  int s_packed;             // S holds packed lower triangles (OdeArgs::s_packed)
  int diag;                 // Q and K are diagonal (diagonal R, H = I)
  double* part;             // [B][M] per-observation terms of the n-D energy (grid-parallel variant) or nullptr
  size_t obs_t_stride, obs_y_stride;   // elements between consecutive problems' obs_t / obs_y; 0: shared by the batch
  // per-problem observation model (vgpa_set_problem_obs_model), last so that the offsets above stay where they were: all set or all 0 / nullptr
  size_t Q_stride, K_stride, rinv_stride;   // D*D, D*D, D: Q / K / rinv_diag are [B][D][D] / [B][D][D] / [B][D]; 0: shared by the batch
  const double* obs_const_v;     // [B] instead of obs_const, or nullptr
  const int32_t* n_obs_v;        // [B] observations of problem p (<= n_obs, the capacity of a row) instead of n_obs, or nullptr
  size_t js_const_stride;        // launch_obs_dense: D*D when its js_const is [B][D][D]; 0: shared by the batch
};

struct GradArgs {
  int model, D, Np, batch, sigma_diag;
  int scalar_product;       // diagnostics: VALU inner products instead of the matrix-core product (VGPA_FLAG_FORCE_GENERIC)
  double dt;
  double theta[kMaxTheta];
  const double* isig;       // [D][D] Sigma^-1
  size_t strideA, strideB;  // elements between consecutive problems in A / b
  const double* A; const double* b;
  const double* m; const double* S;
  const double* lam; const double* psi;
  int s_packed;             // S holds packed lower triangles (OdeArgs::s_packed)
  int psi_is_q;             // `psi` holds Q''_t = Sigma^-1 A_t - 2 Psi_t (OdeArgs::q_on): A is not read
  const double* Ef;
  const double* Am;         // [B][Np][D] A_t m_t left by the energy kernel, or nullptr (then recomputed)
  const double* Edf;        // dense [B][Np][D][D] or nullptr (then recomputed from the model)
  double* g;                // [B][Np*D*D + Np*D]
  // per-problem parameters (vgpa_set_problem_params)
  const double* theta_v;    // [B][kMaxTheta] instead of theta, or nullptr (read where <df/dx> is recomputed)
  size_t isig_stride;       // D*D: isig is [B][D][D]; 0: shared by the batch
};

struct ReduceArgs {
  int Np, batch;
  double dt, pre, div, e0;
  const double* e_t;        // [B][Np]
  const double* eobs;       // [B]
  double* esde;             // [B]
  double* f;                // [B]
  const double* e0v;        // [B] per-problem e0 instead of e0, or nullptr
  const double* div_v;      // [B] per-problem div (1-D models: sigma_p), or nullptr
};

// What a slot of the particle filter carries along its lineage (the host's request and the walks' property use the one word)
enum class Carry { None, Stats, Events };      // nothing; the path statistics (Q, G, H); the event records (X, T, N)
// Euler-Maruyama sample paths (sample.hip): x_k = x_{k-1} + dt drift_{k-1}(x_{k-1}) + R xi_k on the context's grid.  The twelve things a launch
// can do with them (the table at the top of sample.hip); the host names one at every launch_sample_walk, and SampleArgs says what each reads
enum class Walk { Plain, Weighted, Segment, SegmentStats, Replay, Lineage, Forecast, ReplayCov, Backward, Conditional, SegmentEvents, ReplayMarginals };
struct SampleArgs {
  int kind, model, D, Np, batch, n_paths, stride, n_keep;
  double dt;
  uint64_t seed;
  const double* A;          // posterior kind: [B][Np][D][D] (problem stride stride_x)
  const double* b;          // ... [B][Np][D]
  size_t stride_x;
  double theta[kMaxTheta];  // model kind
  const double* theta_v;    // [B][kMaxTheta] instead of theta, or nullptr
  const double* R;          // [D][D] lower factor of Sigma dt, row-major; [B][D][D] with R_stride = D*D
  size_t R_stride;
  int R_diag;               // every R is diagonal: the noise is a scale
  const double* x0;         // [B][D] given start, or nullptr: x_0 = m0 + L0 xi_0
  const double* m0;         // [D], or [B][D] with m0_stride = D
  const double* L0;         // [D][D] lower factor of S0, or [B][D][D] with L0_stride = D*D
  size_t m0_stride, L0_stride;
  double* out;              // [B][n_paths][n_keep][D]
  // importance weights of the posterior paths against the model SDE (vgpa_sample_paths_weighted).  Walk::Weighted reads
  // them (posterior kind, diagonal R, theta / theta_v set): `out` may be nullptr (no path is stored), and every path's x_0 goes to `start`
  double* logw;             // [B][n_paths][2]: the path term, the observation term; nullptr for every other walk
  double* start;            // [B][n_paths][D]
  const int64_t* obs_t;     // [M] grid indices, strictly increasing ([B][M] with obs_t_stride = M), as ObsArgs has them
  const double* obs_y;      // [M][D] ([B][M][D] with obs_y_stride = M*D)
  const double* Q;          // [D][D] H R^-1 H^T ([B][D][D] with Q_stride = D*D); 1-D: 1 / r
  size_t obs_t_stride, obs_y_stride, Q_stride;
  int Q_diag;               // every Q is diagonal
  int n_obs;                // observations of a problem ...
  const int32_t* n_obs_v;   // ... [B] instead of n_obs, or nullptr
  double obs_const;         // the additive constant of E_obs as ObsArgs has it ...
  const double* obs_const_v;   // ... [B] instead of obs_const, or nullptr
  double obs_const_scale;   // ... and the factor E_obs gives it: 1/2 (n-D), 1 (1-D models, whose constant is halved already)
  // Walk::Segment, SegmentStats and Replay (vgpa_particle_filter): the grid steps k_begin < k <= k_end of the weighted
  // walk from and to pf_x, the path and observation increments added to pf_lw.  The observation cursor starts at 0 in the first segment
  // (an observation at grid index 0 applies to the start), else behind k_begin.  x0 / m0 / L0 / out / logw / start are not read.
  int seg_first, k_begin, k_end;
  double* pf_x;             // [B][n_paths][D]
  double* pf_lw;            // [B][n_paths]
  // the path statistics of a lineage (vgpa_particle_statistics): Walk::SegmentStats adds every step's
  // Q_j += r_j^2 / dt, G_j += phi_j r_j, H_j += dt phi_j^2 (r = dt (g - f) + eta, phi_j = df_j / dtheta_a(j) at x_{k-1}) to the slot's row
  double* pf_stats;         // [B][n_paths][3][D]; nullptr for every other walk
  // the replay of vgpa_particle_moments: Walk::Replay is the walk of the segment without its weight sums (pf_lw is
  // not touched); at every kept grid index k = 0 mod stride of the segment (k = 0: the first segment) workgroup (p, blk) stores
  // sum_i W_i x_i(k) and sum_i W_i x_i(k)^2 over its own slots, W = the row of pf_wtab of the problem's stretch
  const double* pf_wtab;    // [B][pf_rows][n_paths] descendant weights; nullptr for every other walk
  double* pf_part;          // [B][sample_segment_blocks()][n_keep][2][D]
  int pf_rows, pf_M;        // rows per problem of pf_wtab; of Walk::Backward's histories (below)
  // Walk::Lineage (vgpa_particle_paths): the unweighted posterior walk of n_paths = K lanes
  // per problem, stored as vgpa_sample_paths stores it, in which lane m draws with the counter word pf_slots[p][j][m] while it is in
  // stretch j of its problem's own observation row (obs_t / n_obs as above): row 0 for the start, the next row behind every observation
  const int32_t* pf_slots;  // [B][pf_slot_rows][n_paths]
  int pf_slot_rows;
  // Walk::Forecast (vgpa_particle_forecast): the model SDE (model kind, diagonal R, theta / theta_v) carried from the
  // cloud pf_x [B][pf_n][D] at absolute grid index k_begin to k_end, lane i drawing from the counters (k_begin + h, word, p, j).  One of
  // two launches.  The cloud: n_paths = pf_n lanes per problem, word = the slot, pf_part set: at h = 0, stride, 2 stride, ... workgroup
  // (p, blk) stores sum_i W_i x_i and sum_i W_i x_i^2 over its own slots with W = pf_wtab [B][pf_n] (n_keep rows), and x(k_end) goes back
  // to pf_x.  The members: n_paths = K lanes per problem, out and pf_slots [B][1][K] set: lane m starts from slot s = pf_slots[p][0][m] of
  // the cloud, draws with word s and stores as Walk::Plain stores; pf_x is read only
  int pf_n;
  // Walk::ReplayCov (vgpa_particle_covariance): Walk::Replay with the whole second-moment matrix.  Every field as for the
  // replay, but pf_part is [B][sample_segment_blocks()][n_keep][V], V = sample_cov_len(D) = D + D (D + 1) / 2: sum_i W_i x_i(k), then the lower
  // triangle of sum_i W_i x_i(k) x_i(k)^T packed by rows, entry (a, b <= a) at D + a (a + 1) / 2 + b.  No field of its own.
  // Walk::Backward (vgpa_particle_backward_paths): Walk::Lineage, every field as there, in which lane m, having completed
  // and stored its problem's observation index t_j, goes on from pf_clouds[p][j][pf_hanc[p][j][pf_slots[p][j + 1][m]]]: the filter's
  // histories (rows of pf_M observations per problem; pf_n particles per cloud)
  const double* pf_clouds;  // [B][pf_M][pf_n][D]; nullptr for every other walk
  const int32_t* pf_hanc;   // [B][pf_M][pf_n]; nullptr for every other walk
  // Walk::Conditional (vgpa_particle_conditional): Walk::Segment, every field as there, in which slot 0 of every problem
  // is pinned to the reference trajectory pf_ref[p] -- [B][Np][D], WalkOwn::pf_ref and no field here: the other
  // walks' kernels take this struct alone --: it draws nothing, takes the increment the reference implies, eta* = (ref_k - ref_{k-1})
  // - dt g(ref_{k-1}), into the step's weight term in place of R xi, and its state becomes ref_k as loaded
  // Walk::SegmentEvents (vgpa_particle_events): Walk::Segment, every field as there, in which every slot carries the row
  // (X, T, N) of event records of its lineage where pf_stats points, [B][n_paths][3][D] as for SegmentStats: with g_j(x) = s_j (x_j - c_j),
  // at every step k of the segment X_j = fmax(X_j, g_j(x_k)) and, where g_j(x_k) > 0, T_j = min(T_j, k), N_j += 1 (T, N: exact integers
  // held as doubles).  The levels c and the sides s are ev_level [B][D] and ev_side [B][D] (+1 / -1), of WalkOwn
  // and no fields here
  // Walk::ReplayMarginals (vgpa_particle_marginals): Walk::Replay's states, every field as there but pf_wtab and pf_part,
  // which stay nullptr: at a kept grid index k' stride slot i adds its integer descendant weight Q_i (MarginalArgs::qtab, the row of the
  // problem's stretch) to mass[p][k'][d][bin(x_i[d])] for every component d, bin(x) = #{l: c_l < x} over the component's ladder of L levels
};
// The levels, weights and result of Walk::ReplayMarginals: WalkOwn::mg and no fields of SampleArgs
struct MarginalArgs {
  const double* levels;            // [B][D][L], finite and strictly increasing along L
  int L;                           // 1 .. kMaxMarginalLevels
  const uint64_t* qtab;            // [B][pf_rows][n_paths] integer descendant weights
  unsigned long long* mass;        // [B][n_keep][D][L + 1], zero before the first segment
};
constexpr int kMaxMarginalLevels = 63;
// What one walk alone reads besides SampleArgs, as the host hands it to launch_sample_walk: no other walk's kernel takes any of it
struct WalkOwn {
  const double* pf_ref = nullptr;        // Walk::Conditional: the reference trajectories [B][Np][D]
  const double* ev_level = nullptr;      // Walk::SegmentEvents: the levels [B][D] ...
  const int32_t* ev_side = nullptr;      // ... and the sides [B][D] (+1 / -1)
  const MarginalArgs* mg = nullptr;      // Walk::ReplayMarginals
};
// hipErrorInvalidValue where a field the walk reads is missing or out of range, where a field that belongs to another walk is set (of
// `own`: pf_ref in every walk but Conditional, which needs it; ev_level and ev_side in every walk but SegmentEvents, which needs both; mg
// in every walk but ReplayMarginals, which needs it whole), and for D = 2 in every walk but Plain (no stochastic model has D = 2)
hipError_t launch_sample_walk(Walk w, const SampleArgs& a, hipStream_t st, const WalkOwn& own = {});
// workgroups per problem of a segment launch: the blocks of the replay's partial sums
int sample_segment_blocks(int D, int n_paths);
int sample_max_paths(int D);      // the largest n_paths per problem a segment, replay or forecast launch takes at this D (grid.y)
// doubles per kept grid index of Walk::ReplayCov's partial sums: the mean and the packed lower triangle
inline size_t sample_cov_len(int D) { return (size_t)D + (size_t)D * (D + 1) / 2; }

// the start and the resampling step of the particle filter (sample.hip: k_pf_start, k_pf_resample)
struct PfArgs {
  int D, batch, n_paths, M;   // M: rows of the histories (the context's observation capacity)
  uint64_t seed;
  // start
  const double* x0;         // [B][D] given start, or nullptr: m0 + L0 xi_0 as in SampleArgs
  const double* m0; const double* L0;
  size_t m0_stride, L0_stride;
  const double* mu0;        // [B][D] prior mean and
  const double* Lt;         // ... [B][D][D] lower factor of the prior covariance: init is evaluated; or nullptr (init = 0)
  double obs_const; const double* obs_const_v; double obs_const_scale;   // as in SampleArgs
  double* x;                // [B][n_paths][D] the particles
  double* ws;               // [B][n_paths][D] work space
  double* lw;               // [B][n_paths] log-weights (both kernels)
  // resampling at grid index k
  int k, last;              // last: k = Np - 1, where nothing is resampled
  double ess_fraction;
  const int64_t* obs_t; size_t obs_t_stride; int n_obs; const int32_t* n_obs_v;   // as in SampleArgs
  const double* x_in; double* x_out;   // [B][n_paths][D] each
  double* cum;              // [B][n_paths] prefix sums
  int32_t* anc;             // [B][n_paths] ancestors of this step
  double* h_ess; int32_t* h_flag;      // [B][M] each
  int32_t* h_anc;           // [B][M][n_paths], or nullptr
  double* h_clouds;         // [B][M][n_paths][D], or nullptr
  double* h_lw;             // [B][M][n_paths] the log-weights a resampling step finds (the observation's term included), or nullptr
  // the rows of vgpa_particle_statistics, gathered by ancestor together with x; both or neither
  const double* st_in; double* st_out;   // [B][n_paths][3][D] each
  // vgpa_particle_conditional: the reference trajectories slot 0 is pinned to (k_pf_pin, k_pf_cresample, k_pf_ref_fill), or nullptr
  const double* ref;        // [B][Np][D]
  int Np;
};
hipError_t launch_pf_start(const PfArgs& a, hipStream_t st);
hipError_t launch_pf_resample(const PfArgs& a, hipStream_t st);
// vgpa_particle_conditional (sample.hip: k_pf_pin, k_pf_cresample, k_pf_ref_fill).  pin, behind launch_pf_start: slot 0 of
// every problem becomes ref[p][0], its log-weight the start's own formula at that state.  cresample: the step between two segments with
// slot 0 pinned -- the decision, ESS and new log-weight of launch_pf_resample, multinomial ancestors for the slots >= 1, the ancestor of slot
// 0 drawn by ancestor sampling against ref[p][k + 1] (a: the model, theta, the diagonal R and dt of the filter's arguments) into the
// history alone, x_out_0 = x_in_0.  ref_fill: out [B][Np][D], the one trajectory per problem of Walk::Backward at stride 1, gets ref[p][k]
// wherever row j(k) of table [B][rows][1] is 0
hipError_t launch_pf_pin(const PfArgs& a, hipStream_t st);
hipError_t launch_pf_cresample(const PfArgs& f, const SampleArgs& a, hipStream_t st);
hipError_t launch_pf_ref_fill(const PfArgs& f, int rows, const int32_t* table, double* out, hipStream_t st);
// mean [B][3][D] = sum_i w_i stats[.][i] / sum_i w_i, w_i = exp(lw_i - max lw) (sample.hip: k_pf_stats_mean)
hipError_t launch_pf_stats_mean(int D, int batch, int n_paths, const double* lw, const double* stats, double* mean, hipStream_t st);
// vgpa_particle_events (sample.hip: k_pf_events_start, k_pf_events_cdf).  start, behind launch_pf_start: rows
// [B][n_paths][3][D] get the record of grid index 0 from the particles x [B][n_paths][D]: X_j = g_j(x), T_j = 0 and N_j = 1 where g_j(x) > 0,
// else T_j = Np (never so far) and N_j = 0.  cdf [B][n_keep][D], n_keep = (Np - 1) / stride + 1: cdf[p][k'][j] = sum_i W_i 1[T_ij <= k' stride]
// with W_i = w_i / sum w, w_i = exp(lw_i - max lw): one workgroup per (problem, component), every addition in an order the launch does not
// change
hipError_t launch_pf_events_start(int D, int batch, int n_paths, int Np, const double* x, const double* level, const int32_t* side, double* rows,
                                  hipStream_t st);
hipError_t launch_pf_events_cdf(int D, int batch, int n_paths, int Np, int stride, const double* lw, const double* rows, double* cdf, hipStream_t st);
// vgpa_particle_moments (sample.hip: k_pf_descend, k_pf_gather, k_pf_moments_sum).  Of PfArgs, descend reads lw, h_flag, h_anc, M and the
// observation counts: wtab [B][rows][n_paths] gets row c = the normalised final weights and rows c-1 .. 0 by the backward recursion
// through the stored ancestors, less [B][rows] the lineage ESS of the rows written (the others stay as they are); gather is the step
// between two segments of the replay, x_out_i = x_in_{h_anc[p][j][i]} at the problem's observation j with t_j = k, a copy without one
hipError_t launch_pf_descend(const PfArgs& a, int rows, double* wtab, double* less, hipStream_t st);
// vgpa_particle_marginals (sample.hip: k_pf_quantise, k_pf_descend_q).  quantise, behind launch_pf_descend: row c of qtab
// [B][rows][n_paths] = (uint64) trunc(W 2^62) of row c of wtab, and the same values densely to qfinal [B][n_paths].  descend_q: rows c-1 .. 0 of qtab by launch_pf_descend's recursion -- the
// same bisections on the stored ancestors -- in 64-bit integer arithmetic
hipError_t launch_pf_quantise(const PfArgs& a, int rows, const double* wtab, uint64_t* qtab, uint64_t* qfinal, hipStream_t st);
hipError_t launch_pf_descend_q(const PfArgs& a, int rows, uint64_t* qtab, hipStream_t st);
hipError_t launch_pf_gather(const PfArgs& a, hipStream_t st);
// vgpa_particle_paths (sample.hip: k_pf_pick, k_pf_trace).  table [B][rows][K] int32, rows > every problem's observation count c.  pick
// reads lw, seed and the counts and overwrites cum: row c gets the final slots of K trajectories, by systematic resampling from the final
// weights with the uniform of Philox counter (Np, 0, p, 0xffffffff).  trace reads row c, h_flag, h_anc and M and writes rows c-1 .. 0: the
// slot each trajectory sat in during every stretch.  sample_lineages_fit: Walk::Lineage can be launched with K lanes per problem
hipError_t launch_pf_pick(const PfArgs& a, int Np, int K, int rows, int32_t* table, hipStream_t st);
hipError_t launch_pf_trace(const PfArgs& a, int K, int rows, int32_t* table, hipStream_t st);
bool sample_lineages_fit(int D, int batch, int K);
bool pf_flat_grid_fits(size_t entries);      // grid.x takes one thread per entry, 256 per workgroup (k_pf_moments_sum, k_pf_cov_unpack, k_pf_trace)
// vgpa_particle_backward_paths (sample.hip: k_pf_backward) in place of the trace: rows c-1 .. 0 of table by backward simulation.  f: the
// histories h_flag, h_anc, h_clouds, h_lw with M, n_paths, seed and the observation rows; a: of the filter's arguments the model, theta,
// A, b, the diagonal R and dt.  One launch: workgroup (p, blk) owns kBackwardBlock trajectories of problem p through all of its cuts
constexpr int kBackwardBlock = 8, kMaxGridY = 65535;
hipError_t launch_pf_backward(const PfArgs& f, const SampleArgs& a, int K, int rows, int32_t* table, hipStream_t st);
inline bool pf_backward_fits(int K) { return (K + kBackwardBlock - 1) / kBackwardBlock <= kMaxGridY; }
// vgpa_particle_forecast (sample.hip: k_pf_normalise): w [B][n_paths] = exp(lw - max lw) / the sum of these, per problem
hipError_t launch_pf_normalise(int batch, int n_paths, const double* lw, double* w, hipStream_t st);
// out [B][len] = sum over blk, in block order, of part [B][n_blocks][len]
hipError_t launch_pf_moments_sum(int batch, int n_blocks, size_t len, const double* part, double* out, hipStream_t st);
// vgpa_particle_covariance (sample.hip: k_pf_cov_unpack): packed [rows][sample_cov_len(D)], rows = B n_keep, as Walk::ReplayCov and the sum
// leave it, to mean [rows][D] and second [rows][D][D], both triangles from the one packed entry.  One thread per entry of second, a
// one-dimensional grid: at most (2^31 - 1) 256 = 2^39 - 256 entries
hipError_t launch_pf_cov_unpack(int D, size_t rows, const double* packed, double* mean, double* second, hipStream_t st);

// Two-time covariance of the posterior process (lag_cov.hip).  LagStartArgs: the starting matrices of every (problem,
// anchor) from S_t as it is resident, or the identity.  LagArgs: the recursion C_{k+1} = step_k(C_k) of the mean equation with b = 0 from
// every anchor to the end of the grid, the kept rows stored
struct LagStartArgs {
  enum Layout { Identity, Whole, Packed, TimeMajor };
  int D, Np, batch, n_anchor, layout, bpad;
  const double* S;          // Whole: [B][Np][D][D]; Packed: [B][Np][D (D + 1) / 2] (OdeArgs::s_packed); TimeMajor: OdeArgs::msT with bpad; Identity: not read
  const int32_t* anchors;   // [n_anchor], on the device
  double* start;            // [B][n_anchor][D][D]
};
struct LagArgs {
  int D, Np, batch, n_anchor, stride, n_keep, method;
  double dt;
  const double* A;          // [B][Np][D][D] (problem stride stride_x)
  size_t stride_x;
  const double* start;      // [B][n_anchor][D][D]
  const int32_t* anchors;   // [n_anchor] grid indices in [0, Np), on the device
  double* out;              // [B][n_anchor][n_keep][D][D]: zero at the kept indices before the anchor
};
hipError_t launch_lag_start(const LagStartArgs& a, hipStream_t st);
hipError_t launch_lag(const LagArgs& a, hipStream_t st);     // D <= kMaxSmallD; hipErrorInvalidValue otherwise
bool lag_grid_fits(int D, int batch, int n_anchor);          // one workgroup (D <= kMaxLaneD: one lane) per (problem, anchor) in grid.x

// Weighted cross moments of stored trajectories (particle_lag.hip): mean [B][n_keep][D] = sum_i W_i X_i(k) and
// cross [B][n_anchor][n_keep][D][D] = sum_i W_i X_i(k) X_i(anchor_rows[q])^T, the paths added in increasing order whatever the launch
struct PathMomentArgs {
  int D, batch, n_paths, n_keep, n_anchor;
  const double* paths;            // [B][n_paths][n_keep][D], as vgpa_sample_paths stores them
  const double* weights;          // [B][n_paths], used as they are; nullptr: 1 / n_paths each
  const int32_t* anchor_rows;     // [n_anchor] rows of the kept axis in [0, n_keep), on the device
  double* mean;
  double* cross;
};
hipError_t launch_path_cross_moments(const PathMomentArgs& g, hipStream_t st);      // D <= kMaxSmallD; hipErrorInvalidValue otherwise
// grid.x: the kept rows (D <= kMaxLaneD: the entries of one anchor's block, 256 per workgroup), grid.y: the anchors, grid.z: the problems
bool path_moments_grid_fits(int D, int batch, int n_keep, int n_anchor);

// The marginal backward smoother (particle_smooth.hip): the smoothing weights of vgpa_particle_backward_moments in place of
// launch_pf_descend's rows c-1 .. 0.  f: the histories h_flag, h_anc, h_clouds, h_lw with M, n_paths, seed, the observation rows and k, the
// grid index of the cut; a: of the filter's arguments the model, theta, A, b, the diagonal R and dt, as launch_pf_backward reads them
struct SmoothArgs {
  int rows;                 // rows per problem of wtab, part and less (> every problem's observation count)
  double* xt;               // [B][n_paths][D] work space: the successors of the cut
  double* rmax;             // [B][n_paths] work space: max_i b_{s,i} ...
  double* rsum;             // ... and sum_i exp(b_{s,i} - max) of every successor s
  double* centre;           // [B][kMaxSmallD] work space: the mean of the cut's cloud (D >= 5: the point the matrix-core scores are centred on)
  double* wtab;             // [B][rows][n_paths]: row c (and less[c]) is launch_pf_descend's
  double* part;             // [B][rows][smooth_column_blocks(n_paths)] the column workgroups' sums of W^2
  double* less;             // [B][rows] 1 / sum_i (W^j_i)^2
};
constexpr int kSmoothRowBlock = 16, kSmoothColBlock = 64;      // successors per workgroup of the row pass, candidates per workgroup of the column pass
// One cut at grid index f.k, behind the cuts above it: every problem with an observation j there gets row j of wtab from row j + 1 -- a
// copy where its cloud was carried on, else x~ (k_ps_successors), the rows' (max, sum) (k_ps_rows) and W^j = W^{j+1} P (k_ps_columns).
// launch_smooth_ess, behind the last cut: less[j] for j < c from the partial sums, in block order (less[j + 1] at a carried cut)
hipError_t launch_smooth_cut(const PfArgs& f, const SampleArgs& a, const SmoothArgs& sm, hipStream_t st);
hipError_t launch_smooth_ess(const PfArgs& f, const SmoothArgs& sm, hipStream_t st);
int smooth_column_blocks(int n_paths);
bool smooth_grid_fits(int D, int n_paths);      // grid.y: the successors 256 / D and 16 per workgroup, the candidates 64 per workgroup

// launchers (each returns hipGetLastError()) -----------------------------------------------------
hipError_t launch_ode_generic(int method, bool fwd, const OdeArgs& a, hipStream_t st);
hipError_t launch_ode_small(int method, bool fwd, const OdeArgs& a, hipStream_t st);     // D <= kMaxLaneD
bool sweep_lane_supported(int model, int D);
hipError_t launch_sweep_lane(int method, const LaneSweepArgs& a, hipStream_t st);
hipError_t launch_theta_lane(const ThetaLaneArgs& a, hipStream_t st);
// msT -> the [B][Np] arrays: all grid points (vgpa_fetch, the separate kernels) or only what the observation terms read
hipError_t launch_ms_untranspose(int D, int Np, int batch, int bpad, const double* msT, double* m, double* S, hipStream_t st);
// observation terms (E_obs, sparse vector jumps) of the fused lane pass: one lane per problem, moments from msT, jumps to jmT
hipError_t launch_obs_lane(const ObsArgs& a, const double* msT, int bpad, double* jmT, hipStream_t st);
hipError_t launch_ode_wave(int method, bool fwd, const OdeArgs& a, hipStream_t st);      // 2 <= D <= kMaxLaneD, few problems
bool ode_mfma_supported(int method, bool fwd, int D);
// helper_roles: sets of helper waves of the fragment-cover kernels (the context's Plan::helper_roles; host-only, like OdeArgs::sym_units)
hipError_t launch_ode_mfma(int method, bool fwd, const OdeArgs& a, int helper_roles, hipStream_t st);
bool sym_stores_q(int method, int D);      // the backward kernel launch_ode_mfma picks for sym_units honours OdeArgs::q_on
bool sym_fuses_grad(int method, int D);    // ... and OdeArgs::grad_on (the gradient assembly on its helper waves)
// Psi_t = (diag(isg) A_t - Q''_t) / 2 in place (A: problem stride strideA, grid-point stride D*D)
// the strict lower triangle of [batch * Np] D x D matrices from their upper one, in place
hipError_t launch_mirror_upper(size_t n_mat, int D, double* m, hipStream_t st);
// n_mat packed lower triangles [D (D + 1) / 2] -> full symmetric D x D matrices
hipError_t launch_unpack_lower(size_t n_mat, int D, const double* packed, double* full, hipStream_t st);
hipError_t launch_psi_from_q(int batch, int Np, int D, size_t strideA, const double* A, const double* isg, size_t isg_stride,
                             double* psi_q, hipStream_t st);   // (isg_stride: D for a per-problem [B][D] isg, else 0)
hipError_t launch_energy(const EnergyArgs& a, hipStream_t st);
hipError_t launch_obs(const ObsArgs& a, hipStream_t st);   // uses the grid-parallel variant when a.part != nullptr
hipError_t launch_obs_dense(const ObsArgs& a, const double* js_const, double* jm_dense, double* js_dense,
                            hipStream_t st);
hipError_t launch_grad(const GradArgs& a, hipStream_t st);
hipError_t launch_reduce(const ReduceArgs& a, hipStream_t st);
// out[p][h] = trapezoid over t of e[p][t][h]
hipError_t launch_trapz_multi(const double* e, int Np, int H, int batch, double dt, double* out, hipStream_t st);
hipError_t launch_edf(const EnergyArgs& a, hipStream_t st);   // dense <df/dx> on request

// One array of a batched context with its per-problem stride: problem p's row is of(p) = rows + p * stride (stride 0: one row, shared by
// the batch).  `+ k` moves into every problem's row alike and keeps the stride.  OutRows: the same for an array the kernels write.
template <typename T> struct Rows {
  const T* rows = nullptr; size_t stride = 0;
  const T* of(int p) const { return rows + (size_t)p * stride; }
  Rows operator+(size_t k) const { return {rows + k, stride}; }
};
template <typename T> struct OutRows {
  T* rows = nullptr; size_t stride = 0;
  T* of(int p) const { return rows + (size_t)p * stride; }
  OutRows operator+(size_t k) const { return {rows + k, stride}; }
  operator Rows<T>() const { return {rows, stride}; }
};

// large-D (per-stage GEMM) single-rank drivers, large_d.hip
namespace ld {
// operands of the single-rank drivers: every array comes with its per-problem stride, stated by the caller (0: shared by the batch)
using In = Rows<double>;
using Out = OutRows<double>;
// One call of the single-rank drivers.  nb problems run side by side in grid.z of every launch; problem p's workspace is
// ws + p * ld_workspace_doubles(D).
struct LdCall {
  int method; double dt; int D, nb;
  bool literal;        // non-symmetric inputs: both products of the slope are formed literally (large_d.hip, run_stage)
  bool library_gemm;   // the plain stage GEMM goes to rocBLAS (lib_gemm.cpp) where it can: one problem, symmetric inputs
  double* ws;
  hipStream_t st;
};
// jumps of the backward recursion: dense arrays over the grid (operator level), or the sparse ones of the observations
struct LdJumps {
  In jm, js;                          // dense: [Np][D], [Np][D][D]; sparse: [M][D] and the constant matrix [D][D]
  const int32_t* obs_idx = nullptr;   // sparse only, on the host: obs_idx[t] = n >= 0: grid point t takes jm[n][:] and js
  static LdJumps dense(In jm, In js) { return {jm, js, nullptr}; }
  static LdJumps sparse(In jm, In js_const, const int32_t* obs_idx_host) { return {jm, js_const, obs_idx_host}; }
};
size_t ld_workspace_doubles(int D);
hipError_t ld_solve_fwd(const LdCall& c, int Np, In A, In b, In m0, In S0, In Sigma, Out m, Out S);
hipError_t ld_solve_bwd(const LdCall& c, int Np, In A, In gm, In gs, const LdJumps& jumps, Out lam, Out psi);
hipError_t ld_bwd_step(const LdCall& c, In At, In Am, In Gt, In Gm, In gt, In gmm, In Pt, In lt, Out Pn, Out ln, In Jn, In jn);
// optional rocBLAS backend of the plain stage GEMM (lib_gemm.cpp), used when LdCall::library_gemm asks for it
bool library_gemm_available();
hipError_t library_gemm(bool transa, int M, int N, int K, const double* A, int lda, const double* B, int ldb, double* C, int ldc,
                        hipStream_t st);
size_t lde_workspace_doubles(int D, int nb);
int lde_batch(int D, double budget_bytes);
hipError_t lde_energy(int D, int Np, double theta, const double* isg, const double* A, const double* b, const double* m,
                      const double* S, double* e_t, double* Ef, double* Edf, double* dEm, double* dEs, int32_t* status,
                      double* ws, int nbmax, hipStream_t st, double* hyp = nullptr, hipStream_t side = nullptr)   /* hyp: [Np][2 D] integrands of dEsde_dtheta | dEsde_dSigma, or nullptr */;
// tg[t] = sum_i isg_i UT-mean(f_i(chi) + (A chi)_i - b_i), the integrand of dF/dtheta, of Np grid points of one problem; writes tg and ws only
hipError_t lde_theta_integrand(int D, int Np, double theta, const double* isg, const double* A, const double* b, const double* m,
                               const double* S, double* tg, int32_t* status, double* ws, int nbmax, hipStream_t st);
hipError_t lde_grad(int D, int Np, double dt, const double* isg, const double* A, const double* b, const double* m,
                    const double* S, const double* lam, const double* psi, const double* Ef, double* gA, double* gB,
                    double* ws, int nbmax, hipStream_t st, const double* isig_dense = nullptr);   // [D][D] Sigma^-1 when it is not diagonal
}  // namespace ld

// device vector algebra for the SCG driver (vecops.hip), segmented over the batch
int vec_blocks_per_seg(long long seglen, int nseg);
hipError_t vec_reduce(int mode, const double* a, const double* b, int nseg, long long seglen, double* scratch, hipStream_t st);
hipError_t vec_axpby(int nseg, long long seglen, const double* alpha_dev, const double* x, const double* beta_dev,
                     const double* y, double* out, hipStream_t st);

// tiny host-side dense helpers (row-major, fp64) ---------------------------------------------------
bool host_cholesky_lower(int n, const double* a, double* l);          // uses the lower triangle of a
void host_lower_inverse(int n, const double* l, double* linv);
bool host_spd_inverse(int n, const double* a, double* ainv, double* logdet);
void host_matmul(int n, const double* a, const double* b, double* c, bool ta, bool tb);

}  // namespace vgpa
