// Euler-Maruyama sample paths of the posterior process dx = (-A_t x + b_t) dt + Sigma^1/2 dW and of the model SDE:
//   x_k = x_{k-1} + dt drift_{k-1}(x_{k-1}) + R xi_k,  R = chol_lower(Sigma dt).
// Four kernels walk the grid:
//   k_sample_small<D, K>   D <= 4, both kinds: one lane per path, the state in registers
//   k_sample_mfma<NT, K>   5 <= D <= 64, posterior kind: a workgroup owns one problem and 64 paths (4 waves x 16 paths); A_k X (and R Xi for a dense
//                          R) on v_mfma_f64_16x16x4_f64 with the 16 paths of a wave as the N side, D padded to NT = 16, 32, 48, 64
//   k_sample_l96           5 <= D <= 64, model kind (Lorenz-96): one lane per path, the state in LDS
//   k_forecast_l96         5 <= D <= 64, the forecast (Lorenz-96): k_sample_l96's lanes and step from a cloud of particles, one wave per
//                          workgroup, the weighted sums of the wave's D x 64 tile of states taken in LDS
// The normals are counter-based (Philox4x32-10 + Box-Muller, vgpa_hip.h): every lane generates exactly the draws it consumes, so no result
// depends on the launch geometry.
// K is the walk (vgpa_internal.h), stated by the host at every launch_sample_walk; every walk but Forecast runs on k_sample_small and
// k_sample_mfma:
// (the properties the kernels branch on for each walk: kWalkTraits below)
//   walk         | what it computes; [the kernels and k_pf_* steps that serve it besides those two]                                 | DESIGN.md
//   Plain        | the paths, every stride-th point stored  [k_sample_l96]                                                          | s.4.8
//   Weighted     | the same paths and, summed where the path is made, the log-ratio of the model SDE's path density to the          | s.4.9
//                | posterior process's and the Gaussian log-likelihood of the observations                                          |
//   Segment      | the grid steps k_begin < k <= k_end of the weighted walk from the particle states in pf_x, the increments added  | s.4.10
//                | to pf_lw, the end states written back  [k_pf_start: the particles and their initial term; k_pf_resample<false>:  |
//                | the step between two segments]                                                                                   |
//   SegmentStats | a segment that also carries each slot's [3][D] row of path statistics  [k_pf_resample<true> gathers the rows by  | s.4.11
//                | ancestor with the states, k_pf_stats_mean reduces them to their self-normalised weighted mean]                   |
//   Replay       | a segment once more: the same states from the same counters, no weight sums, and at every kept grid index the    | s.4.12
//                | workgroup's sums of W x and W x^2 with the descendant weights W  [k_pf_descend pushes the weights back through   |
//                | the stored ancestors, k_pf_gather: the step between two segments, k_pf_moments_sum adds the sums in block order] |
//   Lineage      | K smoothing trajectories of the filter's genealogy in one launch: the unweighted posterior walk, stored as Plain | s.4.13
//                | stores it, each lane drawing with the counter word of the slot its lineage sat in -- one word per stretch between |
//                | two observations of its problem  [k_pf_trace writes the table behind k_pf_pick or the caller's final slots]      |
//   Forecast     | the model SDE carried from the cloud in pf_x at the absolute grid index k_begin to k_end, no weight changing: the | s.4.15
//                | cloud launch sums W x and W x^2 at every kept step as Replay does and writes the end states back; the member      |
//                | launch walks K slots alone, each from its slot's state with its slot's counter word, stored as Plain stores      |
//                | [k_sample_small and k_forecast_l96; k_pf_normalise: W from the log-weights, k_pf_pick: drawn slots,              |
//                | k_pf_moments_sum]                                                                                                |
//   ReplayCov    | the replay with the whole matrix: at every kept grid index the workgroup's sums of W x and of the lower triangle | s.4.16
//                | of W x x^T, above D = 4 as X diag(W) X^T of each wave's 16 states on the matrix pipe  [the replay's steps;        |
//                | k_pf_cov_unpack: the packed sums to mean [D] and second [D][D], both triangles from one entry]                   |
//   Backward     | the lineage walk of a table that backward simulation has drawn: behind every observation of its problem the lane | s.4.17
//                | goes on from the filter's stored particle its next slot was copied from  [k_pf_backward draws the table in the   |
//                | trace's place: at every resampled observation a Gumbel-max draw among all n particles of the stored cloud]       |
//   Conditional  | a segment in which slot 0 of every problem is pinned to a reference trajectory: it draws nothing, is weighted by | s.4.18
//                | the increment the reference implies and follows the reference bit for bit  [k_pf_pin: slot 0 of the start;       |
//                | k_pf_cresample: the step between two segments, multinomial, with ancestor sampling for slot 0; k_pf_ref_fill]    |
//   SegmentEvents| a segment that also carries each slot's [3][D] row of event records (X, T, N) of g_j(x) = s_j (x_j - c_j): the      | s.4.20
//                | largest g, the first grid index with g > 0, the number of such indices  [k_pf_events_start: the rows of grid      |
//                | index 0; k_pf_resample<true>, k_pf_stats_mean as for SegmentStats; k_pf_events_cdf: the first-passage distribution] |
//   ReplayMarginals| the replay with counts in place of sums: at every kept grid index each slot finds, per component, the bin of its  | s.4.21
//                | state on the component's ladder of levels and adds its integer descendant weight to that bin's mass  [the replay's  |
//                | steps; k_pf_quantise: the final weights as integers, k_pf_descend_q: k_pf_descend in 64-bit integer arithmetic]     |
#include "vgpa_internal.h"
#include "dispatch.h"
#include "pf_device.h"

#include <type_traits>

namespace vgpa {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

// ---- D <= 4: one lane per (problem, path) (model_drift: pf_device.h) ---------------------------------------------------------------
// phi_j = d f_j / d theta_a(j) at x, a(j) the one parameter component j's drift depends on
template <int D>
__device__ __forceinline__ void model_phi(int model, const double* x, double* phi) {
  if (model == VGPA_MODEL_OU) { phi[0] = -x[0]; }
  else if (model == VGPA_MODEL_DW) { phi[0] = 4.0 * x[0]; }
  else if (model == VGPA_MODEL_L63) {
    if constexpr (D == 3) { phi[0] = x[1] - x[0]; phi[1] = x[0]; phi[2] = -x[2]; }
  } else {
#pragma unroll
    for (int i = 0; i < D; i++) phi[i] = 1.0;
  }
}

// the observation row of one problem as a weighted kernel walks it: next = the grid index of the next observation, or -1 behind the last one
struct ObsCursor {
  const int64_t* t;
  int n, cur, next;
  __device__ __forceinline__ ObsCursor() : t(nullptr), n(0), cur(0), next(-1) {}
  __device__ __forceinline__ ObsCursor(const SampleArgs& a, uint32_t p)
      : t(a.obs_t + (size_t)p * a.obs_t_stride), n(a.n_obs_v ? a.n_obs_v[p] : a.n_obs), cur(0) { next = n > 0 ? (int)t[0] : -1; }
  __device__ __forceinline__ void advance() { next = ++cur < n ? (int)t[cur] : -1; }
  __device__ __forceinline__ void skip_through(int k) { while (next >= 0 && next <= k) advance(); }      // to the first index > k
};

// (y_n - x)^T Q (y_n - x) of problem p
template <int D>
__device__ __forceinline__ double obs_form(const SampleArgs& a, uint32_t p, int n, const double* x) {
  const double* y = a.obs_y + (size_t)p * a.obs_y_stride + (size_t)n * D;
  const double* Q = a.Q + (size_t)p * a.Q_stride;
  double r[D], s = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++) r[i] = y[i] - x[i];
#pragma unroll
  for (int i = 0; i < D; i++) {
    double qr = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) qr += Q[i * D + j] * r[j];
    s += r[i] * qr;
  }
  return s;
}

__device__ __forceinline__ double obs_constant(const SampleArgs& a, uint32_t p) {
  return a.obs_const_scale * (a.obs_const_v ? a.obs_const_v[p] : a.obs_const);
}

// What a walk's kernels take: SampleArgs, and for Conditional alone the reference trajectories behind it -- no other walk's arguments,
// registers or code know of the pointer.
struct ConditionalArgs : SampleArgs {
  const double* pf_ref;      // [B][Np][D]
};
// ... and for SegmentEvents alone the levels and sides of its events
struct EventArgs : SampleArgs {
  const double* ev_level;    // [B][D]
  const int32_t* ev_side;    // [B][D] +1 / -1
};
// ... and for ReplayMarginals alone the ladders, the integer weights and the masses
struct MarginalWalkArgs : SampleArgs {
  const double* mg_level;            // [B][D][L]
  int mg_L;
  const uint64_t* mg_qtab;           // [B][pf_rows][n_paths]
  unsigned long long* mg_mass;       // [B][n_keep][D][L + 1]
};
template <Walk K> struct WalkArgsOf { using type = SampleArgs; };
template <> struct WalkArgsOf<Walk::Conditional> { using type = ConditionalArgs; };
template <> struct WalkArgsOf<Walk::SegmentEvents> { using type = EventArgs; };
template <> struct WalkArgsOf<Walk::ReplayMarginals> { using type = MarginalWalkArgs; };
template <Walk K> using WalkArgs = typename WalkArgsOf<K>::type;

// What the two kernels branch on, per walk.  Four properties a walk has or has not, and three choices that exclude one another by type:
//   weighted   the walk of the weighted kind (posterior drift, diagonal R)
//   segment    it runs (k_begin, k_end] from and to pf_x
//   forecast   the model's drift from the cloud in pf_x (k_sample_small only)
//   pinned     slot 0 is pinned to pf_ref of ConditionalArgs (a segment)
//   carry      the [3][D] row a slot carries in pf_stats (a segment): Carry::Stats the path statistics, Carry::Events the event records of
//              EventArgs' levels and sides
//   kept       what happens at a kept grid index (a segment launched as the replay): Kept::Moments the sums of W x and W x^2, Kept::Covariance
//              of W x and the whole W x x^T, Kept::Marginals MarginalWalkArgs' integer weights added to the bins of the states, no sum formed
//   words      where the counter words come from: Words::Own the lane's own index, Words::Table pf_slots, Words::TableReload pf_slots with the
//              state reloaded from the filter's histories behind every observation
// and, derived, WS(): the weight sums are formed.  The twelve rows are all there is: no other combination can be instantiated.
enum class Kept { None, Moments, Covariance, Marginals };      // (the words of the host's Behind for the same passes)
enum class Words { Own, Table, TableReload };
struct WalkTraits {
  bool weighted = false, segment = false, forecast = false, pinned = false;
  Carry carry = Carry::None;
  Kept kept = Kept::None;
  Words words = Words::Own;
  constexpr bool WS() const { return weighted && kept == Kept::None; }
  constexpr bool by_problem() const { return kept != Kept::None || forecast; }      // launched with the problem in grid.x, the slots in grid.y
};
constexpr WalkTraits kWalkTraits[] = {      // in the order of Walk
    /* Plain           */ {},
    /* Weighted        */ {.weighted = true},
    /* Segment         */ {.weighted = true, .segment = true},
    /* SegmentStats    */ {.weighted = true, .segment = true, .carry = Carry::Stats},
    /* Replay          */ {.weighted = true, .segment = true, .kept = Kept::Moments},
    /* Lineage         */ {.words = Words::Table},
    /* Forecast        */ {.forecast = true},
    /* ReplayCov       */ {.weighted = true, .segment = true, .kept = Kept::Covariance},
    /* Backward        */ {.words = Words::TableReload},
    /* Conditional     */ {.weighted = true, .segment = true, .pinned = true},
    /* SegmentEvents   */ {.weighted = true, .segment = true, .carry = Carry::Events},
    /* ReplayMarginals */ {.weighted = true, .segment = true, .kept = Kept::Marginals}};

// Walk::ReplayMarginals: the bin of x on a strictly increasing ladder of L levels, #{l: c_l < x}, by bisection on fp64 compares alone (at most 6
// for L <= 63; a NaN compares false everywhere: bin 0), and the slot's weight added to that bin of row [L + 1]
__device__ __forceinline__ void marginal_add(const double* lev, int L, unsigned long long* row, double x, unsigned long long qw) {
  int lo = 0, hi = L;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lev[mid] < x) lo = mid + 1; else hi = mid;
  }
  atomicAdd(row + lo, qw);
}

// ---- the walks' rules, each stated once for both kernels ------------------------------------------------------------------------------
// Carry::Events: behind step k, with d = x_j(k) - c_j (one subtraction) and g = d or -d by the side: X_j = fmax(X_j, g); where g > 0,
// T_j = min(T_j, k) and N_j += 1
__device__ __forceinline__ void event_step(double x, double level, bool below, int k, double& X, int& T, int& N) {
  const double d = x - level, g = below ? -d : d;
  X = fmax(X, g);
  if (g > 0.0) { T = min(T, k); N += 1; }
}
// Carry::Stats: a step's r = dt d + eta (d = g - f) of one component: Q += r^2 / dt, G += phi r.  (H += dt phi^2 is k_sample_small's own:
// with phi = 1 k_sample_mfma writes H as a constant.)
__device__ __forceinline__ void stats_step(double dt, double d, double eta, double phi, double& Q, double& G) {
  const double r = dt * d + eta;
  Q += r * r / dt; G += phi * r;
}
// a slot's [3][D] carried row of pf_stats (Carry::Stats: Q, G, H; Carry::Events: X, T, N), slot = p n_paths + path: member m of component i
__device__ __forceinline__ double& carried(const SampleArgs& a, size_t slot, int D, int m, int i) { return a.pf_stats[slot * 3 * D + m * D + i]; }
// Words::TableReload: the particle slot `word` was copied from at observation j of problem p: pf_clouds[p][j][pf_hanc[p][j][word]]
__device__ __forceinline__ const double* backward_source(const SampleArgs& a, uint32_t p, int j, uint32_t word, int D) {
  const size_t hj = (size_t)p * a.pf_M + j;
  return a.pf_clouds + (hj * a.pf_n + (size_t)a.pf_hanc[hj * a.pf_n + word]) * D;
}
// the replay: a segment lies in one stretch of its problem -- the observations behind it count the row of its weights in a table
// [B][pf_rows][n_paths] (pf_wtab, mg_qtab): the entry of `path`
template <class V>
__device__ __forceinline__ V stretch_weight(const SampleArgs& a, const V* table, uint32_t p, int stretch, uint32_t path) {
  return table[((size_t)p * a.pf_rows + stretch) * a.n_paths + path];
}
// the replay: the next kept grid index (a multiple of the stride) and its slot among the n_keep results
struct KeptCursor {
  long long k = 0, slot = 0;
  __device__ __forceinline__ void first_behind(int k_begin, int stride) { slot = ((long long)k_begin + stride) / stride; k = slot * stride; }
};
// Kept::Marginals: component i of a state x_i at kept slot `slot` of problem p: the weight qw to its bin of mass[p][slot][i][L + 1], on the
// ladder level[p][i][L]
__device__ __forceinline__ const double* marginal_ladder(const MarginalWalkArgs& a, uint32_t p, int i, int D) { return a.mg_level + ((size_t)p * D + i) * a.mg_L; }
__device__ __forceinline__ unsigned long long* mass_row(const MarginalWalkArgs& a, uint32_t p, long long slot, int i, int D) {
  return a.mg_mass + (((size_t)p * a.n_keep + (size_t)slot) * D + i) * ((size_t)a.mg_L + 1);
}

// What each walk does in k_sample_small, by the property of kWalkTraits that brings it in.
// Weighted (weighted): posterior kind, diagonal R: both drifts at x_{k-1}, d = g - f, and per step -sum_i d_i (eta_i + dt d_i / 2) / Sigma_ii with
// 1 / Sigma_ii = dt / R_ii^2; the observation term at the lane's own problem's times.
// Segment (segment): the weighted walk over (k_begin, k_end] from and to pf_x, the sums added to pf_lw; nothing else is stored.
// SegmentStats (Carry::Stats): a segment that adds its steps to the slot's row of pf_stats (carried): Q_i and G_i by stats_step,
// H_i += dt phi_i^2.
// Replay (Kept::Moments): a segment launched with the problem in blockIdx.x and 256 slots per workgroup.  The states only (no model drift, no sums, pf_lw
// untouched); at a kept k the lanes' W x_i and (W x_i) x_i are added over the wave by a butterfly and over the four waves through four
// LDS words per value (two sets, alternating: one barrier per kept k), in that fixed order.  A lane behind the last slot walks from 0
// with the last slot's counters and weight 0 and stores nothing.
// ReplayCov (Kept::Covariance): the replay with D + D (D + 1) / 2 values per kept k in place of 2 D: W x_i, then (W x_a) x_b for b <= a by rows -- the same
// butterfly, LDS words and order; the diagonal entries are the replay's own (W x_i) x_i.
// Lineage (Words::Table): the unweighted posterior walk of lane m = `path`, whose counter word is not m but the entry of its column of pf_slots for the
// stretch it is in: row 0 for the start, the next row each time the walk has completed an observation index of the lane's own problem (an
// observation at index 0: before step 1).  No model drift, no sums.
// Backward (Words::TableReload): the lineage walk, and where it changes its counter word -- behind the completed observation j of its problem,
// whose point has been stored -- the state becomes backward_source's particle of the new word (pf_hanc is the identity where the cloud was
// carried on: the reload then changes no bit).
// Forecast (forecast): launched as the replay is (the problem in blockIdx.x, 256 lanes per workgroup).  The model's drift alone, step h = 1 .. k_end -
// k_begin drawn at the absolute grid index k_begin + h, from the slot's state in pf_x.  The cloud launch (pf_part set): lane = slot, the
// replay's sums with W = pf_wtab at h = 0, stride, ..., the end state back to pf_x.  The member launch (out, pf_slots set): lane m starts from
// slot pf_slots[p][m], draws with that slot's word and stores as Plain stores.  A lane behind the last one walks the last one again with
// weight 0 and stores nothing.
// Conditional (pinned): a segment in which the lane of slot 0 holds x_{k-1} = pf_ref[p][k-1] bit for bit, draws nothing and puts
// eta* = (ref_k - x_{k-1}) - dt g(x_{k-1}) where the other lanes put R xi: the step term, the observation term and the sums are the segment's; its
// state becomes ref_k as loaded (D loads per step for that one lane).  Every other lane is the segment's, bit for bit.
// SegmentEvents (Carry::Events): a segment, bit for bit, that behind every step k takes event_step for each component.  The slot's row of
// pf_stats (carried) is read at the segment's entry and written at
// its exit, T and N as the doubles the integers are; in between they are 32-bit integers.  (The row of grid index 0 is k_pf_events_start's.)
// ReplayMarginals (Kept::Marginals): the replay's launch, states and kept indices; no weight is a double and nothing is summed over lanes.  At a
// kept k a live lane whose integer weight Q (stretch_weight of mg_qtab) is not 0 adds Q to mass_row(p, k', i)[bin(x_i)] for each of its
// components with one 64-bit integer atomic per component, the ladder read from global memory.  Integer addition is associative: the masses
// do not depend on the order the atomics arrive in.
// Walk::Backward: x = the particle slot `word` was copied from at observation j of problem p
template <int D>
__device__ __forceinline__ void backward_reload(const SampleArgs& a, uint32_t p, int j, uint32_t word, double* x) {
  const double* src = backward_source(a, p, j, word, D);
#pragma unroll
  for (int i = 0; i < D; i++) x[i] = src[i];
}

template <int D, Walk K>
__global__ __launch_bounds__(256) void k_sample_small(WalkArgs<K> a) {
  constexpr WalkTraits T = kWalkTraits[(int)K];
  constexpr bool weighted = T.weighted, segment = T.segment, forecast = T.forecast, pinned = T.pinned, sums = T.WS();
  constexpr Carry carry = T.carry;
  constexpr Kept kept = T.kept;
  constexpr bool table = T.words != Words::Own, replay = kept != Kept::None;
  constexpr int NV = kept == Kept::Covariance ? D + D * (D + 1) / 2 : 2 * D;      // values a kept k reduces
  size_t gid;
  uint32_t p, path;
  bool live = true;
  if constexpr (T.by_problem()) {
    const uint32_t slot = blockIdx.y * 256 + threadIdx.x;
    live = slot < (uint32_t)a.n_paths;
    p = blockIdx.x; path = live ? slot : (uint32_t)a.n_paths - 1;
    gid = (size_t)p * a.n_paths + path;
  } else {
    gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (size_t)a.batch * a.n_paths) return;
    p = (uint32_t)(gid / a.n_paths); path = (uint32_t)(gid % a.n_paths);
  }
  uint32_t word = path;      // the counter word of the lane's draws
  const int32_t* lin = nullptr;
  if constexpr (table) { lin = a.pf_slots + (size_t)p * a.pf_slot_rows * a.n_paths + path; word = (uint32_t)lin[0]; }
  if constexpr (forecast) { if (a.pf_slots) word = (uint32_t)a.pf_slots[gid]; }
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  constexpr int NP = (D + 1) / 2;
  // kept points wait in LDS (slot-major, thread fastest: no conflicts) until NBUF of them -- 16 doubles for D = 1, 2, 4, 15 for D = 3 -- go out as
  // one run of consecutive stores into the lane's row: whole 128-byte lines once the row has reached a line boundary
  constexpr int NBUF = 16 / D;
  __shared__ double stage[NBUF * D * 256];
  double* sg = stage + threadIdx.x;
  double R[D * D], th[kMaxTheta], x[D], z[2 * NP];
  {
    const double* Rp = a.R + (size_t)p * a.R_stride;
#pragma unroll
    for (int e = 0; e < D * D; e++) R[e] = Rp[e];
#pragma unroll
    for (int i = 0; i < kMaxTheta; i++) th[i] = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta + i] : a.theta[i];
  }
  if constexpr (forecast) {
#pragma unroll
    for (int i = 0; i < D; i++) x[i] = a.pf_x[((size_t)p * a.pf_n + word) * D + i];
  } else if constexpr (segment) {
#pragma unroll
    for (int i = 0; i < D; i++) x[i] = !replay || live ? a.pf_x[gid * D + i] : 0.0;
  } else if (a.x0) {
#pragma unroll
    for (int i = 0; i < D; i++) x[i] = a.x0[(size_t)p * D + i];
  } else {
    const double* m0 = a.m0 + (size_t)p * a.m0_stride;
    const double* L0 = a.L0 + (size_t)p * a.L0_stride;
#pragma unroll
    for (int j = 0; j < NP; j++) normal_pair(k0, k1, 0u, word, p, (uint32_t)j, &z[2 * j], &z[2 * j + 1]);
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j <= i; j++) s += L0[i * D + j] * z[j];
      x[i] = m0[i] + s;
    }
  }
  const bool store = forecast ? live && a.out != nullptr : !segment && (!weighted || a.out != nullptr);
  double* o = store ? a.out + gid * (size_t)a.n_keep * D : nullptr;
  if (store) {
#pragma unroll
    for (int i = 0; i < D; i++) o[i] = x[i];
    o += D;
  }
  double isg[D], pw = 0.0, ow = 0.0;
  ObsCursor oc;
  if constexpr (sums) {
    oc = ObsCursor(a, p);
#pragma unroll
    for (int i = 0; i < D; i++) {
      isg[i] = a.dt / (R[i * D + i] * R[i * D + i]);
      if constexpr (!segment) a.start[gid * D + i] = x[i];
    }
    if constexpr (segment) { if (!a.seg_first) oc.skip_through(a.k_begin); }
    if (oc.next == 0) { ow += obs_form<D>(a, p, oc.cur, x); oc.advance(); }
  }
  if constexpr (table) {
    oc = ObsCursor(a, p);
    if (oc.next == 0) {
      oc.advance(); word = (uint32_t)lin[(size_t)oc.cur * a.n_paths];
      if constexpr (T.words == Words::TableReload) backward_reload<D>(a, p, 0, word, x);
    }
  }
  // the replay: the slot's weight of the segment's stretch (Kept::Marginals: the integer one), the first kept index behind k_begin
  double wt = 0.0;
  double* red = nullptr;
  int par = 0;
  KeptCursor next_kept;
  unsigned long long qw = 0;
  if constexpr (replay) {
    oc = ObsCursor(a, p);
    if (!a.seg_first) oc.skip_through(a.k_begin);
    if constexpr (kept == Kept::Marginals) qw = live ? stretch_weight(a, a.mg_qtab, p, oc.cur, path) : 0ull;
    else {
      __shared__ double red_lds[2 * NV * 4];
      red = red_lds;
      wt = live ? stretch_weight(a, a.pf_wtab, p, oc.cur, path) : 0.0;
    }
    next_kept.first_behind(a.k_begin, a.stride);
  }
  if constexpr (forecast) {      // (next_kept.k counts steps: h = k + 1 behind step k of the loop below)
    __shared__ double red_lds[2 * 2 * D * 4];
    red = red_lds;
    wt = live && a.pf_wtab ? a.pf_wtab[gid] : 0.0;
    next_kept.slot = 1; next_kept.k = a.stride;
  }
  // the action at a kept index, by the walk's `kept` (the forecast's cloud launch: the moments): Kept::Marginals counts, the others reduce
  auto at_kept = [&](long long slot) {
    if constexpr (kept == Kept::Marginals) {      // count: the slot's weight to the bin of each of its components
      if (qw != 0) {
#pragma unroll
        for (int i = 0; i < D; i++) marginal_add(marginal_ladder(a, p, i, D), a.mg_L, mass_row(a, p, slot, i, D), x[i], qw);
      }
    } else {      // reduce: the workgroup's sums over its slots, NV values
      double v[NV];
      if constexpr (kept == Kept::Covariance) {
#pragma unroll
        for (int i = 0; i < D; i++) v[i] = wt * x[i];
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) v[D + i * (i + 1) / 2 + j] = v[i] * x[j];
      } else {
#pragma unroll
        for (int i = 0; i < D; i++) { v[i] = wt * x[i]; v[D + i] = v[i] * x[i]; }
      }
      double* r = red + par * 4 * NV;
#pragma unroll
      for (int e = 0; e < NV; e++) {
        v[e] = wave_sum(v[e]);
        if ((threadIdx.x & 63) == 0) r[e * 4 + (threadIdx.x >> 6)] = v[e];
      }
      __syncthreads();
      if (threadIdx.x < NV) {
        const double* q4 = r + threadIdx.x * 4;
        a.pf_part[(((size_t)p * gridDim.y + blockIdx.y) * a.n_keep + (size_t)slot) * NV + threadIdx.x] = ((q4[0] + q4[1]) + q4[2]) + q4[3];
      }
      par ^= 1;
    }
  };
  if constexpr (replay) { if (a.seg_first) at_kept(0); }
  if constexpr (forecast) { if (a.pf_part) at_kept(0); }
  constexpr bool stats = carry == Carry::Stats, events = carry == Carry::Events;
  double sq[stats ? D : 1], sg1[stats ? D : 1], sh[stats ? D : 1], phi[stats ? D : 1];
  if constexpr (stats) {
#pragma unroll
    for (int i = 0; i < D; i++) { sq[i] = carried(a, gid, D, 0, i); sg1[i] = carried(a, gid, D, 1, i); sh[i] = carried(a, gid, D, 2, i); }
  }
  double ec[events ? D : 1], ex[events ? D : 1];      // Carry::Events: the levels, the slot's row; the sides as a bit per component
  int et[events ? D : 1], en[events ? D : 1], eneg = 0;
  if constexpr (events) {
#pragma unroll
    for (int i = 0; i < D; i++) {
      ec[i] = a.ev_level[(size_t)p * D + i];
      eneg |= a.ev_side[(size_t)p * D + i] < 0 ? 1 << i : 0;
      ex[i] = carried(a, gid, D, 0, i); et[i] = (int)carried(a, gid, D, 1, i); en[i] = (int)carried(a, gid, D, 2, i);
    }
  }
  const double* A = a.A + (size_t)p * a.stride_x;
  const double* bv = a.b + (size_t)p * a.stride_x;
  int until = a.stride, slot = 0;
  // (the forecast counts its steps from 0: k_begin + h may be the last index an int holds)
  const int k_first = forecast ? 0 : segment ? a.k_begin + 1 : 1, k_stop = forecast ? a.k_end - a.k_begin : segment ? a.k_end + 1 : a.Np;
  bool pin = false;      // pinned: the lane of slot 0
  const double* ref = nullptr;
  if constexpr (pinned) { pin = path == 0; ref = a.pf_ref + (size_t)p * a.Np * D; }
  for (int k = k_first; k < k_stop; k++) {
    double f[D], fm[D];
    if constexpr (sums) model_drift<D>(a.model, th, x, fm);
    if (!forecast && (weighted || table || a.kind == VGPA_PATHS_POSTERIOR)) {
      const double* Ak = A + (size_t)(k - 1) * D * D;
      const double* bk = bv + (size_t)(k - 1) * D;
#pragma unroll
      for (int i = 0; i < D; i++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) s += Ak[i * D + j] * x[j];
        f[i] = bk[i] - s;
      }
    } else {
      model_drift<D>(a.model, th, x, f);
    }
    double xr[pinned ? D : 1];      // pinned: ref_k of the pinned lane
    if constexpr (pinned) {
#pragma unroll
      for (int i = 0; i < D; i++) { xr[i] = pin ? ref[(size_t)k * D + i] : 0.0; z[i] = 0.0; }
    }
    if (!pinned || !pin) {
#pragma unroll
      for (int j = 0; j < NP; j++) normal_pair(k0, k1, forecast ? (uint32_t)a.k_begin + (uint32_t)k + 1u : (uint32_t)k, word, p, (uint32_t)j, &z[2 * j], &z[2 * j + 1]);
    }
    if constexpr (stats) model_phi<D>(a.model, x, phi);
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j <= i; j++) s += R[i * D + j] * z[j];
      if constexpr (pinned) { if (pin) s = (xr[i] - x[i]) - a.dt * f[i]; }      // the increment the reference implies, in R xi's place
      if constexpr (sums) { const double d = f[i] - fm[i]; pw -= isg[i] * d * (s + 0.5 * a.dt * d); }
      if constexpr (stats) { stats_step(a.dt, f[i] - fm[i], s, phi[i], sq[i], sg1[i]); sh[i] += a.dt * (phi[i] * phi[i]); }
      x[i] = (x[i] + a.dt * f[i]) + s;
      if constexpr (pinned) { if (pin) x[i] = xr[i]; }      // (as loaded, not as recomputed)
      if constexpr (events) event_step(x[i], ec[i], (eneg >> i) & 1, k, ex[i], et[i], en[i]);
    }
    if constexpr (sums) {
      if (k == oc.next) { ow += obs_form<D>(a, p, oc.cur, x); oc.advance(); }
    }
    if constexpr (replay) { if (k == next_kept.k) { at_kept(next_kept.slot++); next_kept.k += a.stride; } }
    if constexpr (table) {
      if (k == oc.next) { oc.advance(); word = (uint32_t)lin[(size_t)oc.cur * a.n_paths]; }
    }
    if constexpr (forecast) {
      if (a.pf_part && k + 1 == next_kept.k) { at_kept(next_kept.slot++); next_kept.k += a.stride; }
    }
    if (store && --until == 0) {
      until = a.stride;
#pragma unroll
      for (int i = 0; i < D; i++) sg[(slot * D + i) * 256] = x[i];
      if (++slot == NBUF) {
        slot = 0;
#pragma unroll
        for (int e = 0; e < NBUF * D; e++) o[e] = sg[e * 256];
        o += NBUF * D;
      }
    }
    if constexpr (T.words == Words::TableReload) {      // (the step completed observation oc.cur - 1 of the lane's problem; its point is stored: now the state is replaced)
      if (oc.cur > 0 && (int)oc.t[oc.cur - 1] == k) backward_reload<D>(a, p, oc.cur - 1, word, x);
    }
  }
  for (int e = 0; e < slot * D; e++) o[e] = sg[e * 256];
  if constexpr (segment && sums) a.pf_lw[gid] += pw - 0.5 * ow;
  if constexpr (segment || forecast) {      // back to pf_x: every live slot's end state (the forecast: of the cloud launch alone)
    if (forecast ? live && a.pf_part : live) {
#pragma unroll
      for (int i = 0; i < D; i++) a.pf_x[gid * D + i] = x[i];
    }
  }
  if constexpr (stats) {
#pragma unroll
    for (int i = 0; i < D; i++) { carried(a, gid, D, 0, i) = sq[i]; carried(a, gid, D, 1, i) = sg1[i]; carried(a, gid, D, 2, i) = sh[i]; }
  }
  if constexpr (events) {
#pragma unroll
    for (int i = 0; i < D; i++) { carried(a, gid, D, 0, i) = ex[i]; carried(a, gid, D, 1, i) = (double)et[i]; carried(a, gid, D, 2, i) = (double)en[i]; }
  }
  if constexpr (weighted && !segment) { a.logw[2 * gid] = pw; a.logw[2 * gid + 1] = -0.5 * ow - obs_constant(a, p); }
}

// ---- 5 <= D <= 64, posterior kind ---------------------------------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds C[(l >> 4) + 4 r][l & 15] in r = 0..3.
// LDS: As [NT][LDA] A_{k-1} row-major, zero beyond D (LDA = 2 mod 32 doubles: the 16 rows x 2 columns a half wave reads fall into
// 32 different bank pairs); bs [NT]; Rs [NT][LDA] (dense R); Xs / Zs [4 waves][NT][16]: the state / the normals as the B operand reads them.
template <int NT> struct MfmaShape {
  static constexpr int LDA = NT <= 32 ? 34 : 66;
  static constexpr int MT = NT / 16, KT = NT / 4;
  static constexpr int NPF = (NT * NT + 255) / 256;      // doubles of A_k a thread carries from its load to the LDS write
  static constexpr size_t lds_doubles(bool dense) { return (size_t)NT * LDA * (dense ? 2 : 1) + NT + 2 * 4 * NT * 16; }
};

// the normals of grid index k in the C layout of this lane: rows mt * 16 + q + 4 r.  A pair (2j, 2j + 1) spans the lanes q and q ^ 1: the even one
// draws the pairs of r = 0, 1, the odd one those of r = 2, 3, and each hands the half it does not use to its partner.
template <int NT>
__device__ __forceinline__ void normals_c(uint32_t k0, uint32_t k1, uint32_t k, uint32_t path, uint32_t p, int D, int q, double (*z)[4]) {
  const int odd = q & 1, qe = q & ~1;
#pragma unroll
  for (int mt = 0; mt < NT / 16; mt++) {
    double mine[2], other[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int row = mt * 16 + qe + 4 * (2 * odd + h);      // the even row of the pair
      double c = 0.0, s = 0.0;
      if (row < D) normal_pair(k0, k1, k, path, p, (uint32_t)(row >> 1), &c, &s);
      mine[h] = odd ? s : c;
      other[h] = __shfl_xor(odd ? c : s, 16);
    }
    z[mt][0] = odd ? other[0] : mine[0]; z[mt][1] = odd ? other[1] : mine[1];
    z[mt][2] = odd ? mine[0] : other[0]; z[mt][3] = odd ? mine[1] : other[1];
  }
}

// What each walk does in k_sample_mfma, by the same properties (the rules above are shared; the row nest mt, r is written out in every user).
// Weighted (weighted): Lorenz-96, diagonal R.  At step k the lane holds rows mt * 16 + q + 4 r of x_{k-1}, of g = bs - acc and of eta = nz; the model
// drift f_i reads rows (i + 1) mod D, (i - 2) mod D, (i - 1) mod D of the path's column of Xs.  Each lane sums its rows over time; the four
// q-lanes of a path are added once at the end.  The observation term is evaluated from Xs at the problem's observation times, which a
// workgroup walks with one cursor.
// Segment (segment): as in k_sample_small; A_{k_begin} is the first matrix loaded, and the end states leave through `put` as [path][D].
// SegmentStats (Carry::Stats): the lane adds stats_step with phi = 1 (Lorenz-96) of its own rows to Q and G of the path's row of pf_stats,
// read at the segment's entry and written at its exit; H_j = dt k_end, the constant dt times the steps walked so far, is written and not
// summed.
// Replay (Kept::Moments): the states only.  At a kept k every lane multiplies its rows of x_k by its path's weight (0 behind the last path), four
// cross-lane steps add the 16 paths of the wave, the lanes of path column 0 put their rows into red [4 waves][2][NT] -- the Zs region,
// which a segment does not use --, and behind the next barrier the walk has anyway (the first of the next step, or one behind the loop)
// thread t < 2 D adds the four waves in order and stores moment t / D of component t mod D.
// ReplayCov (Kept::Covariance): the replay, but at a kept k the wave's C_w = sum_{c < 16} W_c x_c x_c^T goes over the matrix pipe.  The wave
// copies its 16 states into its own quarter of the Zs region with the columns of row i rotated by 2 (i >> 1), so that the transposed read of
// the operands -- lane (j16, q) takes row mt 16 + j16, path 4 kk + q -- finds the 32 lanes of a half wave on 32 different bank pairs (from Xs,
// at its row stride of 16 doubles, they sit on 4: an 8-way conflict), and holds them as xa [MT][4].  Tile (ti, tj <= ti) is four products
// A = xa[ti][kk], B = W xa[tj][kk], the weight of path 4 kk + q fetched from its lane; MT tiles at a time go to the wave's quarter, now its
// MT tile slots, and behind a barrier thread t adds entry t of each slot over the four waves in wave order and stores the entries of the
// lower triangle below D.  The mean keeps the replay's cross-lane sum, its [4 waves][NT] words behind the Zs region.  Barriers per kept k:
// 2 ceil(T / MT) - 1 with T = MT (MT + 1) / 2 tiles, that is 1, 3, 3, 5 at NT = 16, 32, 48, 64; none in a step that keeps nothing.  The last
// round's slots are read before the next step's barriers, the next kept k writes them behind those.
// Lineage (Words::Table): as in k_sample_small (diagonal R): every lane of a workgroup belongs to one problem, so all of them change their counter words
// behind the same steps.  A lane behind the last lineage walks the last one again and stores nothing.
// Backward (Words::TableReload): as in k_sample_small; the reload is a gather of the lane's own rows of its path's new particle into the accumulator layout, which
// then goes to Xs as every step's result does, behind the store of the completed observation's point and in front of one more barrier.
// Conditional (pinned): as in k_sample_small.  Slot 0 is path column 0 of wave 0 of workgroup (p, 0): its four lanes request their rows of ref_k
// with the step's A_k, put eta* into nz before the weight term is formed and ref_k into x before the step's own write of x to Xs -- no
// barrier is added, and the model drift of the next step reads the reference from the column of Xs as it reads every other path.
// SegmentEvents (Carry::Events): as in k_sample_small, lane-local: the lane holds X, T, N of its own rows mt * 16 + q + 4 r of its path's row of pf_stats, read
// at the segment's entry, updated behind the step's own update of x and written at its exit; the levels lie in LDS as bs does ([NT], in the
// Zs region) and are read where they are used.  A row beyond D and a lane behind the last path compute on zeros and store nothing.  No
// barrier or cross-lane step is added.
template <int NT, Walk K>
__global__ __launch_bounds__(256) void k_sample_mfma(WalkArgs<K> a) {
  constexpr WalkTraits T = kWalkTraits[(int)K];
  constexpr bool weighted = T.weighted, segment = T.segment, pinned = T.pinned, sums = T.WS();
  constexpr bool stats = T.carry == Carry::Stats, events = T.carry == Carry::Events;
  constexpr Kept kept = T.kept;
  constexpr bool table = T.words != Words::Own, replay = kept != Kept::None;
  using Sh = MfmaShape<NT>;
  constexpr int LDA = Sh::LDA, MT = Sh::MT, KT = Sh::KT, NPF = Sh::NPF;
  extern __shared__ double lds[];
  const int D = a.D, DD = D * D, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j16 = lane & 15, q = lane >> 4;
  const bool dense = !weighted && !table && !a.R_diag;      // (the weighted walks and the lineage walk are launched with diagonal factors only)
  double* As = lds;
  double* bs = As + NT * LDA;
  double* Rs = bs + NT;
  double* Xs = Rs + (dense ? NT * LDA : 0) + w * NT * 16;
  double* Zs = Xs + 4 * NT * 16;
  const uint32_t p = blockIdx.x, path = blockIdx.y * 64 + w * 16 + j16;
  uint32_t word = path;      // the counter word of the lane's draws
  const int32_t* lin = nullptr;
  if constexpr (table) {
    lin = a.pf_slots + (size_t)p * a.pf_slot_rows * a.n_paths + (path < (uint32_t)a.n_paths ? path : (uint32_t)a.n_paths - 1);
    word = (uint32_t)lin[0];
  }
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  const double* A = a.A + (size_t)p * a.stride_x;
  const double* bv = a.b + (size_t)p * a.stride_x;
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const int k_first = segment ? a.k_begin + 1 : 1, k_stop = segment ? a.k_end + 1 : a.Np;

  for (int e = tid; e < NT * LDA * (dense ? 2 : 1) + NT; e += 256) lds[e] = 0.0;
  __syncthreads();
  for (int e = tid; e < DD; e += 256) {
    As[(e / D) * LDA + e % D] = A[(size_t)(k_first - 1) * DD + e];
    if (dense) Rs[(e / D) * LDA + e % D] = Rp[e];
  }
  if (tid < D) bs[tid] = bv[(size_t)(k_first - 1) * D + tid];

  double x[MT][4], rd[MT][4], z[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = mt * 16 + q + 4 * r;
      rd[mt][r] = (!dense && row < D) ? Rp[row * D + row] : 0.0;
    }
  if constexpr (segment) {
    const bool live = path < (uint32_t)a.n_paths;      // (a lane behind the last path walks zeros and stores nothing)
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        x[mt][r] = live && row < D ? a.pf_x[((size_t)p * a.n_paths + path) * D + row] : 0.0;
      }
  } else if (a.x0) {
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        x[mt][r] = row < D ? a.x0[(size_t)p * D + row] : 0.0;
      }
  } else {
    const double* m0 = a.m0 + (size_t)p * a.m0_stride;
    const double* L0 = a.L0 + (size_t)p * a.L0_stride;
    normals_c<NT>(k0, k1, 0u, word, p, D, q, z);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) Zs[(mt * 16 + q + 4 * r) * 16 + j16] = z[mt][r];
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        double s = 0.0;
        if (row < D)
          for (int c = 0; c <= row; c++) s += L0[row * D + c] * Zs[c * 16 + j16];
        x[mt][r] = row < D ? m0[row] + s : 0.0;
      }
  }
  // A kept point leaves from Xs, where the wave's 16 states lie as [row][path]: element e = lane + 64 i of the 16 rows of `out` (path e / D,
  // component e % D), so that one store instruction writes runs of D consecutive doubles instead of 4 per path
  const uint32_t path0 = blockIdx.y * 64 + w * 16;
  const bool store = !segment && (!weighted || a.out != nullptr);
  double* o = store ? a.out + ((size_t)p * a.n_paths + path0) * (size_t)a.n_keep * D : nullptr;
  const size_t row_len = (size_t)a.n_keep * D;
  auto put = [&](double* dst, size_t len) {
#pragma unroll
    for (int i = 0; i < NT / 4; i++) {
      const int e = lane + 64 * i;
      if (e < 16 * D) {
        const int pl = e / D, cmp = e - pl * D;
        if (path0 + pl < (uint32_t)a.n_paths) dst[pl * len + cmp] = Xs[cmp * 16 + pl];
      }
    }
  };
  auto keep = [&]() {
    if (store) { put(o, row_len); o += D; }
  };
  // weighted: 1 / Sigma_ii of the lane's rows, the two sums, theta, the observation cursor
  double isg[sums ? MT : 1][4], pw = 0.0, ow = 0.0, th = 0.0;
  double sq[stats ? MT : 1][4], sg1[stats ? MT : 1][4];
  if constexpr (stats) {
    const double* row0 = &carried(a, (size_t)p * a.n_paths + path, D, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        const bool mine = path < (uint32_t)a.n_paths && row < D;
        sq[mt][r] = mine ? row0[row] : 0.0; sg1[mt][r] = mine ? row0[D + row] : 0.0;
      }
  }
  // SegmentEvents: the records of the lane's rows; the sides as a bit per row; the levels [NT] at the head of the Zs region, which a segment
  // does not use (written in front of the barrier below)
  double ex[events ? MT : 1][4];
  int et[events ? MT : 1][4], en[events ? MT : 1][4], eneg = 0;
  const double* evc = lds + NT * LDA + NT + 4 * NT * 16;
  if constexpr (events) {
    const double* row0 = a.pf_stats + ((size_t)p * a.n_paths + path) * 3 * D;      // (carried()'s row, written out: through it the four kernels move)
    if (tid < NT) lds[NT * LDA + NT + 4 * NT * 16 + tid] = tid < D ? a.ev_level[(size_t)p * D + tid] : 0.0;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        const bool mine = path < (uint32_t)a.n_paths && row < D;
        eneg |= row < D && a.ev_side[(size_t)p * D + row] < 0 ? 1 << (mt * 4 + r) : 0;
        ex[mt][r] = mine ? row0[row] : 0.0; et[mt][r] = mine ? (int)row0[D + row] : 0; en[mt][r] = mine ? (int)row0[2 * D + row] : 0;
      }
  }
  ObsCursor oc;
  if constexpr (weighted || table) oc = ObsCursor(a, p);
  if constexpr (segment) { if (!a.seg_first) oc.skip_through(a.k_begin); }
  auto observe = [&]() {      // x_k is in x and, whole, in the path's column of Xs
    const double* y = a.obs_y + (size_t)p * a.obs_y_stride + (size_t)oc.cur * D;
    const double* Qp = a.Q + (size_t)p * a.Q_stride;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        if (row < D) {
          const double ri = y[row] - x[mt][r];
          double qr = 0.0;
          if (a.Q_diag) qr = Qp[row * D + row] * ri;
          else
            for (int c = 0; c < D; c++) qr += Qp[row * D + c] * (y[c] - Xs[c * 16 + j16]);
          ow += ri * qr;
        }
      }
    oc.advance();
  };
  if constexpr (sums) {
    th = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta] : a.theta[0];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) isg[mt][r] = mt * 16 + q + 4 * r < D ? a.dt / (rd[mt][r] * rd[mt][r]) : 0.0;
  }
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int r = 0; r < 4; r++) Xs[(mt * 16 + q + 4 * r) * 16 + j16] = x[mt][r];
  __syncthreads();
  keep();
  if constexpr (sums) {
    if constexpr (!segment) put(a.start + ((size_t)p * a.n_paths + path0) * D, (size_t)D);
    if (oc.next == 0) observe();
  }
  // Backward: the particle slot `word` was copied from at the problem's observation j, to x and to the path's column of Xs (the points kept so
  // far have left Xs: the stores of `put` precede these writes in every lane of the wave that owns the region)
  auto reload = [&](int j) {
    const double* src = backward_source(a, p, j, word, D);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = mt * 16 + q + 4 * r;
        x[mt][r] = row < D ? src[row] : 0.0;
        Xs[row * 16 + j16] = x[mt][r];
      }
    __syncthreads();      // (uniform: the lanes of a workgroup belong to one problem)
  };
  if constexpr (table) {
    if (oc.next == 0) {
      oc.advance(); word = (uint32_t)lin[(size_t)oc.cur * a.n_paths];
      if constexpr (T.words == Words::TableReload) reload(oc.cur - 1);
    }
  }
  // the replay: the path's weight of the segment's stretch (Kept::Marginals: the integer one), the first kept index behind k_begin
  double wt = 0.0;
  double* red = lds + NT * LDA + NT + 4 * NT * 16;
  KeptCursor next_kept;
  long long pending = -1;
  unsigned long long qw = 0;
  if constexpr (replay) {
    if constexpr (kept == Kept::Marginals) qw = path < (uint32_t)a.n_paths ? stretch_weight(a, a.mg_qtab, p, oc.cur, path) : 0ull;
    else wt = path < (uint32_t)a.n_paths ? stretch_weight(a, a.pf_wtab, p, oc.cur, path) : 0.0;
    next_kept.first_behind(a.k_begin, a.stride);
  }
  // the action at a kept index, by the walk's `kept`
  auto at_kept = [&](long long slot) {
    if constexpr (kept == Kept::Marginals) {      // count, in reduce's place: the lane's own rows of its path, no cross-lane step
      if (qw != 0) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = mt * 16 + q + 4 * r;
            if (row < D) marginal_add(marginal_ladder(a, p, row, D), a.mg_L, mass_row(a, p, slot, row, D), x[mt][r], qw);
          }
      }
    } else if constexpr (kept == Kept::Covariance) {      // reduce_cov
      constexpr int T2 = MT * (MT + 1) / 2, ROUNDS = (T2 + MT - 1) / MT;
      double* zw = red + w * NT * 16;       // the wave's quarter of the Zs region: the rotated copy, then its MT tile slots
      double* mred = red + 4 * NT * 16;     // [4 waves][NT]
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = mt * 16 + q + 4 * r;
          double v1 = wt * x[mt][r];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) v1 += __shfl_xor(v1, o);
          if (j16 == 0) mred[w * NT + row] = v1;
          zw[row * 16 + ((j16 + 2 * (row >> 1)) & 15)] = x[mt][r];
        }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the copy is the wave's own: no barrier)
      __builtin_amdgcn_wave_barrier();
      double xa[MT][4], wq[4];
#pragma unroll
      for (int kk = 0; kk < 4; kk++) wq[kk] = __shfl(wt, kk * 4 + q);
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const int row = mt * 16 + j16;
          xa[mt][kk] = zw[row * 16 + ((kk * 4 + q + 2 * (row >> 1)) & 15)];
        }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the operands are read before the slots overwrite the copy)
      __builtin_amdgcn_wave_barrier();
      const size_t NVc = (size_t)D + (size_t)D * (D + 1) / 2;
      double* dst = a.pf_part + (((size_t)p * gridDim.y + blockIdx.y) * a.n_keep + (size_t)slot) * NVc;
#pragma unroll
      for (int rd = 0; rd < ROUNDS; rd++) {
        if (rd > 0) __syncthreads();      // (the slots of the round before have been read)
#pragma unroll
        for (int ti = 0; ti < MT; ti++)
#pragma unroll
          for (int tj = 0; tj <= ti; tj++) {
            const int t = ti * (ti + 1) / 2 + tj;
            if (t / MT == rd) {
              d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
              for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[ti][kk], wq[kk] * xa[tj][kk], acc, 0, 0, 0);
#pragma unroll
              for (int r = 0; r < 4; r++) zw[(t % MT) * 256 + r * 64 + lane] = acc[r];
            }
          }
        __syncthreads();
        if (rd == 0 && tid < D) dst[tid] = ((mred[tid] + mred[NT + tid]) + mred[2 * NT + tid]) + mred[3 * NT + tid];
#pragma unroll
        for (int ti = 0; ti < MT; ti++)
#pragma unroll
          for (int tj = 0; tj <= ti; tj++) {
            const int t = ti * (ti + 1) / 2 + tj;
            if (t / MT == rd) {
              const double* s0 = red + (t % MT) * 256 + tid;      // entry tid of the tile: row (lane >> 4) + 4 (tid >> 6), column lane & 15
              const double val = ((s0[0] + s0[NT * 16]) + s0[2 * NT * 16]) + s0[3 * NT * 16];
              const int ra = ti * 16 + q + 4 * w, cb = tj * 16 + j16;
              if (ra < D && cb <= ra) dst[D + (size_t)ra * (ra + 1) / 2 + cb] = val;
            }
          }
      }
    } else {      // reduce; flush() stores behind the next barrier
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double v1 = wt * x[mt][r], v2 = v1 * x[mt][r];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) { v1 += __shfl_xor(v1, o); v2 += __shfl_xor(v2, o); }
          if (j16 == 0) { red[(w * 2 + 0) * NT + mt * 16 + q + 4 * r] = v1; red[(w * 2 + 1) * NT + mt * 16 + q + 4 * r] = v2; }
        }
      pending = slot;
    }
  };
  auto flush = [&]() {      // (behind a barrier that follows reduce)
    if (pending >= 0) {
      if (tid < 2 * D) {
        const int m = tid >= D ? 1 : 0, row = tid - m * D;
        const double* r0 = red + m * NT + row;
        a.pf_part[(((size_t)p * gridDim.y + blockIdx.y) * a.n_keep + (size_t)pending) * 2 * D + tid] =
            ((r0[0] + r0[2 * NT]) + r0[4 * NT]) + r0[6 * NT];
      }
      pending = -1;
    }
  };
  if constexpr (replay) { if (a.seg_first) at_kept(0); }

  int until = a.stride;
  // pinned: the four lanes that hold the rows of slot 0 (workgroup (p, 0), wave 0, path column 0)
  bool pin = false;
  const double* ref = nullptr;
  if constexpr (pinned) { pin = path == 0; ref = a.pf_ref + (size_t)p * a.Np * D; }
  for (int k = k_first; k < k_stop; k++) {
    // A_k, b_k for the next step: requested now, written to LDS behind this step's products
    double pa[NPF], pb = 0.0;
    const bool more = k + 1 < k_stop;
    double xref[pinned ? MT : 1][4];      // pinned: the pinned lanes' rows of ref_k, requested now as well
    if constexpr (pinned) {
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = mt * 16 + q + 4 * r;
          xref[mt][r] = pin && row < D ? ref[(size_t)k * D + row] : 0.0;
        }
    }
    if (more) {
      const double* Ak = A + (size_t)k * DD;
#pragma unroll
      for (int n = 0; n < NPF; n++) { const int e = tid + 256 * n; pa[n] = e < DD ? Ak[e] : 0.0; }
      if (tid < D) pb = bv[(size_t)k * D + tid];
    }
    double xb[KT];
#pragma unroll
    for (int kk = 0; kk < KT; kk++) xb[kk] = Xs[(kk * 4 + q) * 16 + j16];
    normals_c<NT>(k0, k1, (uint32_t)k, word, p, D, q, z);
    if (dense) {
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) Zs[(mt * 16 + q + 4 * r) * 16 + j16] = z[mt][r];
      __syncthreads();
    }
    // weighted: the rows of x_{k-1} that the circular drift reaches by wrapping around -- 0, D - 1, D - 2 -- once per step
    const double* xq = Xs + q * 16 + j16;
    double w0 = 0.0, wl1 = 0.0, wl2 = 0.0;
    if constexpr (sums) { w0 = Xs[j16]; wl1 = Xs[(D - 1) * 16 + j16]; wl2 = Xs[(D - 2) * 16 + j16]; }
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* ar = As + (mt * 16 + j16) * LDA + q;
#pragma unroll
      for (int kk = 0; kk < KT; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[kk * 4], xb[kk], acc, 0, 0, 0);
      d4 nz = {rd[mt][0] * z[mt][0], rd[mt][1] * z[mt][1], rd[mt][2] * z[mt][2], rd[mt][3] * z[mt][3]};
      if (dense) {
        nz = d4{0.0, 0.0, 0.0, 0.0};
        const double* rr = Rs + (mt * 16 + j16) * LDA + q;
#pragma unroll
        for (int kk = 0; kk < KT; kk++) nz = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[kk * 4], Zs[(kk * 4 + q) * 16 + j16], nz, 0, 0, 0);
      }
      if constexpr (pinned) {      // the increment the reference implies, in R xi's place (rows beyond D: 0 - 0)
        if (pin) {
#pragma unroll
          for (int r = 0; r < 4; r++) nz[r] = (xref[mt][r] - x[mt][r]) - a.dt * (bs[mt * 16 + q + 4 * r] - acc[r]);
        }
      }
      if constexpr (sums) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = mt * 16 + q + 4 * r;
          if (row < D) {
            // the neighbours at fixed offsets from the lane's own row (one address register); only rows 0, 1 and D - 1 wrap
            const double* xr = xq + (mt * 16 + 4 * r) * 16;
            const double xu = row + 1 < D ? xr[16] : w0;
            double xd1 = wl1, xd2 = wl2;
            if (mt > 0 || r > 0) { xd1 = xr[-16]; xd2 = xr[-32]; }
            else {
              if (q >= 1) xd1 = xr[-16];
              if (q >= 2) xd2 = xr[-32]; else if (q == 1) xd2 = wl1;
            }
            const double f = (xu - xd2) * xd1 - x[mt][r] + th;
            const double d = (bs[row] - acc[r]) - f;
            pw -= isg[mt][r] * d * (nz[r] + 0.5 * a.dt * d);
            if constexpr (stats) stats_step(a.dt, d, nz[r], 1.0, sq[mt][r], sg1[mt][r]);      // (phi = 1: Lorenz-96)
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) x[mt][r] = (x[mt][r] + a.dt * (bs[mt * 16 + q + 4 * r] - acc[r])) + nz[r];
      if constexpr (pinned) {      // (ref_k as loaded, not as recomputed; it goes to Xs with every lane's rows below)
        if (pin) {
#pragma unroll
          for (int r = 0; r < 4; r++) x[mt][r] = xref[mt][r];
        }
      }
      if constexpr (events) {
#pragma unroll
        for (int r = 0; r < 4; r++) event_step(x[mt][r], evc[mt * 16 + q + 4 * r], (eneg >> (mt * 4 + r)) & 1, k, ex[mt][r], et[mt][r], en[mt][r]);
      }
    }
    __syncthreads();
    if constexpr (kept == Kept::Moments) flush();
    if (more) {
#pragma unroll
      for (int n = 0; n < NPF; n++) { const int e = tid + 256 * n; if (e < DD) As[(e / D) * LDA + e % D] = pa[n]; }
      if (tid < D) bs[tid] = pb;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int r = 0; r < 4; r++) Xs[(mt * 16 + q + 4 * r) * 16 + j16] = x[mt][r];
    __syncthreads();
    if (--until == 0) { until = a.stride; keep(); }
    if constexpr (sums) {
      if (k == oc.next) observe();
    }
    if constexpr (replay) { if (k == next_kept.k) { at_kept(next_kept.slot++); next_kept.k += a.stride; } }
    if constexpr (table) {
      if (k == oc.next) {
        oc.advance(); word = (uint32_t)lin[(size_t)oc.cur * a.n_paths];
        if constexpr (T.words == Words::TableReload) reload(oc.cur - 1);
      }
    }
  }
  if constexpr (replay) {
    __syncthreads();
    if constexpr (kept == Kept::Moments) flush();
    put(a.pf_x + ((size_t)p * a.n_paths + path0) * D, (size_t)D);      // (Xs holds x_{k_end} behind the loop's last barrier)
  } else if constexpr (weighted) {
    pw += __shfl_xor(pw, 16); pw += __shfl_xor(pw, 32);
    ow += __shfl_xor(ow, 16); ow += __shfl_xor(ow, 32);
    if constexpr (segment) {
      if (q == 0 && path < (uint32_t)a.n_paths) a.pf_lw[(size_t)p * a.n_paths + path] += pw - 0.5 * ow;
      put(a.pf_x + ((size_t)p * a.n_paths + path0) * D, (size_t)D);      // (Xs holds x_{k_end} behind the loop's last barrier)
      if constexpr (stats) {
        if (path < (uint32_t)a.n_paths) {
          double* row0 = &carried(a, (size_t)p * a.n_paths + path, D, 0, 0);
          const double h = a.dt * (double)a.k_end;
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const int row = mt * 16 + q + 4 * r;
              if (row < D) { row0[row] = sq[mt][r]; row0[D + row] = sg1[mt][r]; row0[2 * D + row] = h; }
            }
        }
      }
      if constexpr (events) {
        if (path < (uint32_t)a.n_paths) {
          double* row0 = a.pf_stats + ((size_t)p * a.n_paths + path) * 3 * D;      // (written out, as at the entry)
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const int row = mt * 16 + q + 4 * r;
              if (row < D) { row0[row] = ex[mt][r]; row0[D + row] = (double)et[mt][r]; row0[2 * D + row] = (double)en[mt][r]; }
            }
        }
      }
    } else if (q == 0 && path < (uint32_t)a.n_paths) {
      double* lw = a.logw + 2 * ((size_t)p * a.n_paths + path);
      lw[0] = pw; lw[1] = -0.5 * ow - obs_constant(a, p);
    }
  }
}

// ---- 5 <= D <= 64, model kind: Lorenz-96 ------------------------------------------------------------------------------------------
// One lane per (problem, path); xs [D][64] in LDS, component-major so that a wave's 64 lanes touch 64 consecutive doubles.  The drift is
// evaluated in place behind three rolling registers of old values.  zs [D][64]: the normals, when a dense factor needs all of them at once.
// x_0 = m0 + L0 xi_0 of path `path` of problem p: the normals of grid index 0 to z, then the rows of L0 in order; S doubles between two
// components of z and of x
template <int S>
__device__ __forceinline__ void start_draw(uint32_t k0, uint32_t k1, uint32_t path, uint32_t p, int D, const double* m0, const double* L0,
                                           double* z, double* x) {
  for (int j = 0; 2 * j < D; j++) {
    double c, s;
    normal_pair(k0, k1, 0u, path, p, (uint32_t)j, &c, &s);
    z[2 * j * S] = c;
    if (2 * j + 1 < D) z[(2 * j + 1) * S] = s;
  }
  for (int i = 0; i < D; i++) {
    double s = 0.0;
    for (int j = 0; j <= i; j++) s += L0[i * D + j] * z[j * S];
    x[i * S] = m0[i] + s;
  }
}

// One Lorenz-96 step of the lane's column xs at grid index k with counter word `word`: a diagonal factor draws each pair of normals where it
// is used, a dense one (dense) finds all of them in the lane's column zs, drawn by the caller (drawn in here, k_sample_l96 takes 98 VGPRs
// for 96 and 4 waves per SIMD for 5)
__device__ __forceinline__ void l96_step(uint32_t k0, uint32_t k1, uint32_t k, uint32_t word, uint32_t p, int D, double th, double dt,
                                         const double* Rp, bool dense, double* xs, const double* zs) {
  const double x_first = xs[0];
  double om2 = xs[(D - 2) * 64], om1 = xs[(D - 1) * 64], cur = x_first, zc = 0.0, zn = 0.0;
  for (int i = 0; i < D; i++) {
    const double nxt = i + 1 < D ? xs[(i + 1) * 64] : x_first;
    const double f = (nxt - om2) * om1 - cur + th;
    double nz;
    if (dense) {
      nz = 0.0;
      for (int j = 0; j <= i; j++) nz += Rp[i * D + j] * zs[j * 64];
    } else {
      if (!(i & 1)) normal_pair(k0, k1, k, word, p, (uint32_t)(i >> 1), &zc, &zn);
      nz = Rp[i * D + i] * ((i & 1) ? zn : zc);
    }
    xs[i * 64] = (cur + dt * f) + nz;
    om2 = om1; om1 = cur; cur = nxt;
  }
}

__global__ __launch_bounds__(64) void k_sample_l96(SampleArgs a) {
  extern __shared__ double lds[];
  const int D = a.D, lane = threadIdx.x;
  double* xs = lds + lane;
  double* zs = lds + (size_t)D * 64 + lane;
  const size_t gid = (size_t)blockIdx.x * 64 + lane;
  if (gid >= (size_t)a.batch * a.n_paths) return;      // (no barrier below: a lane reads and writes its own column only)
  const uint32_t p = (uint32_t)(gid / a.n_paths), path = (uint32_t)(gid % a.n_paths);
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const double th = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta] : a.theta[0];
  const bool dense = !a.R_diag;
  if (a.x0) {
    for (int i = 0; i < D; i++) xs[i * 64] = a.x0[(size_t)p * D + i];
  } else {
    const double* m0 = a.m0 + (size_t)p * a.m0_stride;
    const double* L0 = a.L0 + (size_t)p * a.L0_stride;
    start_draw<64>(k0, k1, path, p, D, m0, L0, zs, xs);
  }
  double* o = a.out + gid * (size_t)a.n_keep * D;
  for (int i = 0; i < D; i++) o[i] = xs[i * 64];
  o += D;
  int until = a.stride;
  for (int k = 1; k < a.Np; k++) {
    if (dense)
      for (int j = 0; 2 * j < D; j++) {
        double c, s;
        normal_pair(k0, k1, (uint32_t)k, path, p, (uint32_t)j, &c, &s);
        zs[2 * j * 64] = c;
        if (2 * j + 1 < D) zs[(2 * j + 1) * 64] = s;
      }
    l96_step(k0, k1, (uint32_t)k, path, p, D, th, a.dt, Rp, dense, xs, zs);
    if (--until == 0) {
      until = a.stride;
      for (int i = 0; i < D; i++) o[i] = xs[i * 64];
      o += D;
    }
  }
}

// ---- 5 <= D <= 64, the forecast: Lorenz-96 from a cloud ---------------------------------------------------------------------------------
// Walk::Forecast above D = 4: workgroup (p, blk) is one wave, lane = slot blk * 64 + lane of problem p (the member launch:
// lane m, which starts from slot pf_slots[p][m] and draws with that slot's word), the state in LDS as in k_sample_l96, whose diagonal step
// this is, drawn at the absolute grid index k_begin + h.  At a kept h of the cloud launch the wave owns the D x 64 tile xs and the 64 weights
// ws: lane l < D adds row l of W x and (W x) x over the 64 columns in the order l, l + 1, ..., 63, 0, ..., l - 1.  (A wave's 64-bit LDS read is
// served in two groups of 32 lanes; with a row stride of 64 doubles every lane of an unskewed read would sit on one bank pair, the skew puts
// the 32 lanes of a group on 32 different pairs.)  One order, whatever the launch: the sums are reproducible.  A lane behind the last one
// walks the last one again with weight 0 and stores nothing.
__global__ __launch_bounds__(64) void k_forecast_l96(SampleArgs a) {
  extern __shared__ double lds[];
  const int D = a.D, lane = threadIdx.x;
  double* xs = lds + lane;
  double* ws = lds + (size_t)D * 64;
  const uint32_t p = blockIdx.x, slot = blockIdx.y * 64 + lane;
  const bool live = slot < (uint32_t)a.n_paths;
  const size_t gid = (size_t)p * a.n_paths + (live ? slot : (uint32_t)a.n_paths - 1);
  const uint32_t word = a.pf_slots ? (uint32_t)a.pf_slots[gid] : (uint32_t)(gid - (size_t)p * a.n_paths);
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  const double* Rp = a.R + (size_t)p * a.R_stride;
  const double th = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta] : a.theta[0];
  {
    const double* x0 = a.pf_x + ((size_t)p * a.pf_n + word) * D;
    for (int i = 0; i < D; i++) xs[i * 64] = x0[i];
  }
  const bool sums = a.pf_part != nullptr, store = live && a.out != nullptr;
  ws[lane] = live && sums ? a.pf_wtab[gid] : 0.0;
  double* part = sums ? a.pf_part + ((size_t)p * gridDim.y + blockIdx.y) * a.n_keep * 2 * D : nullptr;
  auto reduce = [&]() {
    __syncthreads();      // (the tile and the weights are written)
    if (lane < D) {
      const double* row = lds + (size_t)lane * 64;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
      for (int c = 0; c < 64; c++) {
        const int col = (lane + c) & 63;
        const double v = ws[col] * row[col];
        s1 += v; s2 += v * row[col];
      }
      part[lane] = s1; part[D + lane] = s2;
    }
    part += 2 * D;
    __syncthreads();      // (the tile has been read)
  };
  double* o = store ? a.out + gid * (size_t)a.n_keep * D : nullptr;
  if (store) {
    for (int i = 0; i < D; i++) o[i] = xs[i * 64];
    o += D;
  }
  if (sums) reduce();
  int until = a.stride;
  const int H = a.k_end - a.k_begin;
  for (int h = 0; h < H; h++) {      // (step h + 1; k_begin + h + 1 may be the last index an int holds)
    const uint32_t k = (uint32_t)a.k_begin + (uint32_t)h + 1u;
    l96_step(k0, k1, k, word, p, D, th, a.dt, Rp, false, xs, nullptr);
    if (--until == 0) {
      until = a.stride;
      if (sums) reduce();
      if (store) {
        for (int i = 0; i < D; i++) o[i] = xs[i * 64];
        o += D;
      }
    }
  }
  if (live && sums) {
    double* xe = a.pf_x + gid * D;
    for (int i = 0; i < D; i++) xe[i] = xs[i * 64];
  }
}

// ---- the particle filter: the start, the segments, the resampling step between them ------------------------------------------------
// One lane per particle: x_0 (given, or m0 + L0 xi_0 summed as the samplers sum it) to a.x, and lw = init - c_p with
// init = log N(x_0; mu0, tau0) - log N(x_0; m0, S0) for a drawn start under a prior (the two triangular solves against the factors in global
// memory; a.ws [B][n][D] holds the lane's normals, then its solutions), else 0.  Runs once per call.
__global__ __launch_bounds__(256) void k_pf_start(PfArgs a) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.batch * a.n_paths) return;
  const int D = a.D;
  const uint32_t p = (uint32_t)(gid / a.n_paths), path = (uint32_t)(gid % a.n_paths);
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  double* x = a.x + gid * D;
  double* u = a.ws + gid * D;
  double init = 0.0;
  if (a.x0) {
    for (int i = 0; i < D; i++) x[i] = a.x0[(size_t)p * D + i];
  } else {
    const double* m0 = a.m0 + (size_t)p * a.m0_stride;
    const double* L0 = a.L0 + (size_t)p * a.L0_stride;
    start_draw<1>(k0, k1, path, p, D, m0, L0, u, x);
    if (a.mu0) {
      const double* mu = a.mu0 + (size_t)p * D;
      const double* Lt = a.Lt + (size_t)p * D * D;
      double q0 = 0.0, ld0 = 0.0, q1 = 0.0, ld1 = 0.0;
      for (int i = 0; i < D; i++) {      // L0 v = x_0 - m0 (v overwrites the normals it is, up to rounding)
        double s = x[i] - m0[i];
        for (int j = 0; j < i; j++) s -= L0[i * D + j] * u[j];
        u[i] = s / L0[i * D + i];
        q0 += u[i] * u[i]; ld0 += log(L0[i * D + i]);
      }
      for (int i = 0; i < D; i++) {      // Lt v = x_0 - mu0
        double s = x[i] - mu[i];
        for (int j = 0; j < i; j++) s -= Lt[i * D + j] * u[j];
        u[i] = s / Lt[i * D + i];
        q1 += u[i] * u[i]; ld1 += log(Lt[i * D + i]);
      }
      init = (-0.5 * q1 - ld1) - (-0.5 * q0 - ld0);
    }
  }
  a.lw[gid] = init - a.obs_const_scale * (a.obs_const_v ? a.obs_const_v[p] : a.obs_const);
}

// vgpa_particle_conditional, behind k_pf_start: one thread per problem pins slot 0 to ref[p][0] and gives it k_pf_start's own log-weight
// at that state -- the same two triangular solves, x_0 - m0 in place of the drawn normals.
__global__ __launch_bounds__(256) void k_pf_pin(PfArgs a) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= (uint32_t)a.batch) return;
  const int D = a.D;
  const size_t gid = (size_t)p * a.n_paths;
  const double* xr = a.ref + (size_t)p * a.Np * D;
  double* x = a.x + gid * D;
  double* u = a.ws + gid * D;
  for (int i = 0; i < D; i++) x[i] = xr[i];
  double init = 0.0;
  if (!a.x0 && a.mu0) {
    const double* m0 = a.m0 + (size_t)p * a.m0_stride;
    const double* L0 = a.L0 + (size_t)p * a.L0_stride;
    const double* mu = a.mu0 + (size_t)p * D;
    const double* Lt = a.Lt + (size_t)p * D * D;
    double q0 = 0.0, ld0 = 0.0, q1 = 0.0, ld1 = 0.0;
    for (int i = 0; i < D; i++) {
      double s = x[i] - m0[i];
      for (int j = 0; j < i; j++) s -= L0[i * D + j] * u[j];
      u[i] = s / L0[i * D + i];
      q0 += u[i] * u[i]; ld0 += log(L0[i * D + i]);
    }
    for (int i = 0; i < D; i++) {
      double s = x[i] - mu[i];
      for (int j = 0; j < i; j++) s -= Lt[i * D + j] * u[j];
      u[i] = s / Lt[i * D + i];
      q1 += u[i] * u[i]; ld1 += log(Lt[i * D + i]);
    }
    init = (-0.5 * q1 - ld1) - (-0.5 * q0 - ld0);
  }
  a.lw[gid] = init - a.obs_const_scale * (a.obs_const_v ? a.obs_const_v[p] : a.obs_const);
}

// What k_pf_resample, k_pf_pick and k_pf_descend share, a workgroup of 256 threads on the n log-weights of one problem.
// pf_max: max lw (red: 4 doubles of LDS).
// pf_prefix_sums: cum_i = the inclusive prefix sums of w_i = exp(lw_i - mx) in slot order, 256 slots per pass: a shuffle scan per wave, the
// waves' totals and the carry through LDS (tot: 4 doubles); returns the thread's share of sum w^2.  No barrier behind the last store of cum.
// pf_bisect: min(#{m: cum_m <= u}, n - 1), the slot a threshold u falls into.  pf_obs_at: the problem's observation at grid index a.k, or -1.
__device__ __forceinline__ double pf_max(const double* lw, int n, double* red) {
  double mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) mx = fmax(mx, lw[i]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
__device__ __forceinline__ int pf_bisect(const double* cum, int n, double u) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo < n - 1 ? lo : n - 1;
}
__device__ __forceinline__ double pf_prefix_sums(const double* lw, int n, double mx, double* cum, double* tot) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double carry = 0.0, s2 = 0.0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const double wi = i < n ? exp(lw[i] - mx) : 0.0;
    s2 += wi * wi;
    double sc = wi;      // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(sc, o); if (lane >= o) sc += up; }
    __syncthreads();      // (tot of the pass before has been read)
    if (lane == 63) tot[w] = sc;
    __syncthreads();
    double before = carry;
    for (int v = 0; v < w; v++) before += tot[v];
    if (i < n) cum[i] = before + sc;
    carry = (((carry + tot[0]) + tot[1]) + tot[2]) + tot[3];      // (the association of the last slot's own sum)
  }
  return s2;
}

// The step between two segments, one workgroup per problem, at grid index a.k.  A problem without an observation at a.k
// copies its particles through.  Otherwise: w_i = exp(lw_i - max lw), S = sum w, ESS = S^2 / sum w^2, cum = the inclusive prefix sums of w in
// slot order (256 slots per pass: a shuffle scan per wave, the waves' totals and the carry through LDS); resampled iff ESS < ess_fraction n and
// a.k is not the last grid index: anc_i = min(#{m: cum_m <= (U + i) / n S}, n - 1) by bisection, U from Philox counter (k, 0, p, 0xffffffff),
// x_out_i = x_in_{anc_i}, lw_i = max lw + log S - log n; else anc_i = i and lw stays.  The histories of observation j (t_j = a.k) are
// written where asked for; the cloud is x_in, and h_lw gets the log-weights a resampling replaces (no other row of it is written or read).
// ST: the [3][D] rows of path statistics go from st_in to st_out by the same ancestors (two buffers, as for x: no slot is read after it is
// written).
template <bool ST>
__global__ __launch_bounds__(256) void k_pf_resample(PfArgs a) {
  __shared__ double tot[4], red[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n_paths, D = a.D;
  const int j = pf_obs_at(a, p);
  const size_t nD = (size_t)n * D;
  const double* xin = a.x_in + (size_t)p * nD;
  double* xout = a.x_out + (size_t)p * nD;
  if (j < 0) {      // (uniform over the workgroup)
    for (size_t e = tid; e < nD; e += 256) xout[e] = xin[e];
    if constexpr (ST)
      for (size_t e = tid; e < 3 * nD; e += 256) a.st_out[(size_t)p * 3 * nD + e] = a.st_in[(size_t)p * 3 * nD + e];
    return;
  }
  double* lw = a.lw + (size_t)p * n;
  double* cum = a.cum + (size_t)p * n;
  int32_t* anc = a.anc + (size_t)p * n;
  const double mx = pf_max(lw, n, red);
  double s2 = pf_prefix_sums(lw, n, mx, cum, tot);
  // S is what the last slot's prefix sum is, to the last bit: every threshold lies below cum_{n-1} as the exact ones do
  __syncthreads();      // (cum is written; red has been read)
  const double S = cum[n - 1];
  s2 = wave_sum(s2);
  if (lane == 0) red[w] = s2;
  __syncthreads();
  s2 = (red[0] + red[1]) + (red[2] + red[3]);
  const double ess = S * S / s2;
  const bool go = ess < a.ess_fraction * (double)n && !a.last;
  const size_t hj = (size_t)p * a.M + j;
  if (tid == 0) { a.h_ess[hj] = ess; a.h_flag[hj] = go ? 1 : 0; }
  if (a.h_clouds)
    for (size_t e = tid; e < nD; e += 256) a.h_clouds[hj * nD + e] = xin[e];
  double U = 0.0;
  if (go) {
    uint32_t r[4];
    philox4x32_10((uint32_t)a.k, 0u, (uint32_t)p, 0xffffffffu, (uint32_t)(a.seed & 0xffffffffu), (uint32_t)(a.seed >> 32), r);
    U = unit_open(r[0], r[1]);
  }
  const double lw_new = mx + log(S) - log((double)n);
  for (int i = tid; i < n; i += 256) {
    int from = i;
    if (go) {
      const double ui = (U + (double)i) / (double)n * S;
      from = pf_bisect(cum, n, ui);
      if (a.h_lw) a.h_lw[hj * n + i] = lw[i];
      lw[i] = lw_new;
    }
    anc[i] = from;
    if (a.h_anc) a.h_anc[hj * n + i] = from;
  }
  __syncthreads();
  for (size_t e = tid; e < nD; e += 256) {
    const size_t i = e / D;
    xout[e] = xin[(size_t)anc[i] * D + (e - i * D)];
  }
  if constexpr (ST) {
    const size_t D3 = 3 * (size_t)D;
    for (size_t e = tid; e < 3 * nD; e += 256) {
      const size_t i = e / D3;
      a.st_out[(size_t)p * 3 * nD + e] = a.st_in[(size_t)p * 3 * nD + (size_t)anc[i] * D3 + (e - i * D3)];
    }
  }
}

// The self-normalised weighted mean of the rows of path statistics: workgroup (p, s) sums statistic s of problem p over the slots,
// mean[p][s][j] = sum_i w_i stats[p][i][s][j] / sum_i w_i with w_i = exp(lw_i - max lw).  Thread t takes component t mod D of the slots
// t / D, t / D + G, ... (G = 256 / D slots at a time), the G partial sums of a component are added in order through LDS.
__global__ __launch_bounds__(256) void k_pf_stats_mean(int D, int n, const double* lw_all, const double* stats, double* mean) {
  __shared__ double part[256], wpart[256], red[4];
  const int p = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const double* lw = lw_all + (size_t)p * n;
  const double* rows = stats + (size_t)p * n * 3 * D + (size_t)s * D;
  double mx = -INFINITY;      // (pf_max, written out: the call changes this kernel's schedule)
  for (int i = tid; i < n; i += 256) mx = fmax(mx, lw[i]);
  mx = wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const int G = 256 / D, g = tid / D, j = tid - g * D;
  double acc = 0.0, sw = 0.0;
  if (g < G)
    for (int i = g; i < n; i += G) {
      const double wi = exp(lw[i] - mx);
      acc += wi * rows[(size_t)i * 3 * D + j];
      sw += wi;
    }
  part[tid] = acc; wpart[tid] = sw;
  __syncthreads();
  if (tid < D) {
    double num = 0.0, den = 0.0;
    for (int v = 0; v < G; v++) { num += part[v * D + tid]; den += wpart[v * D + tid]; }
    mean[((size_t)p * 3 + s) * D + tid] = num / den;
  }
}

// ---- the smoothing moments: the descendant weights, the gather of the replay, the sum of the workgroups' partial sums -----------------
// v summed over the workgroup in a fixed order: the butterfly of each wave, then the four waves through `red`
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();      // (red of the sum before has been read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The descendant weights, one workgroup per problem with c observations of its own: row c of wtab [rows][n] is
// W_i = w_i / sum w, w_i = exp(lw_i - max lw); for j = c-1 .. 0 row j is row j+1 where the cloud was carried on at observation j, else
// W^j_a = the sum of W^{j+1}_i over the slots i with anc_i = a.  Systematic resampling makes anc non-decreasing, so these slots are the run
// [first i with anc_i >= a, first i with anc_i >= a + 1), found by two bisections and added in increasing i by slot a's own thread: no
// atomics, and no order that depends on the launch.  less[j] = 1 / sum_i (W^j_i)^2.
__global__ __launch_bounds__(256) void k_pf_descend(PfArgs a, int rows, double* wtab_all, double* less_all) {
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x, n = a.n_paths;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  const double* lw = a.lw + (size_t)p * n;
  double* wtab = wtab_all + (size_t)p * rows * n;
  double* less = less_all + (size_t)p * rows;
  const double mx = pf_max(lw, n, red);
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += exp(lw[i] - mx);
  s = block_sum(s, red);
  double* row = wtab + (size_t)cnt * n;
  double s2 = 0.0;
  for (int i = tid; i < n; i += 256) { const double wi = exp(lw[i] - mx) / s; row[i] = wi; s2 += wi * wi; }
  s2 = block_sum(s2, red);      // (its barriers also order the row's stores before the reads below)
  if (tid == 0) less[cnt] = 1.0 / s2;
  for (int j = cnt - 1; j >= 0; j--) {
    const double* next = row;
    row = wtab + (size_t)j * n;
    const size_t hj = (size_t)p * a.M + j;
    const int32_t* anc = a.h_anc + hj * n;
    const bool gathered = a.h_flag[hj] != 0;      // (uniform over the workgroup)
    s2 = 0.0;
    for (int i = tid; i < n; i += 256) {
      double wi = next[i];
      if (gathered) {
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (anc[mid] < i) lo = mid + 1; else hi = mid; }
        int end = lo;
        hi = n;
        while (end < hi) { const int mid = (end + hi) >> 1; if (anc[mid] <= i) end = mid + 1; else hi = mid; }
        wi = 0.0;
        int m = lo;
        for (; m + 8 <= end; m += 8) {      // (eight loads in flight, the additions in slot order)
          double t8[8];
#pragma unroll
          for (int u = 0; u < 8; u++) t8[u] = next[m + u];
#pragma unroll
          for (int u = 0; u < 8; u++) wi += t8[u];
        }
        for (; m < end; m++) wi += next[m];
      }
      row[i] = wi;
      s2 += wi * wi;
    }
    s2 = block_sum(s2, red);
    if (tid == 0) less[j] = 1.0 / s2;
  }
}

// ---- the smoothing marginals: the descendant weights as integers ------------------------------------------------------
// Behind k_pf_descend, one thread per (problem, slot): row c of qtab [rows][n] = (uint64) trunc(W 2^62) of row c of wtab, c the problem's own
// observation count, and the same value to qfinal [B][n], the dense array that leaves in one copy.  W <= 1 and the product by a power of two
// is exact: the conversion alone rounds, towards zero.
__global__ __launch_bounds__(256) void k_pf_quantise(PfArgs a, int rows, const double* wtab, uint64_t* qtab, uint64_t* qfinal) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)a.batch * a.n_paths) return;
  const size_t p = g / a.n_paths, i = g - p * a.n_paths;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  const size_t e = (p * rows + cnt) * a.n_paths + i;
  const double v = wtab[e] * 0x1.0p62;
  const uint64_t qv = v >= 1.0 ? (uint64_t)v : 0ull;      // (a NaN or a negative weight: 0)
  qtab[e] = qv; qfinal[g] = qv;
}

// k_pf_descend's recursion on the integers, one workgroup per problem: for j = c-1 .. 0 row j of qtab is row j+1 where the cloud was carried
// on at observation j, else Q^j_a = the sum of Q^{j+1}_i over the run [first i with anc_i >= a, first i with anc_i >= a + 1) of the
// non-decreasing ancestors, found by the same two bisections and added by slot a's own thread in 64-bit integer arithmetic.
__global__ __launch_bounds__(256) void k_pf_descend_q(PfArgs a, int rows, uint64_t* qtab_all) {
  const int p = blockIdx.x, tid = threadIdx.x, n = a.n_paths;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  uint64_t* qtab = qtab_all + (size_t)p * rows * n;
  uint64_t* row = qtab + (size_t)cnt * n;
  for (int j = cnt - 1; j >= 0; j--) {
    const uint64_t* next = row;
    row = qtab + (size_t)j * n;
    const size_t hj = (size_t)p * a.M + j;
    const int32_t* anc = a.h_anc + hj * n;
    const bool gathered = a.h_flag[hj] != 0;      // (uniform over the workgroup)
    for (int i = tid; i < n; i += 256) {
      uint64_t qi = next[i];
      if (gathered) {
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (anc[mid] < i) lo = mid + 1; else hi = mid; }
        int end = lo;
        hi = n;
        while (end < hi) { const int mid = (end + hi) >> 1; if (anc[mid] <= i) end = mid + 1; else hi = mid; }
        qi = 0;
        int m = lo;
        for (; m + 8 <= end; m += 8) {      // (eight loads in flight, as in k_pf_descend)
          uint64_t t8[8];
#pragma unroll
          for (int u = 0; u < 8; u++) t8[u] = next[m + u];
#pragma unroll
          for (int u = 0; u < 8; u++) qi += t8[u];
        }
        for (; m < end; m++) qi += next[m];
      }
      row[i] = qi;
    }
    __syncthreads();      // (the row is written before the next one reads it)
  }
}

// The forecast's weights, one workgroup per problem: W_i = w_i / sum w with w_i = exp(lw_i - max lw), the sum in the fixed order of block_sum.
__global__ __launch_bounds__(256) void k_pf_normalise(int n, const double* lw_all, double* w_all) {
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* lw = lw_all + (size_t)p * n;
  double* w = w_all + (size_t)p * n;
  const double mx = pf_max(lw, n, red);
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += exp(lw[i] - mx);
  s = block_sum(s, red);
  for (int i = tid; i < n; i += 256) w[i] = exp(lw[i] - mx) / s;
}

// ---- path events: the rows of grid index 0, the first-passage distribution ---------------------------------------------
// Behind k_pf_start, one thread per (problem, particle, component): the record of grid index 0 from the particle's state, in front of the
// first segment and of a resampling decision at grid index 0.  Np is the sentinel "never so far".
__global__ __launch_bounds__(256) void k_pf_events_start(int D, int n, int Np, size_t total, const double* x, const double* level, const int32_t* side,
                                                         double* rows) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const size_t slot = g / D, j = g - slot * D, p = slot / n;
  const double d = x[g] - level[p * D + j], ev = side[p * D + j] < 0 ? -d : d;
  double* row = rows + slot * 3 * D + j;
  row[0] = ev; row[D] = ev > 0.0 ? 0.0 : (double)Np; row[2 * (size_t)D] = ev > 0.0 ? 1.0 : 0.0;
}

// The first-passage distribution on the kept grid, workgroup (p, j) for component j of problem p: cdf[p][k'][j] = sum_i W_i 1[T_ij <= k' stride],
// W_i = w_i / S, w_i = exp(lw_i - max lw).  The bin of T is ceil(T / stride), no bin beyond the last kept index (the sentinel Np always is).
// S is block_sum's fixed order.  The kept indices go in tiles of kCdfTile bins of LDS; per tile the particles' (bin, w) stream through LDS 256
// at a time in increasing i, and thread t, which owns the kCdfTile / 256 consecutive bins from t kCdfTile / 256 on, adds to its own bins the
// w_i that fall into them, in increasing i.  Then the inclusive prefix sums in increasing bin order -- each thread over its own bins, the
// threads' totals in thread order by one thread, the tiles behind one another through `carry` -- and the division by S: every value is the
// value before it plus a sum of weights >= 0, so the row is non-decreasing to the bit, and no addition depends on the launch or the batch.
constexpr int kCdfTile = 2048;
__global__ __launch_bounds__(256) void k_pf_events_cdf(int D, int n, int Np, int stride, const double* lw_all, const double* rows_all, double* cdf_all) {
  constexpr int PER = kCdfTile / 256;
  __shared__ double bins[kCdfTile], ws[256], base[257], red[4];
  __shared__ int bs[256];
  const int p = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const int n_keep = (Np - 1) / stride + 1;
  const double* lw = lw_all + (size_t)p * n;
  const double* tcol = rows_all + (size_t)p * n * 3 * D + D + j;      // T_ij at tcol[i 3 D]
  double* cdf = cdf_all + (size_t)p * n_keep * D + j;                 // cdf[k'] at cdf[k' D]
  const double mx = pf_max(lw, n, red);
  double S = 0.0;
  for (int i = tid; i < n; i += 256) S += exp(lw[i] - mx);
  S = block_sum(S, red);
  double carry = 0.0;
  for (int tile = 0; tile < n_keep; tile += kCdfTile) {
#pragma unroll
    for (int e = 0; e < PER; e++) bins[tid * PER + e] = 0.0;
    for (int i0 = 0; i0 < n; i0 += 256) {
      __syncthreads();      // (the particles before have been read; the first pass: `base` of the tile before)
      const int i = i0 + tid;
      int b = -1;
      double wi = 0.0;
      if (i < n) {
        const long long bin = ((long long)tcol[(size_t)i * 3 * D] + stride - 1) / stride - tile;
        if (bin >= 0 && bin < kCdfTile && bin + tile < n_keep) b = (int)bin;
        wi = exp(lw[i] - mx);
      }
      bs[tid] = b; ws[tid] = wi;
      __syncthreads();
      const int cnt = n - i0 < 256 ? n - i0 : 256;
      for (int m = 0; m < cnt; m++) {
        const int bm = bs[m];
        if (bm >= 0 && bm / PER == tid) bins[bm] += ws[m];
      }
    }
    double run = 0.0;      // the thread's own bins: their inclusive prefix sums in place, their total
#pragma unroll
    for (int e = 0; e < PER; e++) { run += bins[tid * PER + e]; bins[tid * PER + e] = run; }
    base[tid + 1] = run;
    __syncthreads();
    if (tid == 0) {
      base[0] = carry;
      for (int t = 0; t < 256; t++) base[t + 1] = base[t] + base[t + 1];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PER; e++) {
      const int kp = tile + tid * PER + e;
      if (kp < n_keep) cdf[(size_t)kp * D] = (base[tid] + bins[tid * PER + e]) / S;
    }
    carry = base[256];
  }
}

// The step between two segments of the replay at grid index a.k: workgroup (p, y) moves its share of problem p's particles from x_in to
// x_out by the ancestors the filter stored for the problem's observation at a.k (the identity where the cloud was carried on), or
// unchanged where the problem has no observation there.
__global__ __launch_bounds__(256) void k_pf_gather(PfArgs a) {
  const int p = blockIdx.x, n = a.n_paths, D = a.D;
  const int j = pf_obs_at(a, p);
  const size_t nD = (size_t)n * D;
  const double* xin = a.x_in + (size_t)p * nD;
  double* xout = a.x_out + (size_t)p * nD;
  const int32_t* anc = j < 0 ? nullptr : a.h_anc + ((size_t)p * a.M + j) * n;
  for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < nD; e += (size_t)gridDim.y * 256) {
    const size_t i = e / D;
    xout[e] = anc ? xin[(size_t)anc[i] * D + (e - i * D)] : xin[e];
  }
}

// out [B][len] = the sum over the workgroups blk = 0 .. n_blocks-1 of part [B][n_blocks][len], added in that order
__global__ __launch_bounds__(256) void k_pf_moments_sum(int n_blocks, size_t len, size_t total, const double* part, double* out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;      // (one thread per entry of out, the problems behind one another)
  if (g >= total) return;
  const size_t p = g / len, e = g - p * len;
  const double* src = part + p * n_blocks * len + e;
  double s = 0.0;
  for (int blk = 0; blk < n_blocks; blk++) s += src[(size_t)blk * len];
  out[g] = s;
}

// packed [rows][V], V = D + D (D + 1) / 2 (the mean, then the lower triangle by rows) -> mean [rows][D], second [rows][D][D]: one thread per
// entry of second, (a, b) and (b, a) from the one packed entry; the threads of column 0 also carry the mean over
__global__ __launch_bounds__(256) void k_pf_cov_unpack(int D, size_t total, const double* packed, double* mean, double* second) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const size_t DD = (size_t)D * D, row = g / DD, e = g - row * DD, ea = e / D, eb = e - ea * D;
  const size_t hi = ea > eb ? ea : eb, lo = ea > eb ? eb : ea;
  const double* src = packed + row * ((size_t)D + (size_t)D * (D + 1) / 2);
  second[g] = src[D + hi * (hi + 1) / 2 + lo];
  if (eb == 0) mean[row * D + ea] = src[ea];
}

// ---- the smoothing trajectories: the final slots, their genealogy (the lineage walk is an instantiation of the samplers above) ----------
// The final slots of K equally weighted trajectories, one workgroup per problem with c observations of its own:
// systematic resampling from the final weights as k_pf_resample does it -- w_i = exp(lw_i - max lw), cum and S = cum_{n-1} by the same
// code -- with K thresholds u_m = (U + m) / K S, U from Philox counter (Np, 0, p, 0xffffffff): the filter's own draws have grid indices
// below Np.  table [B][rows][K]: row c gets min(#{i: cum_i <= u_m}, n - 1).
__global__ __launch_bounds__(256) void k_pf_pick(PfArgs a, int Np, int K, int rows, int32_t* table) {
  __shared__ double tot[4], red[4];
  const int p = blockIdx.x, n = a.n_paths;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  const double* lw = a.lw + (size_t)p * n;
  double* cum = a.cum + (size_t)p * n;
  const double mx = pf_max(lw, n, red);
  (void)pf_prefix_sums(lw, n, mx, cum, tot);
  __syncthreads();      // (cum is written)
  const double S = cum[n - 1];
  uint32_t r[4];
  philox4x32_10((uint32_t)Np, 0u, (uint32_t)p, 0xffffffffu, (uint32_t)(a.seed & 0xffffffffu), (uint32_t)(a.seed >> 32), r);
  const double U = unit_open(r[0], r[1]);
  int32_t* row = table + ((size_t)p * rows + cnt) * K;
  for (int m = threadIdx.x; m < K; m += 256) {
    const double um = (U + (double)m) / (double)K * S;
    row[m] = pf_bisect(cum, n, um);
  }
}

// The genealogy of the final slots, one thread per (problem, trajectory): from row c of table [B][rows][K] backwards, s_j = anc_j[s_{j+1}]
// where the cloud was resampled at the problem's observation j (h_anc, h_flag: the filter's histories), else s_{j+1}.
__global__ __launch_bounds__(256) void k_pf_trace(PfArgs a, int K, int rows, int32_t* table) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)a.batch * K) return;
  const int p = (int)(g / K), m = (int)(g - (size_t)p * K), n = a.n_paths;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  int32_t* col = table + (size_t)p * rows * K + m;
  int s = col[(size_t)cnt * K];
  for (int j = cnt - 1; j >= 0; j--) {
    const size_t hj = (size_t)p * a.M + j;
    if (a.h_flag[hj]) s = a.h_anc[hj * n + s];
    col[(size_t)j * K] = s;
  }
}

// What the two Gumbel-max draws share (k_pf_backward, k_pf_cresample): the score of a candidate with log-weight lw, quadratic form `quad` of its
// transition density and uniform u; and whether (score, slot) beats the best so far -- the larger score, of equal scores the smaller slot.
__device__ __forceinline__ double pf_gumbel_score(double lw, double quad, double u) { return (lw - 0.5 * quad) + -log(-log(u)); }
__device__ __forceinline__ bool pf_beats(double sc, int slot, double best, int bslot) { return sc > best || (sc == best && slot < bslot); }

// ---- backward simulation: the slot table of vgpa_particle_backward_paths, in the trace's place -------------------------
// Workgroup (p, blk) owns the kBackwardBlock trajectories m = blk kBackwardBlock + mm of problem p and walks that problem's cuts
// j = c-1 .. 0 itself: one launch, nothing between workgroups.  Where the cloud was carried on, row j of the table is row j + 1.  Where it
// was resampled (k = t_j < Np-1):
//   x~   thread e < kBackwardBlock D forms component e mod D of trajectory e / D's next state in plain fp64, (z + dt (b_k - A_k z)) + R_dd xi
//        with z = clouds_j[anc_j[s]], s the trajectory's slot in stretch j + 1, xi the sampler's normal of counter (k + 1, s, p, .); to LDS;
//   mu   the n candidates go through LDS 256 at a time: a tile of clouds_j is 256 D consecutive doubles, loaded in that order and written
//        component-major with a row stride of 257 doubles (consecutive components of a candidate fall into consecutive bank pairs; a
//        thread's own column is read without conflict).  Thread t owns candidate base + t and forms its transition mean x + dt f(x) once
//        per tile -- D = 1, 3: model_drift<DC> in registers; DC = 0: Lorenz-96 of any D, circular on the candidate's own column, in place
//        behind three rolling registers as in k_sample_l96 -- for all of the block's trajectories;
//   b    sum_d ((x~_d - mu_d) (1 / R_dd))^2 for the block's trajectories side by side, mu_d read once per d; b = hlw_j[i] - sum / 2;
//   g    -log(-log u): the lanes of candidates 2 q and 2 q + 1 share the Philox call of counter (k, m, p, 0x80000000 | q) -- the even lane
//        makes it for trajectory mm, the odd one for mm + 1, and each hands the half it does not use to its partner;
//   max  each thread keeps (score, slot) of its best candidate per trajectory; a butterfly over the wave and four LDS words over the
//        workgroup keep the larger score and, of equal scores, the smaller slot: the smallest i that attains the maximum, whatever the
//        tiling.
// A trajectory behind the last one is the last one again and stores nothing.
template <int DC>
__global__ __launch_bounds__(256) void k_pf_backward(PfArgs f, SampleArgs a, int K, int rows, int32_t* table) {
  constexpr int TB = kBackwardBlock, LD = 257;
  extern __shared__ double lds[];
  const int D = DC > 0 ? DC : a.D;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = f.n_paths, odd = lane & 1;
  const uint32_t p = blockIdx.x;
  double* tile = lds;                           // [D][LD]
  double* xt = tile + (size_t)D * LD;           // [TB][D]
  double* ir = xt + TB * D;                     // [D] 1 / R_dd
  double* rbest = ir + D;                       // [4 waves][TB]
  int* rslot = reinterpret_cast<int*>(rbest + 4 * TB);      // [4 waves][TB]
  int* scur = rslot + 4 * TB;                   // [TB] the block's slots in the stretch behind the cut
  const int cnt = f.n_obs_v ? f.n_obs_v[p] : f.n_obs;
  const int64_t* t = f.obs_t + (size_t)p * f.obs_t_stride;
  const uint32_t k0 = (uint32_t)(f.seed & 0xffffffffu), k1 = (uint32_t)(f.seed >> 32);
  const double* Rp = a.R + (size_t)p * a.R_stride;
  double th[kMaxTheta];
#pragma unroll
  for (int i = 0; i < kMaxTheta; i++) th[i] = a.theta_v ? a.theta_v[(size_t)p * kMaxTheta + i] : a.theta[i];
  const int m0 = blockIdx.y * TB;
  if (tid < TB) scur[tid] = table[((size_t)p * rows + cnt) * K + (m0 + tid < K ? m0 + tid : K - 1)];
  if (tid < D) ir[tid] = 1.0 / Rp[tid * D + tid];
  __syncthreads();
  for (int j = cnt - 1; j >= 0; j--) {
    const size_t hj = (size_t)p * f.M + j;
    int32_t* row = table + ((size_t)p * rows + j) * K;
    if (!f.h_flag[hj]) {      // (uniform over the workgroup)
      if (tid < TB && m0 + tid < K) row[m0 + tid] = scur[tid];
      continue;
    }
    const int k = (int)t[j];
    const double* cloud = f.h_clouds + hj * n * D;
    const int32_t* anc = f.h_anc + hj * n;
    const double* hlw = f.h_lw + hj * n;
    const double* Ak = a.A + (size_t)p * a.stride_x + (size_t)k * D * D;
    const double* bk = a.b + (size_t)p * a.stride_x + (size_t)k * D;
    for (int e = tid; e < TB * D; e += 256) {
      const int mm = e / D, d = e - mm * D;
      const uint32_t s = (uint32_t)scur[mm];
      const double* z = cloud + (size_t)anc[s] * D;
      double sum = 0.0, z0, z1;
      for (int c = 0; c < D; c++) sum += Ak[d * D + c] * z[c];
      normal_pair(k0, k1, (uint32_t)k + 1u, s, p, (uint32_t)(d >> 1), &z0, &z1);
      xt[e] = (z[d] + a.dt * (bk[d] - sum)) + Rp[d * D + d] * ((d & 1) ? z1 : z0);
    }
    double best[TB];
    int bslot[TB];
#pragma unroll
    for (int mm = 0; mm < TB; mm++) { best[mm] = -INFINITY; bslot[mm] = 0x7fffffff; }
    for (int base = 0; base < n; base += 256) {
      __syncthreads();      // (x~ is written; the columns of the tile before have been read)
      const int nt = n - base < 256 ? n - base : 256;
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
      double acc[TB];
#pragma unroll
      for (int mm = 0; mm < TB; mm++) acc[mm] = 0.0;
      if (mine) {
        for (int d = 0; d < D; d++) {
          double md;
          if constexpr (DC > 0) md = mu[d]; else md = col[d * LD];
          const double ird = ir[d];
#pragma unroll
          for (int mm = 0; mm < TB; mm++) { const double v = (xt[mm * D + d] - md) * ird; acc[mm] += v * v; }
        }
      }
      const double lwi = mine ? hlw[i] : 0.0;
#pragma unroll
      for (int mm = 0; mm < TB; mm += 2) {
        const int m = m0 + mm + odd;
        uint32_t r[4];
        philox4x32_10((uint32_t)k, (uint32_t)(m < K ? m : K - 1), p, 0x80000000u | ((uint32_t)i >> 1), k0, k1, r);
        const double ua = unit_open(r[0], r[1]), ub = unit_open(r[2], r[3]);
        const double got = __shfl_xor(odd ? ua : ub, 1);
        const double u[2] = {odd ? got : ua, odd ? ub : got};      // this candidate's uniforms of trajectories mm and mm + 1
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const double sc = pf_gumbel_score(lwi, acc[mm + h], u[h]);
          if (mine && pf_beats(sc, i, best[mm + h], bslot[mm + h])) { best[mm + h] = sc; bslot[mm + h] = i; }
        }
      }
    }
#pragma unroll
    for (int mm = 0; mm < TB; mm++) {
      double v = best[mm];
      int sl = bslot[mm];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int os = __shfl_xor(sl, o);
        if (pf_beats(ov, os, v, sl)) { v = ov; sl = os; }
      }
      if (lane == 0) { rbest[w * TB + mm] = v; rslot[w * TB + mm] = sl; }
    }
    __syncthreads();
    if (tid < TB) {
      double v = rbest[tid];
      int sl = rslot[tid];
      for (int q = 1; q < 4; q++) {
        const double ov = rbest[q * TB + tid];
        const int os = rslot[q * TB + tid];
        if (pf_beats(ov, os, v, sl)) { v = ov; sl = os; }
      }
      sl = sl < n ? sl : n - 1;      // (no finite score at all: any slot of the cloud)
      scur[tid] = sl;
      if (m0 + tid < K) row[m0 + tid] = sl;
    }
    __syncthreads();
  }
}

// ---- particle Gibbs: the step between two segments of the conditional filter, the reference's stretches of the result ---
// component d of x + dt f(x; theta): the transition mean of the model SDE from one particle's D states (Lorenz-96 circular on them)
__device__ __forceinline__ double pf_transition_mean(int model, const double* th, const double* x, int D, int d, double dt) {
  double f;
  if (model == VGPA_MODEL_OU) f = -th[0] * x[0];
  else if (model == VGPA_MODEL_DW) f = 4.0 * x[0] * (th[0] - x[0] * x[0]);
  else if (model == VGPA_MODEL_L63) f = d == 0 ? th[0] * (x[1] - x[0]) : d == 1 ? (th[1] - x[2]) * x[0] - x[1] : x[0] * x[1] - th[2] * x[2];
  else {
    const int up = d + 1 < D ? d + 1 : 0, d1 = d >= 1 ? d - 1 : D - 1, d2 = d >= 2 ? d - 2 : D - 2 + d;
    f = (x[up] - x[d2]) * x[d1] - x[d] + th[0];
  }
  return x[d] + dt * f;
}

// k_pf_resample<false> with slot 0 pinned, one workgroup per problem at grid index f.k.  The decision, ESS, cum, S and lw_new are that
// kernel's, over all n slots.  Where the cloud is resampled:
//   slots i >= 1  multinomial: anc_i = pf_bisect(cum, n, u_i S), u_i = unit_open(r0, r1) of Philox counter (k, i, p, 0xfffffffe).  Systematic
//                 resampling with one slot forced is no valid conditional resampling (Chopin & Singh 2015): its n thresholds are one
//                 draw, and conditioning on where one of them fell changes the law of all others.  Independent draws are exchangeable,
//                 so pinning one of them leaves the rest as they are.
//   slot 0        ancestor sampling (Lindsten, Jordan & Schoen 2014): x~ = ref[p][k + 1]; for every candidate i < n, slot 0 included,
//                 b_i = lw_i - 1/2 sum_d ((x~_d - mu_i,d) (1 / R_dd))^2 with lw_i before the reset and mu_i = x_i + dt f(x_i; theta_p);
//                 g_i = -log(-log u_i), u_i from Philox counter (k, 0, p, 0x40000000 | (i >> 1)): unit_open(r0, r1) for even i,
//                 unit_open(r2, r3) for odd i; anc_0 = the smallest i that attains max (b_i + g_i) -- k_pf_backward's score and comparison
//                 for one trajectory and one cut.  Thread t scores the candidates t, t + 256, ... from x_in in global memory
//   x_out_0 = x_in_0: the pinned slot keeps the reference's state; anc_0 goes into the history alone.  lw_i = lw_new for every slot.
__global__ __launch_bounds__(256) void k_pf_cresample(PfArgs a, SampleArgs s) {
  __shared__ double tot[4], red[4], rbest[4], ir[kMaxSmallD];
  __shared__ int rslot[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n_paths, D = a.D;
  const int j = pf_obs_at(a, p);
  const size_t nD = (size_t)n * D;
  const double* xin = a.x_in + (size_t)p * nD;
  double* xout = a.x_out + (size_t)p * nD;
  if (j < 0) {      // (uniform over the workgroup)
    for (size_t e = tid; e < nD; e += 256) xout[e] = xin[e];
    return;
  }
  double* lw = a.lw + (size_t)p * n;
  double* cum = a.cum + (size_t)p * n;
  int32_t* anc = a.anc + (size_t)p * n;
  const double mx = pf_max(lw, n, red);
  double s2 = pf_prefix_sums(lw, n, mx, cum, tot);
  __syncthreads();      // (cum is written; red has been read)
  const double S = cum[n - 1];
  s2 = wave_sum(s2);
  if (lane == 0) red[w] = s2;
  __syncthreads();
  s2 = (red[0] + red[1]) + (red[2] + red[3]);
  const double ess = S * S / s2;
  const bool go = ess < a.ess_fraction * (double)n && !a.last;
  const size_t hj = (size_t)p * a.M + j;
  if (tid == 0) { a.h_ess[hj] = ess; a.h_flag[hj] = go ? 1 : 0; }
  if (a.h_clouds)
    for (size_t e = tid; e < nD; e += 256) a.h_clouds[hj * nD + e] = xin[e];
  const uint32_t k0 = (uint32_t)(a.seed & 0xffffffffu), k1 = (uint32_t)(a.seed >> 32);
  int anc0 = 0;
  if (go) {      // (uniform over the workgroup; k < Np - 1: ref[p][k + 1] exists)
    const double* xt = a.ref + ((size_t)p * a.Np + (size_t)a.k + 1) * D;
    const double* Rp = s.R + (size_t)p * s.R_stride;
    double th[kMaxTheta];
#pragma unroll
    for (int i = 0; i < kMaxTheta; i++) th[i] = s.theta_v ? s.theta_v[(size_t)p * kMaxTheta + i] : s.theta[i];
    if (tid < D) ir[tid] = 1.0 / Rp[tid * D + tid];
    __syncthreads();
    double best = -INFINITY;
    int bslot = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {
      const double* xi = xin + (size_t)i * D;
      double quad = 0.0;
      for (int d = 0; d < D; d++) {
        const double v = (xt[d] - pf_transition_mean(s.model, th, xi, D, d, s.dt)) * ir[d];
        quad += v * v;
      }
      uint32_t r[4];
      philox4x32_10((uint32_t)a.k, 0u, (uint32_t)p, 0x40000000u | ((uint32_t)i >> 1), k0, k1, r);
      const double u = (i & 1) ? unit_open(r[2], r[3]) : unit_open(r[0], r[1]);
      const double sc = pf_gumbel_score(lw[i], quad, u);
      if (pf_beats(sc, i, best, bslot)) { best = sc; bslot = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int os = __shfl_xor(bslot, o);
      if (pf_beats(ov, os, best, bslot)) { best = ov; bslot = os; }
    }
    if (lane == 0) { rbest[w] = best; rslot[w] = bslot; }
    __syncthreads();      // (every lw_i has been read: the loop below replaces them)
    best = rbest[0]; bslot = rslot[0];
    for (int q = 1; q < 4; q++)
      if (pf_beats(rbest[q], rslot[q], best, bslot)) { best = rbest[q]; bslot = rslot[q]; }
    anc0 = bslot < n ? bslot : n - 1;      // (no finite score at all: any slot of the cloud)
  }
  const double lw_new = mx + log(S) - log((double)n);
  for (int i = tid; i < n; i += 256) {
    int from = i, hist = i;
    if (go) {
      if (i == 0) hist = anc0;
      else {
        uint32_t r[4];
        philox4x32_10((uint32_t)a.k, (uint32_t)i, (uint32_t)p, 0xfffffffeu, k0, k1, r);
        from = hist = pf_bisect(cum, n, unit_open(r[0], r[1]) * S);
      }
      if (a.h_lw) a.h_lw[hj * n + i] = lw[i];
      lw[i] = lw_new;
    }
    anc[i] = from;
    if (a.h_anc) a.h_anc[hj * n + i] = hist;
  }
  __syncthreads();
  for (size_t e = tid; e < nD; e += 256) {
    const size_t i = e / D;
    xout[e] = xin[(size_t)anc[i] * D + (e - i * D)];
  }
}

// out [B][Np][D] (one trajectory per problem, stride 1) = ref wherever the trajectory sat in slot 0: grid index k lies in stretch
// j(k) = #{observations of the problem before k}, row j(k) of table [B][rows][1].  One thread per entry.
__global__ __launch_bounds__(256) void k_pf_ref_fill(PfArgs a, int rows, const int32_t* table, double* out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.Np * a.D;
  if (g >= (size_t)a.batch * per) return;
  const size_t p = g / per;
  const int64_t k = (int64_t)((g - p * per) / a.D);
  const int64_t* t = a.obs_t + p * a.obs_t_stride;
  const int cnt = a.n_obs_v ? a.n_obs_v[p] : a.n_obs;
  int j = 0;
  for (int m = 0; m < cnt; m++) j += t[m] < k ? 1 : 0;
  if (table[p * rows + j] == 0) out[g] = a.ref[g];
}

// One walk at the D of the arguments: k_sample_small<D, K> up to D = 4 (one lane per path; the replay: the problem in grid.x, 256 slots per
// workgroup in grid.y), above it k_sample_mfma<NT, K> with NT the next multiple of 16 (grid: problems x 64 paths).  D = 2 exists for the
// plain walk only: every other walk needs a stochastic model, and none has D = 2.  (Twelve walks: 3 instantiations of k_sample_small each
// and one more for Plain, 4 of k_sample_mfma each but Forecast.)
template <Walk K>
hipError_t launch_walk(const SampleArgs& base, hipStream_t st, const WalkOwn& own) {
  WalkArgs<K> a;
  static_cast<SampleArgs&>(a) = base;
  if constexpr (K == Walk::Conditional) a.pf_ref = own.pf_ref;
  if constexpr (K == Walk::SegmentEvents) { a.ev_level = own.ev_level; a.ev_side = own.ev_side; }
  if constexpr (K == Walk::ReplayMarginals) { a.mg_level = own.mg->levels; a.mg_L = own.mg->L; a.mg_qtab = own.mg->qtab; a.mg_mass = own.mg->mass; }
  if (a.D <= kMaxLaneD) {
    const dim3 grid = kWalkTraits[(int)K].by_problem() ? dim3(a.batch, sample_segment_blocks(a.D, a.n_paths))
                                        : dim3((unsigned)(((size_t)a.batch * a.n_paths + 255) / 256));
    return with_int<1, kMaxLaneD>(a.D, [&](auto d) {      // (launch_sample_walk has refused D < 1)
      constexpr int D = decltype(d)::value;
      if constexpr (D != 2 || K == Walk::Plain) {
        hipLaunchKernelGGL((k_sample_small<D, K>), grid, dim3(256), 0, st, a);
        return hipGetLastError();
      } else {
        return hipErrorInvalidValue;
      }
    });
  }
  if constexpr (K == Walk::Forecast) {      // (the matrix-core kernel is posterior kind only: above D = 4 the forecast is Lorenz-96's own kernel)
    hipLaunchKernelGGL(k_forecast_l96, dim3(a.batch, sample_segment_blocks(a.D, a.n_paths)), dim3(64), ((size_t)a.D + 1) * 64 * sizeof(double), st, a);
    return hipGetLastError();
  } else {
    if (a.n_paths > sample_max_paths(a.D)) return hipErrorInvalidValue;
    return with_int<1, kMaxSmallD / 16>((a.D + 15) / 16, [&](auto tiles) {      // (launch_sample_walk has refused D > 64)
      constexpr int NT = 16 * decltype(tiles)::value;
      // (ReplayCov: the [4 waves][NT] words of the mean behind the Zs region)
      const size_t lds = (MfmaShape<NT>::lds_doubles(!a.R_diag) + (kWalkTraits[(int)K].kept == Kept::Covariance ? 4 * NT : 0)) * sizeof(double);
      return launch_lds(k_sample_mfma<NT, K>, dim3(a.batch, sample_segment_blocks(a.D, a.n_paths)), dim3(256), lds, st, a);
    });
  }
}

}  // namespace

hipError_t launch_pf_start(const PfArgs& a, hipStream_t st) {
  if (a.D < 1 || a.D > kMaxSmallD || a.n_paths < 1 || !a.x || !a.ws || !a.lw || (!a.x0 && !(a.m0 && a.L0)) || (a.mu0 && !a.Lt)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_start, dim3((unsigned)(((size_t)a.batch * a.n_paths + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pf_resample(const PfArgs& a, hipStream_t st) {
  if (a.D < 1 || a.n_paths < 1 || !a.x_in || !a.x_out || a.x_in == a.x_out || !a.lw || !a.cum || !a.anc || !a.h_ess || !a.h_flag) return hipErrorInvalidValue;
  if ((a.st_in == nullptr) != (a.st_out == nullptr) || (a.st_in && a.st_in == a.st_out)) return hipErrorInvalidValue;
  if (a.st_in) hipLaunchKernelGGL(k_pf_resample<true>, dim3(a.batch), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_pf_resample<false>, dim3(a.batch), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pf_pin(const PfArgs& a, hipStream_t st) {
  if (a.D < 1 || a.D > kMaxSmallD || a.batch < 1 || a.n_paths < 1 || a.Np < 1 || !a.ref || !a.x || !a.ws || !a.lw || (!a.x0 && !(a.m0 && a.L0)) || (a.mu0 && !a.Lt))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_pin, dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pf_cresample(const PfArgs& f, const SampleArgs& a, hipStream_t st) {
  if (f.D < 1 || f.D > kMaxSmallD || f.n_paths < 1 || !f.x_in || !f.x_out || f.x_in == f.x_out || !f.lw || !f.cum || !f.anc || !f.h_ess || !f.h_flag) return hipErrorInvalidValue;
  if (f.st_in || f.st_out || !f.ref || f.Np < 1 || f.k < 0 || f.k >= f.Np || (!f.last && f.k + 1 >= f.Np)) return hipErrorInvalidValue;
  if (a.D != f.D || !a.R || !a.R_diag) return hipErrorInvalidValue;
  const bool model_fits = (a.D == 1 && (a.model == VGPA_MODEL_OU || a.model == VGPA_MODEL_DW)) || (a.D == 3 && a.model == VGPA_MODEL_L63) ||
                          (a.D >= 3 && a.model == VGPA_MODEL_L96);
  if (!model_fits) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_cresample, dim3(f.batch), dim3(256), 0, st, f, a);
  return hipGetLastError();
}

hipError_t launch_pf_ref_fill(const PfArgs& f, int rows, const int32_t* table, double* out, hipStream_t st) {
  const size_t total = (size_t)f.batch * (size_t)(f.Np > 0 ? f.Np : 0) * (size_t)f.D;
  if (f.batch < 1 || f.D < 1 || f.Np < 1 || rows < 1 || !pf_flat_grid_fits(total) || !f.ref || !f.obs_t || !table || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_ref_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, f, rows, table, out);
  return hipGetLastError();
}

// the slots of a problem in grid.y, 256 per workgroup up to D = 4 and 64 above it; one-dimensional grids in grid.x
static int segment_slots(int D) { return D <= kMaxLaneD ? 256 : 64; }
int sample_segment_blocks(int D, int n_paths) { return (n_paths + segment_slots(D) - 1) / segment_slots(D); }
int sample_max_paths(int D) { return kMaxGridY * segment_slots(D); }
bool pf_flat_grid_fits(size_t entries) { return (entries + 255) / 256 <= 0x7fffffffu; }

hipError_t launch_pf_descend(const PfArgs& a, int rows, double* wtab, double* less, hipStream_t st) {
  if (a.batch < 1 || a.n_paths < 1 || a.M < 1 || rows < a.M + 1 || !a.lw || !a.h_flag || !a.h_anc || !wtab || !less) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_descend, dim3(a.batch), dim3(256), 0, st, a, rows, wtab, less);
  return hipGetLastError();
}

hipError_t launch_pf_quantise(const PfArgs& a, int rows, const double* wtab, uint64_t* qtab, uint64_t* qfinal, hipStream_t st) {
  const size_t lanes = (size_t)(a.batch > 0 ? a.batch : 0) * (size_t)(a.n_paths > 0 ? a.n_paths : 0);
  if (a.batch < 1 || a.n_paths < 1 || a.M < 1 || rows < a.M + 1 || !pf_flat_grid_fits(lanes) || !wtab || !qtab || !qfinal) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_quantise, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, rows, wtab, qtab, qfinal);
  return hipGetLastError();
}

hipError_t launch_pf_descend_q(const PfArgs& a, int rows, uint64_t* qtab, hipStream_t st) {
  if (a.batch < 1 || a.n_paths < 1 || a.M < 1 || rows < a.M + 1 || !a.h_flag || !a.h_anc || !qtab) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_descend_q, dim3(a.batch), dim3(256), 0, st, a, rows, qtab);
  return hipGetLastError();
}

hipError_t launch_pf_gather(const PfArgs& a, hipStream_t st) {
  if (a.D < 1 || a.batch < 1 || a.n_paths < 1 || !a.x_in || !a.x_out || a.x_in == a.x_out || !a.h_anc) return hipErrorInvalidValue;
  const size_t nD = (size_t)a.n_paths * a.D;
  const unsigned shares = (unsigned)((nD + 1023) / 1024 < 64 ? (nD + 1023) / 1024 : 64);
  hipLaunchKernelGGL(k_pf_gather, dim3(a.batch, shares), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pf_moments_sum(int batch, int n_blocks, size_t len, const double* part, double* out, hipStream_t st) {
  const size_t total = (size_t)batch * len;
  if (batch < 1 || n_blocks < 1 || len < 1 || !pf_flat_grid_fits(total) || !part || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_moments_sum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n_blocks, len, total, part, out);
  return hipGetLastError();
}

hipError_t launch_pf_cov_unpack(int D, size_t rows, const double* packed, double* mean, double* second, hipStream_t st) {
  const size_t total = rows * (size_t)D * D;
  if (D < 1 || D > kMaxSmallD || rows < 1 || !pf_flat_grid_fits(total) || !packed || !mean || !second) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_cov_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, total, packed, mean, second);
  return hipGetLastError();
}

hipError_t launch_pf_pick(const PfArgs& a, int Np, int K, int rows, int32_t* table, hipStream_t st) {
  if (a.batch < 1 || a.n_paths < 1 || Np < 1 || K < 1 || rows < 1 || !a.lw || !a.cum || !table) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_pick, dim3(a.batch), dim3(256), 0, st, a, Np, K, rows, table);
  return hipGetLastError();
}

hipError_t launch_pf_trace(const PfArgs& a, int K, int rows, int32_t* table, hipStream_t st) {
  const size_t lanes = (size_t)a.batch * (K > 0 ? K : 0);
  if (a.batch < 1 || a.n_paths < 1 || a.M < 1 || K < 1 || rows < 1 || !pf_flat_grid_fits(lanes) || !a.h_flag || !a.h_anc || !table)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_trace, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, K, rows, table);
  return hipGetLastError();
}

hipError_t launch_pf_backward(const PfArgs& f, const SampleArgs& a, int K, int rows, int32_t* table, hipStream_t st) {
  if (f.batch < 1 || f.n_paths < 1 || f.M < 1 || K < 1 || rows < 1 || !pf_backward_fits(K) || !f.h_flag || !f.h_anc || !f.h_clouds || !f.h_lw || !table)
    return hipErrorInvalidValue;
  if (a.D < 1 || a.D > kMaxSmallD || a.D != f.D || !a.A || !a.b || !a.R || !a.R_diag) return hipErrorInvalidValue;
  const dim3 grid(f.batch, (K + kBackwardBlock - 1) / kBackwardBlock), block(256);
  const size_t lds = ((size_t)a.D * 257 + (size_t)kBackwardBlock * a.D + a.D + 4 * kBackwardBlock) * sizeof(double) + 5 * kBackwardBlock * sizeof(int);
  auto kern = a.model == VGPA_MODEL_L96 && a.D >= 3                            ? k_pf_backward<0>      // (the circular drift on a column of any length)
              : a.D == 1 && (a.model == VGPA_MODEL_OU || a.model == VGPA_MODEL_DW) ? k_pf_backward<1>
              : a.D == 3 && a.model == VGPA_MODEL_L63                              ? k_pf_backward<3>
                                                                                   : nullptr;
  if (!kern) return hipErrorInvalidValue;
  return launch_lds(kern, grid, block, lds, st, f, a, K, rows, table);
}

hipError_t launch_pf_normalise(int batch, int n_paths, const double* lw, double* w, hipStream_t st) {
  if (batch < 1 || n_paths < 1 || !lw || !w) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_normalise, dim3(batch), dim3(256), 0, st, n_paths, lw, w);
  return hipGetLastError();
}

bool sample_lineages_fit(int D, int batch, int K) {
  return D <= kMaxLaneD ? pf_flat_grid_fits((size_t)batch * K) : K <= sample_max_paths(D);
}

hipError_t launch_pf_stats_mean(int D, int batch, int n_paths, const double* lw, const double* stats, double* mean, hipStream_t st) {
  if (D < 1 || D > kMaxSmallD || batch < 1 || n_paths < 1 || !lw || !stats || !mean) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_stats_mean, dim3(batch, 3), dim3(256), 0, st, D, n_paths, lw, stats, mean);
  return hipGetLastError();
}

hipError_t launch_pf_events_start(int D, int batch, int n_paths, int Np, const double* x, const double* level, const int32_t* side, double* rows,
                                  hipStream_t st) {
  const size_t total = (size_t)(batch > 0 ? batch : 0) * (size_t)(n_paths > 0 ? n_paths : 0) * (size_t)(D > 0 ? D : 0);
  if (D < 1 || D > kMaxSmallD || batch < 1 || n_paths < 1 || Np < 1 || !pf_flat_grid_fits(total) || !x || !level || !side || !rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_events_start, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, D, n_paths, Np, total, x, level, side, rows);
  return hipGetLastError();
}

hipError_t launch_pf_events_cdf(int D, int batch, int n_paths, int Np, int stride, const double* lw, const double* rows, double* cdf, hipStream_t st) {
  if (D < 1 || D > kMaxSmallD || batch < 1 || n_paths < 1 || Np < 1 || stride < 1 || !lw || !rows || !cdf) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pf_events_cdf, dim3(batch, D), dim3(256), 0, st, D, n_paths, Np, stride, lw, rows, cdf);
  return hipGetLastError();
}

// The walk is what the caller says it is; the fields that walk reads must be set, and the fields that would have meant another walk must not.
hipError_t launch_sample_walk(Walk w, const SampleArgs& a, hipStream_t st, const WalkOwn& own) {
  if (a.D < 1 || a.D > kMaxSmallD || a.n_paths < 1) return hipErrorInvalidValue;
  const bool known_model = a.model == VGPA_MODEL_OU || a.model == VGPA_MODEL_DW || a.model == VGPA_MODEL_L63 || a.model == VGPA_MODEL_L96;
  // the weighted kind: the posterior process with diagonal factors against the model's drift; above D = 4 the model is Lorenz-96
  const bool weighable = a.kind == VGPA_PATHS_POSTERIOR && a.R_diag && known_model && (a.D <= kMaxLaneD || a.model == VGPA_MODEL_L96);
  const bool segment = weighable && a.pf_x && a.pf_lw && a.k_begin >= 0 && a.k_end >= a.k_begin && a.k_end < a.Np;
  // what is one walk's alone: the histories Backward's (and the sums never its), the reference Conditional's, the levels and sides
  // SegmentEvents', the ladders, integer weights and masses ReplayMarginals'
  const bool foreign = (w == Walk::Backward ? a.pf_wtab || a.pf_part : a.pf_clouds || a.pf_hanc) || (w != Walk::Conditional && own.pf_ref) ||
                       (w != Walk::SegmentEvents && (own.ev_level || own.ev_side)) || (w != Walk::ReplayMarginals && own.mg);
  if (foreign) return hipErrorInvalidValue;
  const MarginalArgs* mg = own.mg;
  switch (w) {
    case Walk::Plain: {
      if (a.stride < 1 || a.logw) return hipErrorInvalidValue;
      if (a.D <= kMaxLaneD || a.kind == VGPA_PATHS_POSTERIOR) return launch_walk<Walk::Plain>(a, st, own);
      if (a.model != VGPA_MODEL_L96) return hipErrorInvalidValue;
      const size_t lanes = (size_t)a.batch * a.n_paths, lds = (size_t)a.D * 64 * sizeof(double) * ((!a.R_diag || !a.x0) ? 2 : 1);
      hipLaunchKernelGGL(k_sample_l96, dim3((unsigned)((lanes + 63) / 64)), dim3(64), lds, st, a);
      return hipGetLastError();
    }
    case Walk::Weighted:
      if (a.stride < 1 || !a.logw || !a.start || !weighable) return hipErrorInvalidValue;
      return launch_walk<Walk::Weighted>(a, st, own);
    case Walk::Segment:
      if (!segment || a.pf_stats || a.pf_wtab) return hipErrorInvalidValue;
      return launch_walk<Walk::Segment>(a, st, own);
    case Walk::SegmentStats:
      if (!segment || !a.pf_stats || a.pf_wtab) return hipErrorInvalidValue;
      return launch_walk<Walk::SegmentStats>(a, st, own);
    case Walk::Conditional:      // (the segment's fields and the reference)
      if (!segment || a.pf_stats || a.pf_wtab || !own.pf_ref) return hipErrorInvalidValue;
      return launch_walk<Walk::Conditional>(a, st, own);
    case Walk::SegmentEvents:      // (the fields of SegmentStats -- the rows are where pf_stats points -- and the levels and sides)
      if (!segment || !a.pf_stats || a.pf_wtab || !own.ev_level || !own.ev_side) return hipErrorInvalidValue;
      return launch_walk<Walk::SegmentEvents>(a, st, own);
    case Walk::Replay:
      if (!segment || !a.pf_wtab || a.pf_stats || !a.pf_part || a.stride < 1 || a.pf_rows < 1) return hipErrorInvalidValue;
      if (a.n_paths > sample_max_paths(a.D)) return hipErrorInvalidValue;
      return launch_walk<Walk::Replay>(a, st, own);
    case Walk::ReplayCov:      // (the replay's fields; pf_part holds sample_cov_len(D) doubles per kept index)
      if (!segment || !a.pf_wtab || a.pf_stats || !a.pf_part || a.stride < 1 || a.pf_rows < 1) return hipErrorInvalidValue;
      if (a.n_paths > sample_max_paths(a.D)) return hipErrorInvalidValue;
      return launch_walk<Walk::ReplayCov>(a, st, own);
    case Walk::ReplayMarginals:      // (the replay's fields without its weights and sums; the ladders, the integer weights, the masses)
      if (!segment || a.pf_wtab || a.pf_stats || a.pf_part || a.stride < 1 || a.pf_rows < 1 || a.n_keep < 1) return hipErrorInvalidValue;
      if (!mg || !mg->levels || !mg->qtab || !mg->mass || mg->L < 1 || mg->L > kMaxMarginalLevels) return hipErrorInvalidValue;
      if (a.n_paths > sample_max_paths(a.D)) return hipErrorInvalidValue;
      return launch_walk<Walk::ReplayMarginals>(a, st, own);
    case Walk::Lineage:
      if (a.stride < 1 || a.kind != VGPA_PATHS_POSTERIOR || !a.R_diag || !a.out || !a.pf_slots || a.pf_slot_rows < 1 || a.logw) return hipErrorInvalidValue;
      if (!sample_lineages_fit(a.D, a.batch, a.n_paths)) return hipErrorInvalidValue;
      return launch_walk<Walk::Lineage>(a, st, own);
    case Walk::Backward:      // (the lineage walk's fields and the histories)
      if (a.stride < 1 || a.kind != VGPA_PATHS_POSTERIOR || !a.R_diag || !a.out || !a.pf_slots || a.pf_slot_rows < 1 || a.logw) return hipErrorInvalidValue;
      if (!a.pf_clouds || !a.pf_hanc || a.pf_M < 1 || a.pf_n < 1 || !sample_lineages_fit(a.D, a.batch, a.n_paths)) return hipErrorInvalidValue;
      return launch_walk<Walk::Backward>(a, st, own);
    case Walk::Forecast: {
      const bool cloud = a.pf_part && a.pf_wtab && !a.out && !a.pf_slots && a.n_paths == a.pf_n;
      const bool members = a.out && a.pf_slots && a.pf_slot_rows == 1 && !a.pf_part && !a.pf_wtab;
      if (a.stride < 1 || a.kind != VGPA_PATHS_MODEL || !a.R_diag || !known_model || (a.D > kMaxLaneD && a.model != VGPA_MODEL_L96)) return hipErrorInvalidValue;
      if (!a.pf_x || a.pf_n < 1 || a.k_begin < 0 || a.k_end < a.k_begin || cloud == members || a.logw || a.pf_lw || a.pf_stats) return hipErrorInvalidValue;
      if (a.n_keep != (a.k_end - a.k_begin) / a.stride + 1 || a.n_paths > sample_max_paths(a.D)) return hipErrorInvalidValue;
      return launch_walk<Walk::Forecast>(a, st, own);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace vgpa
