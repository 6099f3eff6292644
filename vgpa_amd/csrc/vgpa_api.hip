// C ABI of libvgpa_hip.so (see include/vgpa_hip.h for the contract and the reference interfaces).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <limits>
#include <vector>

#include "vgpa_internal.h"

using namespace vgpa;

namespace {
thread_local std::string g_create_error;

// Where every problem reads every batch input (Rows: vgpa_internal.h).  vgpa_create points it at the shared values, vgpa_set_problem_data /
// vgpa_set_problem_params / vgpa_set_prior_energy at per-problem rows; nothing else writes it, and the argument builders copy from it.
// theta, sigma1, e0 and 1 / sigma^2 have no shared device row: null rows, and the kernels take the shared value (vgpa_ctx).
struct BatchInputs {
  Rows<double> m0, S0, obs_y, e0;      // [B][D], [B][D][D], [B][M][D], [B]
  Rows<int64_t> obs_t;                 // [B][M]
  Rows<int32_t> obs_idx;               // [B][Np] -> observation counter n, or -1
  Rows<double> theta, Sigma, isig, isg;   // [B][kMaxTheta], [B][D][D], [B][D][D] Sigma^-1, [B][D] its diagonal (above D = 64: theta only)
  Rows<double> sig1, qs;               // [B] 1-D sigma, [B] 1 / sigma_p^2 of an isotropic row
  // the observation model (vgpa_set_problem_obs_model): Q = H R^-1 H^T, K, diag R^-1, the constant matrix jump whole and as a packed lower
  // triangle (rows of D*D doubles both), the additive constant of E_obs and the observation count -- the last two null while shared
  Rows<double> Q, K, rinv, jsc, jscp, obs_const;   // [B][D][D] x2, [B][D], [B][D][D] x2, [B]
  Rows<int32_t> n_obs;                 // [B]
  std::vector<double> h_theta, h_isig, h_sig1, h_e0;  // host copies of the per-problem values (theta_of, isig_of, sigma1_of, e0_of)
  std::vector<double> h_Sigma, h_S0;   // ... and of the Sigma / S0 rows in force (empty: the shared one), which vgpa_sample_paths factorises
};

struct SigmaForm { bool diag = true, iso = true, sym = true; };   // of one Sigma: diagonal, sigma^2 I, symmetric

// the stepping kernels of one sweep direction: ld::ld_solve_* (D > 64), one lane per problem (ode_small.hip), 16 lanes per problem
// (ode_wave.hip), the matrix-core kernels (launch_ode_mfma, which takes Plan::sym_units), one workgroup per problem (ode_generic.hip)
enum class Stepper { LargeD, Lane, Wave, Mfma, Generic };

// Which kernels a context's fused sweep runs, and in which layout the arrays travel between them.  make_plan() derives it from cfg, D,
// B, the CU count, the form of the inputs in force and the environment -- in vgpa_create and again when vgpa_set_problem_data /
// vgpa_set_problem_params change the inputs; nothing else writes it.  (DESIGN.md s.4.0 has the table.)
struct Plan {
  bool sigma_diag = true, isg_iso = false, sym_inputs = true;   // the inputs in force: Sigma diagonal, sigma^2 I; every s0 / Sigma / constant jump symmetric
  bool sym_units = false;       // matrix-core family: symmetric-unit kernels, not the role-specialised ones; heads the layout chain below
  bool launch_sym_units = false;   // what launch_ode_mfma is told (OdeArgs::sym_units): sym_units, or VGPA_ODE_KERNEL=sym, which leaves the layouts alone
  // ... and the sets of helper waves it is told to put beside the product waves of the fragment-cover steppers (k_ode_sym, HLP / H2): 0, 1 or
  // 2; 0 wherever launch_ode_mfma's steppers are not those.  (The backward kernel with the gradient waves keeps its fixed 768-thread shape
  // -- one helper role and the gradient waves -- whatever the count says.)
  int helper_roles = 0;
  Stepper fwd = Stepper::Generic, bwd = Stepper::Generic;
  bool lane_pass = false;      // the objective is the fused lane pass (enqueue_lane_sweep)
  // the layout chain of the fragment-cover kernels, each step implying the one before:
  bool bwd_upper = false;       // the backward kernel reads the upper triangle of dEsde_dS only: the energy kernel writes nothing else
  bool store_q = false;         // ... and stores Q''_t instead of Psi_t (OdeArgs::q_on)
  bool packed = false;          // ... S_t and dEsde_dS travel as packed lower triangles (OdeArgs::s_packed, EnergyArgs::ds_packed)
  bool grad_in_bwd = false;     // ... the backward kernel can assemble the gradient (OdeArgs::grad_on): F-only evaluations skip the recursion
  bool grad_in_bwd_now = false; // ... and does, at this batch size
};

// What the device buffers hold right now (the plan says what a sweep WILL produce).  Written through the transitions below and nowhere
// else; the argument builders take their layout fields from it, everything else reads it behind `cached`.  (DESIGN.md s.4.0 has the table.)
struct Resident {
  bool cached = false;       // a fused sweep's state is cached
  enum class Moments { RowMajor, TimeMajor } moments = Moments::RowMajor;   // in d_m / d_S; in d_msT alone (fused lane pass: untransposed on demand)
  enum class SLayout { Whole, Packed } S = SLayout::Whole;                  // d_S: whole matrices; packed lower triangles (the s_packed of every argument struct)
  // d_dEs: whole matrices; the upper triangles alone (EnergyArgs::ds_upper); packed lower triangles (ds_packed; the constant jump is then d_jscp)
  enum class DesLayout { Whole, Upper, Packed } dEs = DesLayout::Whole;
  // d_lam / d_psi: nothing of this state (an F-only evaluation, or a backward kernel that assembled the gradient and kept Psi_t to itself:
  // vgpa_fetch materialises); lam_t and Psi_t; lam_t and Q''_t = A_t / sigma^2 - 2 Psi_t (OdeArgs::q_on, GradArgs::psi_is_q)
  enum class Bwd { None, Psi, Q } bwd = Bwd::None;
  bool terms = false;        // dEsde_dm / dEsde_dS / <f> / E_sde(t) belong to the cached moments (false behind a fused lane pass)
  void sweep_begins(const Plan& p) { *this = Resident{}; S = p.packed ? SLayout::Packed : SLayout::Whole; }   // the only copy of the plan
  void forward_wrote(Moments where) { moments = where; }
  void energy_wrote(DesLayout how) { dEs = how; terms = true; }
  void backward_stored(Bwd what) { bwd = what; }
  void sweep_cached() { cached = true; }
  void lane_pass_cached() { terms = false; cached = true; }     // (the pass keeps the per-grid-point terms to itself)
  void moments_untransposed() { moments = Moments::RowMajor; }  // vgpa_fetch's conversions in place ...
  void psi_recovered() { bwd = Bwd::Psi; }
  void des_mirrored() { dEs = DesLayout::Whole; }
  void taken_over() { *this = Resident{}; }   // an operator-level call: the caller's whole matrices and row-major moments, no cache
  void cache_dropped() { cached = false; }    // the inputs or the caller's x behind the cached state are gone
};
}  // namespace

struct vgpa_ctx {
  vgpa_config cfg{};
  int D = 0, Np = 0, B = 1, M = 0;
  size_t DD = 0, len_x = 0;
  bool single = false, full = false;
  Plan plan;                          // which kernels run and in which layouts (make_plan)
  int n_cu = 256; bool keep_pe = false, force_sym = false;   // make_plan's inputs read once, in vgpa_create: the CU count, VGPA_ODE_KERNEL=pe / =sym
  int forced_helpers = -1;                                   // ... and VGPA_SYM_HELPERS (-1: not set)
  Resident res;                       // what the device buffers hold right now
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;      // side stream of the D > 64 energy terms (lde_energy's look-ahead), created on first use
  std::string err;
  double theta[kMaxTheta] = {0, 0, 0, 0};
  // device buffers
  std::vector<void*> allocs;
  const double* xcur = nullptr;   // where the kernels read [A|b] from (d_x or the caller's device buffer)
  double *d_x = nullptr, *d_m = nullptr, *d_S = nullptr, *d_Ef = nullptr, *d_dEm = nullptr, *d_dEs = nullptr, *d_Am = nullptr;
  double *d_lam = nullptr, *d_psi = nullptr, *d_g = nullptr, *d_et = nullptr, *d_eobs = nullptr, *d_esde = nullptr;
  double *d_f = nullptr, *d_jm = nullptr, *d_Edf = nullptr, *d_jm_dense = nullptr, *d_js_dense = nullptr;
  double *d_m0 = nullptr, *d_S0 = nullptr, *d_Sigma = nullptr, *d_isig = nullptr, *d_isg = nullptr;
  double *d_obs_y = nullptr, *d_Q = nullptr, *d_K = nullptr, *d_rinv = nullptr, *d_jsc = nullptr;
  double *d_op_m0 = nullptr, *d_op_S0 = nullptr, *d_op_Sigma = nullptr;
  double* d_ld_ws = nullptr;      // workspace of the large-D drivers
  double* d_lde_ws = nullptr;     // workspace of the large-D energy / gradient kernels
  // time-chunked ("streamed") large-D sweep: Psi_t and dEsde_dS_t live only in chunk buffers of ld_chunk + 1 matrices
  bool stream_ld = false;
  int ld_chunk = 0;
  double *d_dEs_c = nullptr, *d_psi_c = nullptr;
  void* h_fs = nullptr;        // pinned host block [B doubles | B status words]: F and the status words come back in one round trip (vgpa_fetch_f)
  double* d_jscp = nullptr;    // the constant matrix jump as a packed lower triangle (Resident::DesLayout::Packed)
  double isg0 = 1.0;           // 1 / sigma^2 of a shared Sigma = sigma^2 I (Plan::isg_iso)
  std::vector<int32_t> h_obs_idx; // host copy of obs_idx [Np]
  bool obs_diag = false;          // diagonal R and H = I: Q, K are diagonal
  double* d_obs_part = nullptr;   // [B][M] per-observation energy terms (large-D observation kernel)
  double* d_hyp = nullptr;        // [B][Np][H] integrands of the hyper-parameter gradients (vgpa_energy_hyper only)
  double* d_hypT = nullptr;       // [B][H] their trapezoids
  double* d_tg = nullptr;         // [B][Np] integrand of dF/dtheta (vgpa_theta_gradient, Lorenz-96)
  double* d_thT = nullptr;        // [B][kMaxTheta] ... its trapezoids / the lane kernel's results
  std::vector<double> h_isig;     // host copy of Sigma^-1 [D][D]
  double* d_vec_scratch = nullptr; // [2B coefficients | B results | B*bps partials] of the vector algebra
  size_t vec_scratch_n = 0;
  // axpby coefficients travel through a pinned ring (the caller's arrays may be temporaries that die on return)
  static constexpr int kCoefSlots = 16;
  double* h_coef = nullptr;        // pinned [kCoefSlots][2B]
  hipEvent_t ev_coef[kCoefSlots] = {};
  unsigned coef_next = 0;
  std::vector<void*> user_allocs;  // vgpa_dev_alloc memory not yet returned through vgpa_dev_free
  int lde_nb = 1;
  double lde_budget = 1.0e9;      // bytes the batched large-D energy workspace may take
  int64_t* d_obs_t = nullptr;
  int32_t *d_obs_idx = nullptr, *d_status = nullptr;
  double obs_const = 0.0, sigma1 = 1.0;
  double* d_msT = nullptr;       // fused lane pass: the moments time-major, problem fastest (OdeArgs::msT), [Np][D(D+1)/2 + D][bpad]: packed lower triangle of S_t, then m_t
  double* d_jmT = nullptr;       // ... and its sparse vector jumps, [M][D][bpad]
  int bpad = 0;
  double* d_Sfull = nullptr;     // the unpacked copy of a packed d_S, made when vgpa_fetch (or a kernel that wants S_t whole) asks
  BatchInputs in;                // where each problem reads each batch input
  // the per-problem rows the setters upload, allocated on first use (the record points at them)
  double *d_pp_m0 = nullptr, *d_pp_S0 = nullptr, *d_pp_e0 = nullptr, *d_pp_obs_y = nullptr, *d_pp_theta = nullptr, *d_pp_Sigma = nullptr;
  double *d_pp_isig = nullptr, *d_pp_isg = nullptr, *d_pp_sig1 = nullptr, *d_pp_qs = nullptr;
  int64_t* d_pp_obs_t = nullptr; int32_t* d_pp_obs_idx = nullptr;
  double *d_jm_pt = nullptr, *d_js_pt = nullptr;   // dense jumps [B][Np][D], [B][Np][D][D]: per-problem times on the 16-lane kernels
  bool pt_dense_zeroed = false;  // ... which are zero off the observation rows of the current times (each sweep rewrites only those rows)
  std::vector<double> h_sigma, h_s0; // host copies of the shared Sigma and S0 [D][D] (h_s0 empty: vgpa_config gave none)
  // per-problem observation model (vgpa_set_problem_obs_model)
  double *d_pp_Q = nullptr, *d_pp_K = nullptr, *d_pp_rinv = nullptr, *d_pp_jsc = nullptr, *d_pp_jscp = nullptr, *d_pp_obsc = nullptr;
  int32_t* d_pp_nobs = nullptr;
  std::vector<double> h_R, h_H;       // host copies of the shared R and H [D][D] (H: the identity when vgpa_config gave none)
  std::vector<int64_t> h_obs_t;       // host copy of the shared observation times [M] ...
  std::vector<int64_t> h_pp_obs_t;    // ... and of the per-problem rows in force [B][M] (empty: the shared row), so that either setter validates against the other's state
  std::vector<int32_t> h_nobs;        // the per-problem counts in force [B] (empty: M each)
  bool obs_model_rows = false;        // a per-problem observation model is in force
  bool shared_obs_diag = false, jsc_rows_sym = true;   // obs_diag of vgpa_config's model; every per-problem constant jump symmetric
  SigmaForm sigma_form, rows_form;            // make_plan's inputs: the form of the shared Sigma, of the per-problem rows in force,
  bool inputs_sym = true, s0_rows_sym = true;  // ... the shared s0 and constant jump symmetric, the per-problem s0 rows symmetric
  // vgpa_sample_paths: the result, the noise factors R, the factors of S0 and the given starts; grown on demand, freed in vgpa_destroy
  double *d_sp_out = nullptr, *d_sp_R = nullptr, *d_sp_L0 = nullptr, *d_sp_x0 = nullptr;
  size_t sp_out_n = 0, sp_R_n = 0, sp_L0_n = 0, sp_x0_n = 0;
  double *d_sp_logw = nullptr, *d_sp_start = nullptr;      // vgpa_sample_paths_weighted: the two sums and x_0 of every path
  size_t sp_logw_n = 0, sp_start_n = 0;
  double* d_lag_start = nullptr;   // vgpa_lag_covariance: the starting matrices [B][n_anchor][D][D] and, behind them, the anchors (int32); the result goes through d_sp_out
  size_t lag_start_n = 0;
  // vgpa_particle_filter: the two particle buffers, log-weights, prefix sums, ancestors of a step (int32), the histories (ess, flags and
  // ancestors as int32, clouds), the prior's mean and factor; vgpa_particle_statistics: the two buffers of rows and their mean;
  // vgpa_particle_moments: the descendant weights, the lineage ESS, the workgroups' partial sums, the moments; vgpa_particle_paths: the
  // slot table (int32; the trajectories themselves go through d_sp_out); vgpa_particle_forecast: of these the particles, log-weights, prefix
  // sums, normalised weights (PF_WTAB), partial sums, moments and slot table; vgpa_particle_covariance: the buffers of the moments (the
  // partial sums and their sum packed, sample_cov_len(D) per kept index) and PF_COV: the mean and behind it the whole matrices;
  // vgpa_particle_backward_paths: the buffers of vgpa_particle_paths, the clouds and PF_HLW: the log-weights the resamplings replaced;
  // vgpa_particle_conditional: the buffers of vgpa_particle_paths, the clouds and PF_REF: the reference trajectories;
  // vgpa_particle_events: the buffers of vgpa_particle_statistics (the rows are the event records), PF_EVC: the levels, PF_EVS: the sides
  // (int32), PF_CDF: the first-passage distribution; vgpa_particle_marginals: the descendant weights and the lineage ESS of the moments,
  // PF_QTAB: the integer descendant weights (uint64), PF_QFIN: their final row of every problem [B][n], PF_MGL: the ladders, PF_MASS: the masses (uint64);
  // vgpa_particle_lag_covariance: the slot table and d_sp_out of vgpa_particle_paths with all n_paths trajectories, [B][n][n_keep][D], which
  // stay on the device (the stride is the lever on their size), the descendant weights and behind them the normalised final weights
  // (PF_WTAB), the lineage ESS, PF_LAGR: the anchors' rows of the kept axis (int32), PF_LAG: the mean and behind it the cross moments;
  // vgpa_path_cross_moments: d_sp_out (the given paths), PF_WTAB (the given weights), PF_LAGR and PF_LAG;
  // vgpa_particle_backward_moments: the buffers of vgpa_particle_moments (PF_WTAB: the smoothing weights), the clouds and PF_HLW, PF_SMX: the
  // successors of one cut [B][n][D], PF_SMR: every successor's (max, sum) [2][B][n], PF_SMP: the column workgroups' sums of W^2
  enum { PF_XA, PF_XB, PF_LW, PF_CUM, PF_ANC, PF_ESS, PF_FLAG, PF_HANC, PF_CLOUDS, PF_MU, PF_LT, PF_STA, PF_STB, PF_MEAN, PF_WTAB, PF_LESS, PF_PART,
         PF_MOM, PF_SLOTS, PF_COV, PF_HLW, PF_REF, PF_EVC, PF_EVS, PF_CDF, PF_QTAB, PF_QFIN, PF_MGL, PF_MASS, PF_LAGR, PF_LAG, PF_SMX, PF_SMR, PF_SMP, PF_COUNT };
  double* d_pf[PF_COUNT] = {};
  size_t pf_n[PF_COUNT] = {};
  int32_t pf_hlw_paths = 0;        // n_paths of the last particle call if it kept PF_HLW (vgpa_particle_replaced_logw reads it with PF_FLAG), else 0
  // profiling
  bool prof = false;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double prof_ms[4] = {0, 0, 0, 0};
  int64_t prof_n = 0;
  bool prof_pending = false;
};

namespace {

int fail(vgpa_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

#define HIP_TRY(c, expr)                                                                            \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail((c), VGPA_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
// a launcher's status: "<what> failed: <error>"
#define LAUNCH_TRY(c, what, expr)                                                                   \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail((c), VGPA_ERR_DEVICE, what " failed: %s", hipGetErrorString(e_)); \
  } while (0)

template <typename T>
int dev_alloc(vgpa_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(&q, count * sizeof(T));
  if (e != hipSuccess) return fail(c, VGPA_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
  c->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return VGPA_OK;
}

// buffers that only some entry points need are allocated on first use
template <typename T>
int ensure(vgpa_ctx* c, T** p, size_t count) { return *p ? VGPA_OK : dev_alloc(c, p, count); }

template <typename T>
int upload(vgpa_ctx* c, T* dst, const T* src, size_t count) {
  HIP_TRY(c, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return VGPA_OK;
}

// the setters' per-problem rows: B rows of `stride` elements into *buf (allocated on first use); the record's entry then points there
template <typename T>
int upload_rows(vgpa_ctx* c, T** buf, const T* src, size_t stride, Rows<T>* entry) {
  int rc = ensure(c, buf, (size_t)c->B * stride);
  if (rc == VGPA_OK && (rc = upload(c, *buf, src, (size_t)c->B * stride)) == VGPA_OK) *entry = {*buf, stride};
  return rc;
}

template <typename T>
int download(vgpa_ctx* c, T* dst, const T* src, size_t count) {
  HIP_TRY(c, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return VGPA_OK;
}

bool is_symmetric(const double* a, int n) {
  double mx = 0.0, df = 0.0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      mx = std::fmax(mx, std::fabs(a[i * n + j]));
      df = std::fmax(df, std::fabs(a[i * n + j] - a[j * n + i]));
    }
  return df <= 1e-14 * mx;
}

bool stack_symmetric(const double* a, size_t count, int n) {
  for (size_t t = 0; t < count; t++)
    if (!is_symmetric(a + t * n * n, n)) return false;
  return true;
}

// Sigma^-1 [D][D], its diagonal isg [D] and the form of one Sigma [D][D]; 1-D models: sigma1 = Sigma, Sigma^-1 = 1 / sigma1.
// VGPA_ERR_ARG: a 1-D sigma that is not positive; VGPA_ERR_NOT_PD: an n-D Sigma that is not positive definite.
int invert_sigma(int D, bool single, const double* sigma, double* isig, double* isg, double* sigma1, SigmaForm* f) {
  std::fill(isig, isig + (size_t)D * D, 0.0); *f = SigmaForm{};
  *sigma1 = single ? sigma[0] : 1.0;
  if (single && !(sigma[0] > 0.0)) return VGPA_ERR_ARG;
  if (single) { isig[0] = isg[0] = 1.0 / sigma[0]; return VGPA_OK; }
  for (int i = 0; i < D && f->diag; i++)
    for (int j = 0; j < D; j++)
      if (i != j && sigma[(size_t)i * D + j] != 0.0) { f->diag = false; break; }
  if (f->diag) {   // chol_inv of a diagonal matrix: C = diag(1/sqrt(s)), C^T C = diag(C_ii * C_ii)
    for (int i = 0; i < D; i++) {
      const double sii = sigma[(size_t)i * D + i];
      if (!(sii > 0.0)) return VGPA_ERR_NOT_PD;
      const double ci = 1.0 / std::sqrt(sii);
      isg[i] = isig[(size_t)i * D + i] = ci * ci;
    }
  } else {
    if (!host_spd_inverse(D, sigma, isig, nullptr)) return VGPA_ERR_NOT_PD;
    for (int i = 0; i < D; i++) isg[i] = isig[(size_t)i * D + i];
  }
  f->iso = f->diag;
  for (int i = 1; i < D; i++) f->iso = f->iso && isg[i] == isg[0];
  f->sym = is_symmetric(sigma, D);
  return VGPA_OK;
}

// The observation terms' constants from R = obs_noise and H = obs_h (null: the identity), into arrays that are zero on entry:
// Q = H R^-1 H^T, K = H^T R^-1 H^T, rinv = diag(R^-1), jsc = H^T R^-1 H / 2 (the constant matrix jump), obs_const = the Gaussian
// normalisation of the M observations; diag: diagonal R and H = I, so that Q and K are diagonal.  1-D models: the scalars r and h.
// VGPA_ERR_NOT_PD: R is not positive (definite).
int obs_constants(int D, int M, bool single, const double* obs_noise, const double* obs_h, double* Q, double* K, double* rinv, double* jsc,
                  double* obs_const, bool* diag) {
  *diag = false;
  if (single) {
    const double r = obs_noise[0];
    if (!(r > 0.0)) return VGPA_ERR_NOT_PD;
    const double h = obs_h ? obs_h[0] : 1.0;
    Q[0] = 1.0 / r; K[0] = h; rinv[0] = 1.0 / r; jsc[0] = 0.5 / r;
    *obs_const = 0.5 * M * (std::log(2.0 * M_PI) + std::log(r));
    return VGPA_OK;
  }
  const size_t DD = (size_t)D * D;
  double logdet = 0.0;
  // fast path: diagonal R and H = I (no O(D^3) host work at large D).  An explicitly passed identity counts as
  // "no operator" (the reference's Likelihood materialises np.eye(d) when the operator is None, likelihood.py:33-40).
  bool h_identity = true;
  if (obs_h)
    for (int i = 0; i < D && h_identity; i++)
      for (int j = 0; j < D; j++)
        if (obs_h[(size_t)i * D + j] != (i == j ? 1.0 : 0.0)) { h_identity = false; break; }
  bool r_diag = h_identity;
  for (int i = 0; i < D && r_diag; i++)
    for (int j = 0; j < D; j++)
      if (i != j && obs_noise[(size_t)i * D + j] != 0.0) { r_diag = false; break; }
  *diag = r_diag;
  if (r_diag) {
    for (int i = 0; i < D; i++) {
      const double rii = obs_noise[(size_t)i * D + i];
      if (!(rii > 0.0)) return VGPA_ERR_NOT_PD;
      const double ci = 1.0 / std::sqrt(rii);
      const double ri = ci * ci;
      Q[(size_t)i * D + i] = ri; K[(size_t)i * D + i] = ri; jsc[(size_t)i * D + i] = 0.5 * ri; rinv[i] = ri;
      logdet += std::log(std::sqrt(rii));
    }
    logdet *= 2.0;
  } else {
    std::vector<double> Rinv(DD, 0.0), H(DD, 0.0), T(DD);
    if (!host_spd_inverse(D, obs_noise, Rinv.data(), &logdet)) return VGPA_ERR_NOT_PD;
    if (obs_h && !h_identity) H.assign(obs_h, obs_h + DD); else for (int i = 0; i < D; i++) H[(size_t)i * D + i] = 1.0;
    host_matmul(D, H.data(), Rinv.data(), T.data(), false, false);      // H R^-1
    host_matmul(D, T.data(), H.data(), Q, false, true);                 // H R^-1 H^T
    host_matmul(D, H.data(), Rinv.data(), T.data(), true, false);       // H^T R^-1
    host_matmul(D, T.data(), H.data(), K, false, true);                 // H^T R^-1 H^T
    host_matmul(D, T.data(), H.data(), jsc, false, false);              // H^T R^-1 H
    for (size_t e = 0; e < DD; e++) jsc[e] *= 0.5;
    for (int i = 0; i < D; i++) rinv[i] = Rinv[(size_t)i * D + i];
  }
  *obs_const = M * (D * std::log(2.0 * M_PI) + logdet);
  return VGPA_OK;
}

// one row of observation times: false unless strictly increasing indices in [0, Np); idx [Np] -> observation counter n, or -1
bool index_obs_times(const int64_t* obs_t, int M, int Np, int32_t* idx) {
  std::fill(idx, idx + Np, -1);
  for (int n = 0; n < M; n++) {
    const int64_t tn = obs_t[n];
    if (tn < 0 || tn >= Np || (n > 0 && tn <= obs_t[n - 1])) return false;
    idx[tn] = n;
  }
  return true;
}

}  // namespace

// The variational parameters are consumed in the caller's x layout: problem p at xcur + p*len_x, A first, then b.
// xcur is either the context's own copy d_x (host entry points) or the caller's device buffer (zero copy).
static inline const double* ctx_A(vgpa_ctx* c) { return c->xcur; }
static inline const double* ctx_b(vgpa_ctx* c) { return c->xcur + (size_t)c->Np * c->DD; }

static int ingest_x(vgpa_ctx* c, const double* x, bool on_device) {
  if (on_device) { c->xcur = x; return VGPA_OK; }
  { int rc = ensure(c, &c->d_x, (size_t)c->B * c->len_x); if (rc) return rc; }
  HIP_TRY(c, hipMemcpyAsync(c->d_x, x, (size_t)c->B * c->len_x * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->xcur = c->d_x;
  return VGPA_OK;
}

// operator-level inputs arrive as separate [B][Np][D][D] / [B][Np][D] host arrays: pack them into the x layout
static int ingest_ab(vgpa_ctx* c, const double* lin_a, const double* off_b) {
  const size_t na = (size_t)c->Np * c->DD, nb = (size_t)c->Np * c->D;
  { int rc = ensure(c, &c->d_x, (size_t)c->B * c->len_x); if (rc) return rc; }
  c->xcur = c->d_x;
  if (lin_a) HIP_TRY(c, hipMemcpy2DAsync(c->d_x, c->len_x * sizeof(double), lin_a, na * sizeof(double), na * sizeof(double), c->B, hipMemcpyHostToDevice, c->stream));
  if (off_b) HIP_TRY(c, hipMemcpy2DAsync(c->d_x + na, c->len_x * sizeof(double), off_b, nb * sizeof(double), nb * sizeof(double), c->B, hipMemcpyHostToDevice, c->stream));
  return VGPA_OK;
}

// problem p's values on the host: its own rows once a setter has set them, else the shared ones
static const double* theta_of(const vgpa_ctx* c, int p) { return c->in.theta.rows ? c->in.h_theta.data() + (size_t)p * kMaxTheta : c->theta; }
static const double* isig_of(const vgpa_ctx* c, int p) { return c->in.isig.stride ? c->in.h_isig.data() + p * c->DD : c->h_isig.data(); }
static double sigma1_of(const vgpa_ctx* c, int p) { return c->in.sig1.rows ? c->in.h_sig1[p] : c->sigma1; }
static double e0_of(const vgpa_ctx* c, int p) { return c->in.e0.rows ? c->in.h_e0[p] : c->cfg.e0; }

static void prof_mark(vgpa_ctx* c, int i) {
  if (c->prof) (void)hipEventRecord(c->ev[i], c->stream);
}

static void prof_collect(vgpa_ctx* c) {
  if (!c->prof || !c->prof_pending) return;
  (void)hipEventSynchronize(c->ev[4]);
  for (int i = 0; i < 4; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess) c->prof_ms[i] += ms;
  }
  c->prof_n += c->B;
  c->prof_pending = false;
}

// a gradient is behind everything enqueued so far: close the profile's last phase
static int prof_end(vgpa_ctx* c, int rc) {
  if (rc == VGPA_OK && c->prof) { prof_mark(c, 4); c->prof_pending = true; }
  return rc;
}

// The stepper of one sweep direction; sym: the caller's matrices are symmetric (Plan::sym_inputs for the fused sweep, the symmetry of
// the arrays it brought for an operator-level call).
// D <= 4: one lane per problem (any inputs) -- always at D = 1, from 512 problems at D = 2..4 (below that a problem per
// workgroup has the shorter latency: Lorenz-63 RK4 Np = 1001 forward 1.2 ms vs 1.6 ms; at 65536 problems 108 ms vs
// 6 ms); D = 2..4 below that: 16 lanes per problem, operands exchanged by ds_bpermute (ode_wave.hip).
// VGPA_FLAG_FORCE_GENERIC keeps the workgroup-per-problem kernels.
static Stepper stepper(const vgpa_ctx* c, bool fwd, bool sym) {
  if (c->D > kMaxSmallD) return Stepper::LargeD;
  if (c->cfg.flags & VGPA_FLAG_FORCE_GENERIC) return Stepper::Generic;
  if (c->D <= kMaxLaneD) {
    // (the lane kernels address a wave's 64 problems with 32-bit byte offsets from a wave-uniform base)
    if ((c->D == 1 || c->B >= 512) && c->len_x < ((size_t)1 << 22)) return Stepper::Lane;
    if (c->D >= 2) return Stepper::Wave;
  }
  return sym && ode_mfma_supported(c->cfg.method, fwd, c->D) ? Stepper::Mfma : Stepper::Generic;
}

// ... from kFusedGradMinBatch problems on (VGPA_FUSED_GRAD in the environment: 1 always, 0 never).  The third wave set costs the recursion
// ~0.4-0.5 ms per launch round (its matrix-core and vector-ALU instructions share the SIMDs' issue port with the product waves), the
// separate assembly ~7 us per problem: below ~70 problems the backward kernel followed by k_grad_mfma_q is the shorter way.
constexpr int kFusedGradMinBatch = 64;
static char fused_grad_switch() { static const char v = [] { const char* e = getenv("VGPA_FUSED_GRAD"); return e ? e[0] : '\0'; }(); return v; }

// The one place that decides a context's kernels (Plan).  Reads cfg, D, B, len_x, full, n_cu, keep_pe, force_sym, forced_helpers and the forms
// of the inputs.
static void make_plan(vgpa_ctx* c) {
  Plan p;
  // the form of the shared Sigma or of the per-problem rows (isotropic: every row sigma_p^2 I with its own sigma_p); symmetric: every
  // s0 / Sigma and the constant jump (else both products of the slope literally)
  const SigmaForm& f = c->in.Sigma.stride ? c->rows_form : c->sigma_form;
  p.sigma_diag = f.diag; p.isg_iso = f.iso;
  p.sym_inputs = c->inputs_sym && c->s0_rows_sym && c->jsc_rows_sym && c->sigma_form.sym && f.sym;
  // D <= 44 has two families of matrix-core stepping kernels: the symmetric-unit ones (two problems per CU, 4 waves each) win
  // once there are more problems than CUs, the role-specialised ones (one problem per CU, 8 waves) below that and for one
  // problem.  (D = 41 .. 44: one symmetric-unit workgroup per CU only -- its LDS -- so the role-specialised kernels stay.)
  // 33 <= D <= 40 (round 3): the fragment-cover kernels win at every batch size -- a lone workgroup steps 4 % faster than the
  // role-specialised pair (4.45 / 4.93 against 4.65 / 4.97 ms per forward / backward sweep of one problem), and the Q'' stream and
  // the pipelined gradient assembly come with them; VGPA_ODE_KERNEL=pe in the environment keeps the role-specialised family there
  // (comparison runs, tests).
  // (D > 44 has no other matrix-core stepper: launch_ode_mfma always takes the symmetric-unit kernels there, so the context
  //  says so too and the energy kernel writes dEsde_dS as the upper triangle those kernels read)
  const int nb = (c->D + 3) / 4;
  p.sym_units = (c->cfg.flags & VGPA_FLAG_SYM_UNITS) != 0 || (c->B > c->n_cu && nb <= 10) || ((nb == 9 || nb == 10) && !c->keep_pe) ||
                (nb >= 12 && c->D <= kMaxSmallD);
  p.launch_sym_units = p.sym_units || c->force_sym;   // (VGPA_ODE_KERNEL=sym: that family at D <= 44 too, in the layouts sym_units itself implies below)
  // Helper waves beside the cover kernels' product waves: two roles up to one problem per CU (a workgroup has the CU to itself), none
  // beyond; VGPA_SYM_HELPERS=0 / 1 / 2 in the environment forces none / one role / two roles at every batch size (comparison runs, tests)
  if (p.launch_sym_units && (nb == 9 || nb == 10))
    p.helper_roles = c->forced_helpers < 0 ? (c->B <= c->n_cu ? 2 : 0) : c->forced_helpers == 0 ? 0 : c->forced_helpers == 2 ? 2 : 1;
  p.fwd = stepper(c, true, p.sym_inputs);
  p.bwd = stepper(c, false, p.sym_inputs);
  // the fused lane pass (ode_small.hip::k_sweep_lane): forward kernel -> observations -> ONE kernel for the E_sde terms, the backward
  // recursion, the gradient and F
  // (msT carries S_t as its lower triangle: a non-symmetric s0 / Sigma keeps the four-kernel path, which handles both halves literally)
  p.lane_pass = p.fwd == Stepper::Lane && c->full && sweep_lane_supported(c->cfg.model, c->D) && !(c->cfg.flags & VGPA_FLAG_MATERIALIZE) &&
                 (c->D == 1 || p.sym_inputs);
  // (a symmetric-unit backward kernel reads the upper triangle of dEsde_dS only; VGPA_FLAG_KEEP_PSI keeps whole matrices and Psi_t)
  p.bwd_upper = p.sym_units && p.bwd == Stepper::Mfma && !(c->cfg.flags & VGPA_FLAG_KEEP_PSI);
  // Q''_t instead of Psi_t on the fragment-cover kernels (33 <= D <= 40, RK2 / RK4) with Sigma = sigma^2 I and Lorenz-96: the gradient
  // assembly (k_grad_mfma_q) then does not read A_t
  p.store_q = p.bwd_upper && p.sigma_diag && p.isg_iso && c->cfg.model == VGPA_MODEL_L96 && sym_stores_q(c->cfg.method, c->D);
  // S_t as its packed lower triangle between the kernels of a fused sweep: exactly where the gradient assembly will be k_grad_mfma_q
  // and the energy terms come from k_energy_l96_r; dEsde_dS between that kernel and the backward cover kernel likewise
  p.packed = p.store_q && p.fwd == Stepper::Mfma;
  // the backward kernel assembles the gradient itself: wherever S_t is packed and the stepper's kernel can.  F-only evaluations of
  // such a context skip the backward recursion altogether (F does not depend on it); gradient(x, eval_fun=False) runs it.
  p.grad_in_bwd = p.packed && sym_fuses_grad(c->cfg.method, c->D) && fused_grad_switch() != '0';
  p.grad_in_bwd_now = p.grad_in_bwd && (fused_grad_switch() == '1' || c->B >= kFusedGradMinBatch);
  c->plan = p;
}

// the small-D steppers share OdeArgs (the large-D drivers take their arrays one by one, each with its stride: run_fwd / run_bwd call them)
static hipError_t launch_stepper(const vgpa_ctx* c, Stepper k, bool fwd, const OdeArgs& a) {
  const int method = c->cfg.method;
  hipStream_t st = c->stream;
  switch (k) {
    case Stepper::Lane: return launch_ode_small(method, fwd, a, st);
    case Stepper::Wave: return launch_ode_wave(method, fwd, a, st);
    case Stepper::Mfma: return launch_ode_mfma(method, fwd, a, c->plan.helper_roles, st);
    case Stepper::Generic: return launch_ode_generic(method, fwd, a, st);
    case Stepper::LargeD: break;
  }
  return hipErrorInvalidValue;
}

static int ensure_ld_ws(vgpa_ctx* c) {
  if (c->d_ld_ws) return VGPA_OK;
  return dev_alloc(c, &c->d_ld_ws, (size_t)c->B * ld::ld_workspace_doubles(c->D));
}

// One call of the D > 64 drivers (ld::LdCall): the whole batch in grid.z of the per-stage kernels, every array handed over with its
// per-problem stride.  literal: non-symmetric inputs, both products of the slope formed literally (ode_solver.py:60,94).
static ld::LdCall ld_call(vgpa_ctx* c, bool literal) {
  return {c->cfg.method, c->cfg.dt, c->D, c->B, literal, (c->cfg.flags & VGPA_FLAG_LIBRARY_GEMM) != 0, c->d_ld_ws, c->stream};
}

// what every stepping kernel's OdeArgs starts with: the sizes, x, the moment histories and the matrix-core family
static OdeArgs ode_args(vgpa_ctx* c) {
  OdeArgs a{};
  a.D = c->D; a.Np = c->Np; a.batch = c->B; a.dt = c->cfg.dt;
  a.sym_units = c->plan.launch_sym_units ? 1 : 0;
  a.strideA = a.strideB = c->len_x;
  a.A = ctx_A(c); a.b = ctx_b(c); a.m = c->d_m; a.S = c->d_S;
  return a;
}

// the forward sweep's OdeArgs: ... with the initial moments and the forcing term
static OdeArgs fwd_args(vgpa_ctx* c, Rows<double> m0, Rows<double> S0, Rows<double> Sigma) {
  OdeArgs a = ode_args(c);
  a.m0 = m0.rows; a.m0_stride = m0.stride; a.S0 = S0.rows; a.S0_stride = S0.stride; a.Sigma = Sigma.rows; a.Sigma_stride = Sigma.stride;
  return a;
}

static void copy_theta(const vgpa_ctx* c, double* theta) {
  for (int i = 0; i < kMaxTheta; i++) theta[i] = c->theta[i];
}

// the sparse observation jumps of the backward recursion (dEsde_dS is never packed behind the lane pass: js_const = d_jsc there)
static void sparse_jumps(vgpa_ctx* c, OdeArgs& a) {
  a.obs_idx = c->in.obs_idx.rows; a.obs_idx_stride = (int)c->in.obs_idx.stride;
  a.jm_sparse = c->d_jm; a.js_const = c->res.dEs == Resident::DesLayout::Packed ? c->in.jscp.rows : c->in.jsc.rows; a.n_obs = c->M;
  a.js_const_stride = c->in.jsc.stride;      // (the packed copy's rows are D*D apart too)
}

// sym: Plan::sym_inputs for the fused sweep (the stepper is then Plan::fwd), the symmetry of the caller's arrays for vgpa_solve_fwd
static int run_fwd(vgpa_ctx* c, Rows<double> m0, Rows<double> S0, Rows<double> Sigma, bool sym) {
  c->res.forward_wrote(Resident::Moments::RowMajor);   // (every path below writes the [B][Np] arrays m / S)
  const Stepper k = stepper(c, true, sym);
  if (k == Stepper::LargeD) {
    int rc = ensure_ld_ws(c);
    if (rc) return rc;
    const size_t NpD = (size_t)c->Np * c->D, NpDD = (size_t)c->Np * c->DD;
    LAUNCH_TRY(c, "large-D forward sweep", ld::ld_solve_fwd(ld_call(c, !sym), c->Np, {ctx_A(c), c->len_x}, {ctx_b(c), c->len_x}, m0, S0, Sigma,
                                                            {c->d_m, NpD}, {c->d_S, NpDD}));
    return VGPA_OK;
  }
  OdeArgs a = fwd_args(c, m0, S0, Sigma);
  a.s_packed = c->res.S == Resident::SLayout::Packed ? 1 : 0;
  LAUNCH_TRY(c, "forward sweep launch", launch_stepper(c, k, true, a));
  return VGPA_OK;
}

static ObsArgs obs_args(vgpa_ctx* c);
// sym: as in run_fwd (dense_jumps: vgpa_solve_bwd's call, with the caller's arrays).  g_fused: the backward kernel assembles the
// gradient into it (Plan::grad_in_bwd contexts; Psi_t is then not stored)
static int run_bwd(vgpa_ctx* c, bool dense_jumps, bool sym, double* g_fused = nullptr) {
  int rc;
  if (g_fused && (dense_jumps || !c->plan.grad_in_bwd || c->res.S != Resident::SLayout::Packed)) return fail(c, VGPA_ERR_STATE, "fused gradient assembly asked of a context without it");
  if ((rc = ensure(c, &c->d_psi, (size_t)c->B * c->Np * c->DD))) return rc;
  if ((rc = ensure(c, &c->d_dEs, (size_t)c->B * c->Np * c->DD))) return rc;
  const Stepper k = stepper(c, false, sym);
  if (k == Stepper::LargeD) {
    if ((rc = ensure_ld_ws(c))) return rc;
    c->res.backward_stored(Resident::Bwd::Psi);
    const size_t NpD = (size_t)c->Np * c->D, NpDD = (size_t)c->Np * c->DD;
    // operator-level calls bring dense jump arrays; the fused sweep uses the sparse ones (obs index on the host, one constant matrix)
    const ld::LdJumps jumps = dense_jumps ? ld::LdJumps::dense({c->d_jm_dense, NpD}, {c->d_js_dense, NpDD})
                                          : ld::LdJumps::sparse({c->d_jm, (size_t)c->M * c->D}, {c->d_jsc, 0}, c->h_obs_idx.data());
    LAUNCH_TRY(c, "large-D backward sweep", ld::ld_solve_bwd(ld_call(c, !sym), c->Np, {ctx_A(c), c->len_x}, {c->d_dEm, NpD}, {c->d_dEs, NpDD}, jumps,
                                                             {c->d_lam, NpD}, {c->d_psi, NpDD}));
    return VGPA_OK;
  }
  OdeArgs a = ode_args(c);   // (b, m, S: read only with grad_on)
  a.dEm = c->d_dEm; a.dEs = c->d_dEs; a.lam = c->d_lam; a.psi = c->d_psi;
  if (dense_jumps) { a.jm_dense = c->d_jm_dense; a.js_dense = c->d_js_dense; }
  else if (c->in.obs_idx.stride && k == Stepper::Wave) {
    // per-problem times on the 16-lane kernels (four problems per wave, whose jump index is wave-uniform): dense jump arrays
    // (B Np (D + D^2) doubles, zeroed once per set of times; a sweep rewrites the B M (D + D^2) entries of the observation rows)
    if ((rc = ensure(c, &c->d_jm_pt, (size_t)c->B * c->Np * c->D))) return rc;
    if ((rc = ensure(c, &c->d_js_pt, (size_t)c->B * c->Np * c->DD))) return rc;
    if (!c->pt_dense_zeroed) {
      HIP_TRY(c, hipMemsetAsync(c->d_jm_pt, 0, sizeof(double) * c->B * c->Np * c->D, c->stream));
      HIP_TRY(c, hipMemsetAsync(c->d_js_pt, 0, sizeof(double) * c->B * c->Np * c->DD, c->stream));
      c->pt_dense_zeroed = true;
    }
    LAUNCH_TRY(c, "obs dense launch", launch_obs_dense(obs_args(c), c->in.jsc.rows, c->d_jm_pt, c->d_js_pt, c->stream));
    a.jm_dense = c->d_jm_pt; a.js_dense = c->d_js_pt;
  } else {
    sparse_jumps(c, a);
  }
  a.ds_packed = c->res.dEs == Resident::DesLayout::Packed ? 1 : 0;
  // (the fused sweep's call: the stepper is Plan::bwd then.  An operator-level call wants Psi_t itself)
  const bool q = !dense_jumps && c->plan.store_q;
  a.q_on = q ? 1 : 0;
  a.q_scale = c->isg0;
  a.q_scale_v = c->in.qs.rows;               // (read only by the Q'' kernels: every row isotropic then)
  if (g_fused) {                           // the gradient assembly on the kernel's helper waves (k_ode_sym, GF)
    if (!q) return fail(c, VGPA_ERR_STATE, "fused gradient assembly: the backward kernel is not the Q'' one");
    a.grad_on = 1; a.g = g_fused; a.s_packed = 1;      // (S_t is packed: checked on entry)
    a.Ef = c->d_Ef; a.Am = c->d_Am;
  }
  c->res.backward_stored(g_fused ? Resident::Bwd::None : q ? Resident::Bwd::Q : Resident::Bwd::Psi);   // (g_fused: nothing is stored in d_psi)
  LAUNCH_TRY(c, "backward sweep launch", launch_stepper(c, k, false, a));
  return VGPA_OK;
}

static EnergyArgs energy_args(vgpa_ctx* c, double* edf, bool hyper = false) {
  EnergyArgs a{};         // (ds_upper / ds_packed = 0: run_energy, the one caller that has dEsde_dS written, sets them)
  a.s_packed = c->res.S == Resident::SLayout::Packed ? 1 : 0;
  a.model = c->cfg.model; a.D = c->D; a.Np = c->Np; a.batch = c->B; a.dt = c->cfg.dt;
  copy_theta(c, a.theta);
  a.sigma1 = c->sigma1; a.isg = c->in.isg.rows; a.isg_stride = c->in.isg.stride;
  a.theta_v = c->in.theta.rows; a.sigma1_v = c->in.sig1.rows;
  a.strideA = a.strideB = c->len_x;
  a.A = ctx_A(c); a.b = ctx_b(c); a.m = c->d_m; a.S = c->d_S;
  a.e_t = c->d_et; a.Ef = c->d_Ef; a.Edf = edf; a.dEm = c->d_dEm; a.dEs = c->d_dEs; a.status = c->d_status;
  a.Am = (c->cfg.model == VGPA_MODEL_L96) ? c->d_Am : nullptr;
  a.hyp = hyper ? c->d_hyp : nullptr;
  return a;
}

static int ensure_lde_ws(vgpa_ctx* c) {
  if (!c->stream2 && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) {
    c->stream2 = nullptr;               // (lde_energy then runs on the one stream)
    (void)hipGetLastError();
  }
  if (c->d_lde_ws) return VGPA_OK;
  c->lde_nb = ld::lde_batch(c->D, c->lde_budget);
  if (c->lde_nb > c->Np) c->lde_nb = c->Np;
  return dev_alloc(c, &c->d_lde_ws, ld::lde_workspace_doubles(c->D, c->lde_nb));
}

// The layout the energy kernels write dEsde_dS in when asked for `want`: the L96 kernels of 5 <= D <= 64 honour the upper triangle, and
// k_energy_l96_r, the kernel that reads packed S_t, the packed lower one; everything else writes whole matrices.
static Resident::DesLayout des_layout(const vgpa_ctx* c, Resident::DesLayout want) {
  using L = Resident::DesLayout;
  if (want == L::Whole || c->cfg.model != VGPA_MODEL_L96 || c->D < 5 || c->D > kMaxSmallD) return L::Whole;
  return want == L::Packed && c->res.S == Resident::SLayout::Packed ? L::Packed : L::Upper;
}
// want: the plan's layout for a fused sweep (enqueue_free_energy), whole matrices for everything else; hyper: the integrands of d_hyp as well
static int run_energy(vgpa_ctx* c, double* edf, Resident::DesLayout want = Resident::DesLayout::Whole, bool hyper = false) {
  c->res.energy_wrote(des_layout(c, want));
  { int rc = ensure(c, &c->d_dEs, (size_t)c->B * c->Np * c->DD); if (rc) return rc; }
  if (c->D > kMaxSmallD) {
    if (c->cfg.model != VGPA_MODEL_L96) return fail(c, VGPA_ERR_UNSUPPORTED, "large-D energy terms exist for Lorenz-96 only");
    int rc = ensure_lde_ws(c);
    if (rc) return rc;
    // the energy terms are batched over grid points already: problem by problem
    const size_t NpD = (size_t)c->Np * c->D, NpDD = (size_t)c->Np * c->DD;
    for (int p = 0; p < c->B; p++) {
      LAUNCH_TRY(c, "large-D energy", ld::lde_energy(c->D, c->Np, theta_of(c, p)[0], c->in.isg.of(p), ctx_A(c) + p * c->len_x,
                                                     ctx_b(c) + p * c->len_x, c->d_m + p * NpD, c->d_S + p * NpDD, c->d_et + (size_t)p * c->Np,
                                                     c->d_Ef + p * NpD, edf ? edf + p * NpDD : nullptr, c->d_dEm + p * NpD, c->d_dEs + p * NpDD,
                                                     c->d_status + p, c->d_lde_ws, c->lde_nb, c->stream,
                                                     hyper ? c->d_hyp + (size_t)p * c->Np * 2 * c->D : nullptr, c->stream2));
    }
    return VGPA_OK;
  }
  EnergyArgs a = energy_args(c, edf, hyper);
  a.ds_upper = c->res.dEs == Resident::DesLayout::Upper ? 1 : 0;
  a.ds_packed = c->res.dEs == Resident::DesLayout::Packed ? 1 : 0;
  LAUNCH_TRY(c, "energy launch", launch_energy(a, c->stream));
  return VGPA_OK;
}

static ObsArgs obs_args(vgpa_ctx* c) {
  ObsArgs a{};
  a.D = c->D; a.Np = c->Np; a.batch = c->B; a.n_obs = c->M; a.single = c->single ? 1 : 0;
  a.obs_t = c->in.obs_t.rows; a.obs_t_stride = c->in.obs_t.stride; a.obs_y = c->in.obs_y.rows; a.obs_y_stride = c->in.obs_y.stride;
  a.Q = c->in.Q.rows; a.Q_stride = c->in.Q.stride; a.K = c->in.K.rows; a.K_stride = c->in.K.stride;
  a.rinv_diag = c->in.rinv.rows; a.rinv_stride = c->in.rinv.stride; a.js_const_stride = c->in.jsc.stride;
  a.obs_const_v = c->in.obs_const.rows; a.n_obs_v = c->in.n_obs.rows;
  a.obs_const = c->obs_const; a.m = c->d_m; a.S = c->d_S; a.jm_sparse = c->d_jm; a.eobs = c->d_eobs;
  a.diag = c->obs_diag ? 1 : 0; a.part = c->d_obs_part;
  a.s_packed = c->res.S == Resident::SLayout::Packed ? 1 : 0;
  return a;
}

static int run_reduce(vgpa_ctx* c) {
  ReduceArgs r{};
  r.Np = c->Np; r.batch = c->B; r.dt = c->cfg.dt; r.e0 = c->cfg.e0; r.e0v = c->in.e0.rows;
  r.pre = c->single ? 0.5 : 1.0; r.div = c->single ? c->sigma1 : 1.0; r.div_v = c->single ? c->in.sig1.rows : nullptr;
  r.e_t = c->d_et; r.eobs = c->d_eobs; r.esde = c->d_esde; r.f = c->d_f;
  LAUNCH_TRY(c, "reduce launch", launch_reduce(r, c->stream));
  return VGPA_OK;
}

static int unpack_S(vgpa_ctx* c, const double** full);

static int run_grad(vgpa_ctx* c, double* g_dev) {
  if (c->D > kMaxSmallD) {
    int rc = ensure_lde_ws(c);
    if (rc) return rc;
    const size_t NpD = (size_t)c->Np * c->D, NpDD = (size_t)c->Np * c->DD;
    for (int p = 0; p < c->B; p++) {
      double* gp = g_dev + p * c->len_x;
      LAUNCH_TRY(c, "large-D gradient", ld::lde_grad(c->D, c->Np, c->cfg.dt, c->in.isg.of(p), ctx_A(c) + p * c->len_x, ctx_b(c) + p * c->len_x, c->d_m + p * NpD,
                                                     c->d_S + p * NpDD, c->d_lam + p * NpD, c->d_psi + p * NpDD, c->d_Ef + p * NpD, gp, gp + NpDD, c->d_lde_ws,
                                                     c->lde_nb, c->stream, c->plan.sigma_diag ? nullptr : c->in.isig.of(p)));
    }
    return VGPA_OK;
  }
  GradArgs a{};
  a.model = c->cfg.model; a.D = c->D; a.Np = c->Np; a.batch = c->B; a.sigma_diag = c->plan.sigma_diag ? 1 : 0;
  a.dt = c->cfg.dt;
  copy_theta(c, a.theta);
  a.strideA = a.strideB = c->len_x;
  a.A = ctx_A(c); a.b = ctx_b(c); a.m = c->d_m; a.S = c->d_S; a.lam = c->d_lam; a.psi = c->d_psi;
  a.isig = c->in.isig.rows; a.isig_stride = c->in.isig.stride; a.theta_v = c->in.theta.rows;
  a.Ef = c->d_Ef; a.Edf = nullptr; a.g = g_dev;
  const bool q = c->res.bwd == Resident::Bwd::Q, packed = c->res.S == Resident::SLayout::Packed;
  a.psi_is_q = q ? 1 : 0;
  a.s_packed = (packed && q) ? 1 : 0;
  if (packed && !q) {        // (an assembly kernel that wants S_t whole: behind VGPA_FETCH_PSIT, which recovers Psi_t in place)
    const double* full = nullptr;
    int rc = unpack_S(c, &full);
    if (rc) return rc;
    a.S = full;
  }
  a.Am = c->d_Am;                                  // written by the L96 energy kernel of the same sweep (else null)
  a.scalar_product = (c->cfg.flags & VGPA_FLAG_FORCE_GENERIC) ? 1 : 0;
  LAUNCH_TRY(c, "gradient launch", launch_grad(a, c->stream));
  return VGPA_OK;
}

// ---- time-chunked large-D sweep (BASELINE config 4: Np x D x D arrays do not all fit in HBM) -------------------------
// Keeps x, S_t and the gradient (caller's buffer); Psi_t and dEsde_dS_t exist only for a chunk of ld_chunk + 1 grid
// points.  From the last grid point backwards, per chunk [t0, t1]:  energy terms of the chunk -> backward steps
// t1 .. t0+1 (Psi in the chunk buffer, lam_t in full) -> gradient of the grid points whose Psi_t is now final.
// g_dev == nullptr: energy integrand only (what F needs).  Same kernels, same per-grid-point arithmetic as the
// resident path, so the results are identical.
static int stream_pass(vgpa_ctx* c, double* g_dev) {
  const int D = c->D, Np = c->Np, C = c->ld_chunk;
  const size_t DD = c->DD;
  int rc;
  if ((rc = ensure_lde_ws(c))) return rc;
  if ((rc = ensure_ld_ws(c))) return rc;
  if ((rc = ensure(c, &c->d_dEs_c, (size_t)(C + 1) * DD))) return rc;
  if (g_dev && (rc = ensure(c, &c->d_psi_c, (size_t)(C + 1) * DD))) return rc;
  const double *A = ctx_A(c), *b = ctx_b(c);
  hipStream_t st = c->stream;
  const ld::LdCall step = ld_call(c, false);      // (one problem: every operand of ld_bwd_step below has stride 0)
  int t1 = Np - 1;
  if (g_dev) HIP_TRY(c, hipMemsetAsync(c->d_lam + (size_t)t1 * D, 0, sizeof(double) * D, st));
  bool first = true;
  while (true) {
    const int t0 = (t1 - C > 0) ? (t1 - C) : 0;
    const int n = t1 - t0 + 1;
    LAUNCH_TRY(c, "large-D energy", ld::lde_energy(D, n, c->theta[0], c->d_isg, A + (size_t)t0 * DD, b + (size_t)t0 * D, c->d_m + (size_t)t0 * D,
                                                   c->d_S + (size_t)t0 * DD, c->d_et + t0, c->d_Ef + (size_t)t0 * D, nullptr,
                                                   c->d_dEm + (size_t)t0 * D, c->d_dEs_c, c->d_status, c->d_lde_ws, c->lde_nb, st, nullptr, c->stream2));
    if (g_dev) {
      // Psi_{t1} sits in slot n-1: zero at the very end of the grid, else carried over from slot 0 of the previous chunk
      if (first) HIP_TRY(c, hipMemsetAsync(c->d_psi_c + (size_t)(n - 1) * DD, 0, sizeof(double) * DD, st));
      for (int t = t1; t > t0; t--) {
        const int k = t - t0;
        const int nobs = c->h_obs_idx[t - 1];
        LAUNCH_TRY(c, "large-D backward step", ld::ld_bwd_step(step, {A + (size_t)t * DD}, {A + (size_t)(t - 1) * DD},
                                                               {c->d_dEs_c + (size_t)k * DD}, {c->d_dEs_c + (size_t)(k - 1) * DD}, {c->d_dEm + (size_t)t * D},
                                                               {c->d_dEm + (size_t)(t - 1) * D}, {c->d_psi_c + (size_t)k * DD}, {c->d_lam + (size_t)t * D},
                                                               {c->d_psi_c + (size_t)(k - 1) * DD}, {c->d_lam + (size_t)(t - 1) * D},
                                                               {nobs >= 0 ? c->d_jsc : nullptr}, {nobs >= 0 ? c->d_jm + (size_t)nobs * D : nullptr}));
      }
      // gradient of (t0, t1] -- and of t0 itself once the grid start is reached
      const int g0 = (t0 == 0) ? 0 : t0 + 1;
      const int gn = t1 - g0 + 1;
      double* gA = g_dev + (size_t)g0 * DD;
      double* gB = g_dev + (size_t)Np * DD + (size_t)g0 * D;
      LAUNCH_TRY(c, "large-D gradient", ld::lde_grad(D, gn, c->cfg.dt, c->d_isg, A + (size_t)g0 * DD, b + (size_t)g0 * D, c->d_m + (size_t)g0 * D,
                                                     c->d_S + (size_t)g0 * DD, c->d_lam + (size_t)g0 * D, c->d_psi_c + (size_t)(g0 - t0) * DD,
                                                     c->d_Ef + (size_t)g0 * D, gA, gB, c->d_lde_ws, c->lde_nb, st, c->plan.sigma_diag ? nullptr : c->d_isig));
    }
    if (t0 == 0) break;
    if (g_dev) {   // Psi_{t0} becomes Psi_{t1} of the next chunk: slot 0 -> slot (t0 - t0_next)
      const int t0n = (t0 - C > 0) ? (t0 - C) : 0;
      HIP_TRY(c, hipMemcpyAsync(c->d_psi_c + (size_t)(t0 - t0n) * DD, c->d_psi_c, sizeof(double) * DD, hipMemcpyDeviceToDevice, st));
    }
    t1 = t0;
    first = false;
  }
  c->res.energy_wrote(Resident::DesLayout::Whole);   // (the per-grid-point vectors; dEsde_dS_t itself chunk by chunk only: vgpa_fetch refuses it)
  return VGPA_OK;
}

// fwd -> E_obs -> chunked [E_sde terms -> bwd -> gradient] -> F, for the streamed large-D context
static int enqueue_stream_sweep(vgpa_ctx* c, double* g_dev) {
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  int rc;
  prof_collect(c);
  HIP_TRY(c, hipMemsetAsync(c->d_status, 0, sizeof(int32_t) * c->B, c->stream));
  c->res.sweep_begins(c->plan);
  prof_mark(c, 0);
  if ((rc = run_fwd(c, c->in.m0, c->in.S0, c->in.Sigma, c->plan.sym_inputs))) return rc;
  prof_mark(c, 1);
  LAUNCH_TRY(c, "obs launch", launch_obs(obs_args(c), c->stream));
  prof_mark(c, 2);
  if ((rc = stream_pass(c, g_dev))) return rc;
  prof_mark(c, 3);
  if ((rc = run_reduce(c))) return rc;
  c->res.sweep_cached();
  return g_dev ? prof_end(c, VGPA_OK) : VGPA_OK;
}

// DIAGNOSTIC (tools/power_per_kernel.sh): VGPA_DIAG_REPEAT="<fwd|energy|bwd|grad>:<n>" launches that phase of the fused sweep n times
// instead of once -- every phase is a pure function of its inputs, so the results do not change -- to hold one kernel on the chip long
// enough for clock / power samples.  Read once; absent = 1.
static int diag_repeat(const char* phase) {
  static const std::string spec = [] { const char* e = getenv("VGPA_DIAG_REPEAT"); return std::string(e ? e : ""); }();
  const size_t colon = spec.find(':');
  if (colon == std::string::npos || spec.compare(0, colon, phase) != 0) return 1;
  const int n = atoi(spec.c_str() + colon + 1);
  return n > 1 ? n : 1;
}

// the fused lane pass over the cached (m, S): F (want_grad = false) or F and the gradient
static int run_lane_pass(vgpa_ctx* c, double* g_dev) {
  LaneSweepArgs q{};
  OdeArgs& a = q.o;
  a = ode_args(c);
  a.msT = c->d_msT; a.bpad = c->bpad; a.jmT = c->d_jmT;
  sparse_jumps(c, a);
  q.model = c->cfg.model; q.want_grad = g_dev ? 1 : 0;
  copy_theta(c, q.theta);
  q.sigma1 = c->sigma1;
  for (int i = 0; i < c->D; i++) q.isg[i] = c->h_isig[(size_t)i * c->D + i];
  for (size_t e = 0; e < c->DD; e++) q.isig[e] = c->h_isig[e];
  q.e0 = c->cfg.e0; q.e0v = c->in.e0.rows; q.pre = c->single ? 0.5 : 1.0; q.div = c->single ? c->sigma1 : 1.0;
  q.theta_v = c->in.theta.rows; q.sigma1_v = c->in.sig1.rows; q.isig_v = c->in.isig.stride ? c->in.isig.rows : nullptr;
  q.eobs = c->d_eobs; q.esde = c->d_esde; q.f = c->d_f; q.g = g_dev;
  LAUNCH_TRY(c, "fused lane pass launch", launch_sweep_lane(c->cfg.method, q, c->stream));
  return VGPA_OK;
}

// forward moments -> observation terms -> fused lane pass (F, and the gradient when g_dev is given)
static int enqueue_lane_sweep(vgpa_ctx* c, double* g_dev) {
  int rc;
  prof_collect(c);
  HIP_TRY(c, hipMemsetAsync(c->d_status, 0, sizeof(int32_t) * c->B, c->stream));
  c->res.sweep_begins(c->plan);
  prof_mark(c, 0);
  if (!c->d_msT) {
    c->bpad = 64 * ((c->B + 63) / 64);
    if ((rc = dev_alloc(c, &c->d_msT, (size_t)c->Np * (c->D * (c->D + 1) / 2 + c->D) * c->bpad))) return rc;
    if ((rc = dev_alloc(c, &c->d_jmT, (size_t)(c->M > 0 ? c->M : 1) * c->D * c->bpad))) return rc;
  }
  {
    OdeArgs a = fwd_args(c, c->in.m0, c->in.S0, c->in.Sigma);
    a.msT = c->d_msT; a.bpad = c->bpad;
    LAUNCH_TRY(c, "forward lane kernel launch", launch_ode_small(c->cfg.method, true, a, c->stream));
  }
  c->res.forward_wrote(Resident::Moments::TimeMajor);
  prof_mark(c, 1);
  LAUNCH_TRY(c, "obs launch", launch_obs_lane(obs_args(c), c->d_msT, c->bpad, c->d_jmT, c->stream));
  prof_mark(c, 2);
  if ((rc = run_lane_pass(c, g_dev))) return rc;
  prof_mark(c, 3);
  c->res.lane_pass_cached();
  return g_dev ? prof_end(c, VGPA_OK) : VGPA_OK;
}

// what vgpa_fetch wants of the arrays the fused lane pass never wrote: the separate kernels over the cached (m, S)
static int materialize_moments(vgpa_ctx* c) {
  if (c->res.moments == Resident::Moments::RowMajor) return VGPA_OK;
  LAUNCH_TRY(c, "moment untranspose launch", launch_ms_untranspose(c->D, c->Np, c->B, c->bpad, c->d_msT, c->d_m, c->d_S, c->stream));
  c->res.moments_untransposed();
  return VGPA_OK;
}

static int materialize_derived(vgpa_ctx* c) {
  if (c->res.terms) return VGPA_OK;
  int rc;
  if ((rc = materialize_moments(c))) return rc;
  // the separate backward kernel reads the jumps in the [B][M][D] layout: the observation kernel over the [B][Np] moments
  LAUNCH_TRY(c, "obs launch", launch_obs(obs_args(c), c->stream));
  if ((rc = run_energy(c, nullptr))) return rc;
  return run_bwd(c, false, c->plan.sym_inputs);
}

// consumers that want S_t whole (vgpa_fetch, the operator-level kernels): the unpacked copy
static int unpack_S(vgpa_ctx* c, const double** full) {
  *full = c->d_S;
  if (c->res.S == Resident::SLayout::Whole) return VGPA_OK;
  const size_t BN = (size_t)c->B * c->Np;
  int rc;
  if ((rc = ensure(c, &c->d_Sfull, BN * c->DD))) return rc;
  LAUNCH_TRY(c, "unpack launch", launch_unpack_lower(BN, c->D, c->d_S, c->d_Sfull, c->stream));
  *full = c->d_Sfull;
  return VGPA_OK;
}

// fwd -> E_obs -> E_sde terms -> bwd -> F     (VarGP.free_energy, variational.py:141-200)
static int enqueue_free_energy(vgpa_ctx* c) {
  if (c->stream_ld) return enqueue_stream_sweep(c, nullptr);
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  if (c->plan.lane_pass) return enqueue_lane_sweep(c, nullptr);
  int rc;
  prof_collect(c);
  c->res.sweep_begins(c->plan);
  HIP_TRY(c, hipMemsetAsync(c->d_status, 0, sizeof(int32_t) * c->B, c->stream));
  prof_mark(c, 0);
  for (int r = diag_repeat("fwd"); r > 0; r--)
    if ((rc = run_fwd(c, c->in.m0, c->in.S0, c->in.Sigma, c->plan.sym_inputs))) return rc;
  prof_mark(c, 1);
  LAUNCH_TRY(c, "obs launch", launch_obs(obs_args(c), c->stream));
  using L = Resident::DesLayout;
  const L des = c->plan.packed ? L::Packed : c->plan.bwd_upper ? L::Upper : L::Whole;
  for (int r = diag_repeat("energy"); r > 0; r--)
    if ((rc = run_energy(c, nullptr, des))) return rc;
  prof_mark(c, 2);
  if (!c->plan.grad_in_bwd) {              // (else F needs no backward recursion; the gradient's comes with its assembly: finish_gradient)
    for (int r = diag_repeat("bwd"); r > 0; r--)
      if ((rc = run_bwd(c, false, c->plan.sym_inputs))) return rc;
    prof_mark(c, 3);
  }
  if ((rc = run_reduce(c))) return rc;
  c->res.sweep_cached();
  return VGPA_OK;
}

// a sweep's status words, on the host: bit 0 of problem p's says that its S_t lost positive definiteness
static int report_status(vgpa_ctx* c, const int32_t* st) {
  for (int p = 0; p < c->B; p++)
    if (st[p] & 1)
      return fail(c, VGPA_ERR_NOT_PD, "problem %d: marginal covariance S_t is not positive definite "
                  "(reference: LinAlgError from chol_inv, variational.py:380)", p);
  return VGPA_OK;
}

static int check_status(vgpa_ctx* c) {
  std::vector<int32_t> st(c->B);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->d_status, sizeof(int32_t) * c->B, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return report_status(c, st.data());
}

// =====================================================================================================
extern "C" {

int vgpa_abi_version(void) { return VGPA_ABI_VERSION; }

int vgpa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* vgpa_last_error(const vgpa_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void vgpa_destroy(vgpa_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (void* p : c->allocs) (void)hipFree(p);
  for (void* p : c->user_allocs) (void)hipFree(p);
  for (double* p : {c->d_sp_out, c->d_sp_R, c->d_sp_L0, c->d_sp_x0, c->d_sp_logw, c->d_sp_start, c->d_lag_start}) if (p) (void)hipFree(p);
  for (double* p : c->d_pf) if (p) (void)hipFree(p);
  if (c->h_coef) (void)hipHostFree(c->h_coef);
  if (c->h_fs) (void)hipHostFree(c->h_fs);
  for (auto& e : c->ev_coef) if (e) (void)hipEventDestroy(e);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int vgpa_create(vgpa_ctx** out, const vgpa_config* cfg) {
  if (!out || !cfg) return fail(nullptr, VGPA_ERR_ARG, "null argument");
  *out = nullptr;
  if (cfg->abi_version != VGPA_ABI_VERSION) return fail(nullptr, VGPA_ERR_ARG, "ABI version mismatch: %d != %d", cfg->abi_version, VGPA_ABI_VERSION);
  if (!(cfg->dt > 0.0)) return fail(nullptr, VGPA_ERR_ARG, "Discrete time step should be strictly positive -> %g.", cfg->dt);
  if (cfg->method < VGPA_ODE_EULER || cfg->method > VGPA_ODE_RK4) return fail(nullptr, VGPA_ERR_ARG, "Integration method is unknown -> %d.", cfg->method);
  if (cfg->model < VGPA_MODEL_NONE || cfg->model > VGPA_MODEL_L96) return fail(nullptr, VGPA_ERR_ARG, "Unknown stochastic model -> %d", cfg->model);
  if (cfg->dim_d < 1 || cfg->n_pts < 2 || cfg->batch < 1 || cfg->n_obs < 0) return fail(nullptr, VGPA_ERR_ARG, "bad sizes: D=%d Np=%d batch=%d M=%d", cfg->dim_d, cfg->n_pts, cfg->batch, cfg->n_obs);
  const bool single = (cfg->model == VGPA_MODEL_OU || cfg->model == VGPA_MODEL_DW) ||
                      (cfg->model == VGPA_MODEL_NONE && cfg->dim_d == 1);
  if (single && cfg->dim_d != 1) return fail(nullptr, VGPA_ERR_ARG, "1-D model with D=%d", cfg->dim_d);
  if (cfg->model == VGPA_MODEL_L63 && cfg->dim_d != 3) return fail(nullptr, VGPA_ERR_ARG, "Lorenz-63 needs D=3, got %d", cfg->dim_d);
  if (cfg->model == VGPA_MODEL_L96 && cfg->dim_d < 4) return fail(nullptr, VGPA_ERR_ARG, "Insufficient state vector dimensions: %d", cfg->dim_d);
  if (cfg->dim_d > kMaxSmallD && cfg->model != VGPA_MODEL_NONE && cfg->model != VGPA_MODEL_L96)
    return fail(nullptr, VGPA_ERR_UNSUPPORTED, "D=%d > %d is built for the ODE operators (model NONE) and for Lorenz-96 only",
                cfg->dim_d, kMaxSmallD);
  const int need_theta = (cfg->model == VGPA_MODEL_L63) ? 3 : (cfg->model == VGPA_MODEL_NONE ? 0 : 1);
  if (cfg->n_theta != need_theta || (need_theta > 0 && !cfg->theta)) return fail(nullptr, VGPA_ERR_ARG, "model needs %d drift parameter(s)", need_theta);
  if (!cfg->sigma) return fail(nullptr, VGPA_ERR_ARG, "sigma is required");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, VGPA_ERR_DEVICE, "no HIP device is visible (libvgpa_hip has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, VGPA_ERR_DEVICE, "device %d out of range (%d visible)", cfg->device, ndev);

  vgpa_ctx* c = new vgpa_ctx();
  c->cfg = *cfg;
  c->D = cfg->dim_d; c->Np = cfg->n_pts; c->B = cfg->batch; c->M = cfg->n_obs;
  c->DD = (size_t)c->D * c->D;
  c->len_x = (size_t)c->Np * c->DD + (size_t)c->Np * c->D;
  c->single = single;
  for (int i = 0; i < cfg->n_theta; i++) c->theta[i] = cfg->theta[i];
  c->full = cfg->model != VGPA_MODEL_NONE && cfg->m0 && cfg->s0 && (cfg->n_obs == 0 || (cfg->obs_t && cfg->obs_y && cfg->obs_noise));
  const int D = c->D;
  const size_t DD = c->DD;
  int rc = VGPA_OK;
  // every error exit: the message, then everything allocated so far goes back
#define FAIL(code, ...) do { const int code_ = fail(nullptr, (code), __VA_ARGS__); vgpa_destroy(c); return code_; } while (0)
#define TRY(expr) do { if ((rc = (expr)) != VGPA_OK) FAIL(rc, "%s", c->err.c_str()); } while (0)
#define HTRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) FAIL(VGPA_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  HTRY(hipSetDevice(cfg->device));
  HTRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || c->n_cu <= 0) c->n_cu = 256;
  { const char* fam = getenv("VGPA_ODE_KERNEL"); c->keep_pe = fam && !strcmp(fam, "pe"); c->force_sym = fam && !strcmp(fam, "sym"); }
  { const char* hlp = getenv("VGPA_SYM_HELPERS"); c->forced_helpers = hlp ? atoi(hlp) : -1; }
  // (phase events: no system-scope fence behind them -- nothing on the host reads device memory at a phase boundary; with the default
  //  flags five events cost a batched Ornstein-Uhlenbeck step 0.4 of its 1.4 ms)
  for (auto& e : c->ev) HTRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));

  // ---- host-side constants -------------------------------------------------------------------
  std::vector<double> sigma(cfg->sigma, cfg->sigma + DD), isig(DD, 0.0), isg(D, 1.0);
  if (cfg->model == VGPA_MODEL_NONE && !single) {   // ODE-only: Sigma^-1 = I is not used
    for (int i = 0; i < D; i++) isig[(size_t)i * D + i] = 1.0;
    c->sigma_form.sym = is_symmetric(sigma.data(), D);
  } else {
    rc = invert_sigma(D, single, sigma.data(), isig.data(), isg.data(), &c->sigma1, &c->sigma_form);
    if (rc == VGPA_ERR_ARG) FAIL(rc, "The diffusion noise value: %g, should be strictly positive.", sigma[0]);
    if (rc) FAIL(rc, "Noise matrix is not positive definite.");
  }
  c->inputs_sym = !cfg->s0 || is_symmetric(cfg->s0, D);

  const size_t BN = (size_t)c->B * c->Np;
  TRY(dev_alloc(c, &c->d_m, BN * D));
  TRY(dev_alloc(c, &c->d_S, BN * DD));
  TRY(dev_alloc(c, &c->d_Ef, BN * D));
  if (cfg->model == VGPA_MODEL_L96 && D <= kMaxSmallD) TRY(dev_alloc(c, &c->d_Am, BN * D));
  TRY(dev_alloc(c, &c->d_dEm, BN * D));
  TRY(dev_alloc(c, &c->d_lam, BN * D));
  TRY(dev_alloc(c, &c->d_et, BN));
  TRY(dev_alloc(c, &c->d_eobs, (size_t)c->B));
  TRY(dev_alloc(c, &c->d_esde, (size_t)c->B));
  TRY(dev_alloc(c, &c->d_f, (size_t)c->B));
  TRY(dev_alloc(c, &c->d_status, (size_t)c->B));
  TRY(dev_alloc(c, &c->d_jm, (size_t)c->B * (c->M > 0 ? c->M : 1) * D));
  TRY(dev_alloc(c, &c->d_Sigma, DD));
  TRY(dev_alloc(c, &c->d_isig, DD));
  TRY(dev_alloc(c, &c->d_isg, (size_t)D));
  TRY(dev_alloc(c, &c->d_m0, (size_t)D));
  TRY(dev_alloc(c, &c->d_S0, DD));
  TRY(dev_alloc(c, &c->d_op_m0, (size_t)D));
  TRY(dev_alloc(c, &c->d_op_S0, DD));
  TRY(dev_alloc(c, &c->d_op_Sigma, DD));
  TRY(dev_alloc(c, &c->d_obs_idx, (size_t)c->Np));
  TRY(dev_alloc(c, &c->d_obs_t, (size_t)(c->M > 0 ? c->M : 1)));
  TRY(dev_alloc(c, &c->d_obs_y, (size_t)(c->M > 0 ? c->M : 1) * D));
  TRY(dev_alloc(c, &c->d_Q, DD));
  TRY(dev_alloc(c, &c->d_K, DD));
  TRY(dev_alloc(c, &c->d_rinv, (size_t)D));
  TRY(dev_alloc(c, &c->d_jsc, DD));
  HTRY(hipMemsetAsync(c->d_status, 0, sizeof(int32_t) * c->B, c->stream));
  HTRY(hipMemsetAsync(c->d_eobs, 0, sizeof(double) * c->B, c->stream));
  HTRY(hipMemsetAsync(c->d_jm, 0, sizeof(double) * (size_t)c->B * (c->M > 0 ? c->M : 1) * D, c->stream));
  HTRY(hipMemsetAsync(c->d_jsc, 0, sizeof(double) * DD, c->stream));

  TRY(upload(c, c->d_Sigma, sigma.data(), DD));
  c->h_sigma = sigma;
  c->h_isig = isig;
  TRY(upload(c, c->d_isig, isig.data(), DD));
  TRY(upload(c, c->d_isg, isg.data(), (size_t)D));
  c->isg0 = isg[0];
  if (cfg->m0) TRY(upload(c, c->d_m0, cfg->m0, (size_t)D));
  if (cfg->s0) { TRY(upload(c, c->d_S0, cfg->s0, DD)); c->h_s0.assign(cfg->s0, cfg->s0 + DD); }

  std::vector<int32_t> obs_idx(c->Np, -1);
  std::vector<double> Q(DD, 0.0), K(DD, 0.0), rinv(D, 0.0), jsc(DD, 0.0);
  if (c->M > 0 && cfg->obs_t && cfg->obs_y && cfg->obs_noise) {
    if (!index_obs_times(cfg->obs_t, c->M, c->Np, obs_idx.data())) FAIL(VGPA_ERR_ARG, "obs_t must be strictly increasing indices in [0, Np)");
    rc = obs_constants(D, c->M, single, cfg->obs_noise, cfg->obs_h, Q.data(), K.data(), rinv.data(), jsc.data(), &c->obs_const, &c->obs_diag);
    if (rc) FAIL(rc, single ? "observation noise must be positive" : "observation noise matrix is not positive definite");
    c->inputs_sym = c->inputs_sym && is_symmetric(jsc.data(), D);
    c->shared_obs_diag = c->obs_diag;
    c->h_obs_t.assign(cfg->obs_t, cfg->obs_t + c->M);
    c->h_R.assign(cfg->obs_noise, cfg->obs_noise + (single ? 1 : DD));
    c->h_H.assign(DD, 0.0);
    for (int i = 0; i < D; i++) c->h_H[(size_t)i * D + i] = 1.0;
    if (cfg->obs_h) c->h_H.assign(cfg->obs_h, cfg->obs_h + (single ? 1 : DD));
    if (D > kMaxSmallD) TRY(dev_alloc(c, &c->d_obs_part, (size_t)c->B * c->M));   // one workgroup per observation
    TRY(upload(c, c->d_obs_t, cfg->obs_t, (size_t)c->M));
    TRY(upload(c, c->d_obs_y, cfg->obs_y, (size_t)c->M * D));
  }
  c->h_obs_idx = obs_idx;
  TRY(upload(c, c->d_obs_idx, obs_idx.data(), (size_t)c->Np));
  if (D > kMaxSmallD && c->full && cfg->model == VGPA_MODEL_L96) {
    // resident large-D sweep: S, dEsde_dS, Psi next to the caller's x and gradient.  Stream when asked to, or when
    // that does not fit into what is free on the device now.
    size_t free_b = 0, total_b = 0;
    HTRY(hipMemGetInfo(&free_b, &total_b));
    const double need = 8.0 * (double)BN * (double)DD * 4.0;        // dEs + Psi + the caller's x and g still to come
    c->stream_ld = (cfg->flags & VGPA_FLAG_STREAM_LARGE_D) != 0 || need > 0.9 * (double)free_b;
    if (c->stream_ld && c->B > 1)      // (everything allocated so far goes back: this fires exactly when memory is short)
      FAIL(VGPA_ERR_UNSUPPORTED, "the time-chunked large-D sweep holds one problem (a batch of %d does not fit resident)", c->B);
    c->lde_budget = std::fmin(16.0e9, std::fmax(1.0e9, 0.05 * (double)free_b));   // workspace of the batched energy terms
    c->ld_chunk = ld::lde_batch(D, c->lde_budget) - 1;   // a chunk evaluates ld_chunk + 1 grid points: exactly one energy batch
    if (c->ld_chunk > c->Np - 1) c->ld_chunk = c->Np - 1;
    if (c->ld_chunk < 1) c->ld_chunk = 1;
  }
  TRY(upload(c, c->d_Q, Q.data(), DD));
  TRY(upload(c, c->d_K, K.data(), DD));
  TRY(upload(c, c->d_rinv, rinv.data(), (size_t)D));
  TRY(upload(c, c->d_jsc, jsc.data(), DD));
  {      // the same (symmetric) matrix as a packed lower triangle, for the backward kernels that read a packed dEsde_dS stream
    std::vector<double> jp((size_t)DD, 0.0);
    for (int r = 0; r < D; r++)
      for (int q = 0; q <= r; q++) jp[(size_t)r * (r + 1) / 2 + q] = jsc[(size_t)r * D + q];
    TRY(dev_alloc(c, &c->d_jscp, DD));
    TRY(upload(c, c->d_jscp, jp.data(), DD));
  }
  HTRY(hipStreamSynchronize(c->stream));
  BatchInputs& in = c->in;       // every problem on the inputs of vgpa_config
  in.m0 = {c->d_m0, 0}; in.S0 = {c->d_S0, 0}; in.obs_y = {c->d_obs_y, 0}; in.obs_t = {c->d_obs_t, 0}; in.obs_idx = {c->d_obs_idx, 0};
  in.Sigma = {c->d_Sigma, 0}; in.isig = {c->d_isig, 0}; in.isg = {c->d_isg, 0};
  in.Q = {c->d_Q, 0}; in.K = {c->d_K, 0}; in.rinv = {c->d_rinv, 0}; in.jsc = {c->d_jsc, 0}; in.jscp = {c->d_jscp, 0};
  make_plan(c);
#undef FAIL
#undef TRY
#undef HTRY
  *out = c;
  return VGPA_OK;
}

int vgpa_synchronize(vgpa_ctx* c) {
  if (!c) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}

void* vgpa_stream(vgpa_ctx* c) { return c ? (void*)c->stream : nullptr; }

// ---- operator level ---------------------------------------------------------------------------------
int vgpa_solve_fwd(vgpa_ctx* c, const double* lin_a, const double* off_b, const double* m0, const double* s0,
                   const double* sigma, double* mt, double* st) {
  if (!c || !lin_a || !off_b || !m0 || !s0 || !sigma || !mt || !st) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t BN = (size_t)c->B * c->Np;
  int rc;
  c->res.taken_over();
  if ((rc = ingest_ab(c, lin_a, off_b))) return rc;
  if ((rc = upload(c, c->d_op_m0, m0, (size_t)c->D))) return rc;
  if ((rc = upload(c, c->d_op_S0, s0, c->DD))) return rc;
  if ((rc = upload(c, c->d_op_Sigma, sigma, c->DD))) return rc;
  const bool sym = is_symmetric(s0, c->D) && is_symmetric(sigma, c->D);
  if ((rc = run_fwd(c, {c->d_op_m0, 0}, {c->d_op_S0, 0}, {c->d_op_Sigma, 0}, sym))) return rc;
  if ((rc = download(c, mt, c->d_m, BN * c->D))) return rc;
  if ((rc = download(c, st, c->d_S, BN * c->DD))) return rc;
  return vgpa_synchronize(c);
}

int vgpa_solve_bwd(vgpa_ctx* c, const double* lin_a, const double* desde_dm, const double* desde_ds,
                   const double* deobs_dm, const double* deobs_ds, double* lam, double* psi) {
  if (!c || !lin_a || !desde_dm || !desde_ds || !deobs_dm || !deobs_ds || !lam || !psi) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t BN = (size_t)c->B * c->Np;
  int rc;
  c->res.taken_over();
  if ((rc = ensure(c, &c->d_jm_dense, BN * c->D))) return rc;
  if ((rc = ensure(c, &c->d_js_dense, BN * c->DD))) return rc;
  if ((rc = ingest_ab(c, lin_a, nullptr))) return rc;
  if ((rc = upload(c, c->d_dEm, desde_dm, BN * c->D))) return rc;
  if ((rc = ensure(c, &c->d_dEs, BN * c->DD))) return rc;
  if ((rc = ensure(c, &c->d_psi, BN * c->DD))) return rc;
  if ((rc = upload(c, c->d_dEs, desde_ds, BN * c->DD))) return rc;
  if ((rc = upload(c, c->d_jm_dense, deobs_dm, BN * c->D))) return rc;
  if ((rc = upload(c, c->d_js_dense, deobs_ds, BN * c->DD))) return rc;
  const bool sym = stack_symmetric(desde_ds, BN, c->D) && stack_symmetric(deobs_ds, BN, c->D);
  if ((rc = run_bwd(c, true, sym))) return rc;
  if ((rc = download(c, lam, c->d_lam, BN * c->D))) return rc;
  if ((rc = download(c, psi, c->d_psi, BN * c->DD))) return rc;
  return vgpa_synchronize(c);
}

// dEsde/dtheta and dEsde/dSigma of <model>.energy (ornstein_uhlenbeck.py:222-226, double_well.py:250-254,
// lorenz_63.py:329-342, lorenz_96.py:421-434): the kernels emit the per-grid-point integrands, one trapezoid per
// component reduces them, the O(D^3) scaling by Sigma^-1 is finished on the host.
int vgpa_energy_full(vgpa_ctx* c, const double* lin_a, const double* off_b, const double* mt, const double* st,
                     double* esde_out, double* efx, double* edf, double* desde_dm, double* desde_ds,
                     double* desde_dth, double* desde_dsig) {
  if (!c || !lin_a || !off_b || !mt || !st) return fail(c, VGPA_ERR_ARG, "null argument");
  if ((desde_dth != nullptr) != (desde_dsig != nullptr)) return fail(c, VGPA_ERR_ARG, "dEsde_dth and dEsde_dsig come together");
  const bool hyper = desde_dth != nullptr;
  if (hyper && c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_STATE, "context has no stochastic model");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int D = c->D;
  const int H = c->single ? 1 : 2 * D;
  const size_t BN = (size_t)c->B * c->Np;
  int rc;
  c->res.taken_over();
  if (edf && (rc = ensure(c, &c->d_Edf, BN * c->DD))) return rc;
  if (hyper && !c->d_hyp) {
    if ((rc = dev_alloc(c, &c->d_hyp, BN * H))) return rc;
    if ((rc = dev_alloc(c, &c->d_hypT, (size_t)c->B * H))) return rc;
  }
  if ((rc = ingest_ab(c, lin_a, off_b))) return rc;
  if ((rc = upload(c, c->d_m, mt, BN * c->D))) return rc;
  if ((rc = upload(c, c->d_S, st, BN * c->DD))) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_status, 0, sizeof(int32_t) * c->B, c->stream));
  if ((rc = run_energy(c, edf ? c->d_Edf : nullptr, Resident::DesLayout::Whole, hyper))) return rc;
  if ((rc = run_reduce(c))) return rc;
  if (hyper) LAUNCH_TRY(c, "trapezoid launch", launch_trapz_multi(c->d_hyp, c->Np, H, c->B, c->cfg.dt, c->d_hypT, c->stream));
  if ((rc = check_status(c))) return rc;
  std::vector<double> T(hyper ? (size_t)c->B * H : 0), esde(c->B);
  if ((rc = download(c, esde.data(), c->d_esde, esde.size()))) return rc;
  if (hyper && (rc = download(c, T.data(), c->d_hypT, T.size()))) return rc;
  if (efx && (rc = download(c, efx, c->d_Ef, BN * c->D))) return rc;
  if (edf && (rc = download(c, edf, c->d_Edf, BN * c->DD))) return rc;
  if (desde_dm && (rc = download(c, desde_dm, c->d_dEm, BN * c->D))) return rc;
  if (desde_ds && (rc = download(c, desde_ds, c->d_dEs, BN * c->DD))) return rc;
  if ((rc = vgpa_synchronize(c))) return rc;
  if (esde_out) for (int p = 0; p < c->B; p++) esde_out[p] = esde[p];
  if (!hyper) return VGPA_OK;
  for (int p = 0; p < c->B; p++) {
    const double* Tp = T.data() + (size_t)p * H;
    if (c->single) {
      const double s1 = sigma1_of(c, p);
      desde_dth[p] = (c->cfg.model == VGPA_MODEL_DW ? 4.0 : 1.0) * Tp[0] / s1;
      desde_dsig[p] = -esde[p] / s1;
      continue;
    }
    const double* is = isig_of(c, p);
    for (int i = 0; i < D; i++) desde_dth[(size_t)p * D + i] = is[(size_t)i * D + i] * Tp[i];
    double* out = desde_dsig + (size_t)p * D * D;          // -0.5 * Sigma^-1 diag(v) Sigma^-1
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) {
        double sacc = 0.0;
        for (int k = 0; k < D; k++) sacc += (is[(size_t)i * D + k] * Tp[D + k]) * is[(size_t)k * D + j];
        out[(size_t)i * D + j] = -0.5 * sacc;
      }
  }
  return VGPA_OK;
}

int vgpa_energy(vgpa_ctx* c, const double* lin_a, const double* off_b, const double* mt, const double* st,
                double* esde, double* efx, double* edf, double* desde_dm, double* desde_ds) {
  return vgpa_energy_full(c, lin_a, off_b, mt, st, esde, efx, edf, desde_dm, desde_ds, nullptr, nullptr);
}

int vgpa_obs_energy(vgpa_ctx* c, const double* mt, const double* st, double* eobs, double* deobs_dm, double* deobs_ds) {
  if (!c || !mt || !st) return fail(c, VGPA_ERR_ARG, "null argument");
  if (!c->cfg.obs_t && c->M > 0) return fail(c, VGPA_ERR_STATE, "context has no observations");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t BN = (size_t)c->B * c->Np;
  int rc;
  c->res.taken_over();
  if ((rc = upload(c, c->d_m, mt, BN * c->D))) return rc;
  if ((rc = upload(c, c->d_S, st, BN * c->DD))) return rc;
  ObsArgs a = obs_args(c);
  LAUNCH_TRY(c, "obs launch", launch_obs(a, c->stream));
  if (eobs && (rc = download(c, eobs, c->d_eobs, (size_t)c->B))) return rc;
  if (deobs_dm || deobs_ds) {
    if ((rc = ensure(c, &c->d_jm_dense, BN * c->D))) return rc;
    if ((rc = ensure(c, &c->d_js_dense, BN * c->DD))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_jm_dense, 0, sizeof(double) * BN * c->D, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_js_dense, 0, sizeof(double) * BN * c->DD, c->stream));
    LAUNCH_TRY(c, "obs dense launch", launch_obs_dense(a, c->in.jsc.rows, c->d_jm_dense, c->d_js_dense, c->stream));
    if (deobs_dm && (rc = download(c, deobs_dm, c->d_jm_dense, BN * c->D))) return rc;
    if (deobs_ds && (rc = download(c, deobs_ds, c->d_js_dense, BN * c->DD))) return rc;
  }
  return vgpa_synchronize(c);
}

// ---- fused objective --------------------------------------------------------------------------------
static int free_energy(vgpa_ctx* c, const double* x, bool on_device, double* f_host) {
  if (!c || !x || !f_host) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = ingest_x(c, x, on_device))) return rc;
  if ((rc = enqueue_free_energy(c))) return rc;
  return vgpa_fetch_f(c, f_host);
}
int vgpa_free_energy(vgpa_ctx* c, const double* x, double* f) { return free_energy(c, x, false, f); }
int vgpa_free_energy_dev(vgpa_ctx* c, const double* x_dev, double* f_host) { return free_energy(c, x_dev, true, f_host); }

int vgpa_fetch_f(vgpa_ctx* c, double* f_host) {
  if (!c || !f_host) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  // F and the status words through one pinned block, one synchronisation (a pageable destination makes the copy synchronous by itself,
  // and check_status is a second round trip: ~0.3 ms per call of a batched context, 15 % of an Ornstein-Uhlenbeck step)
  const size_t B = (size_t)c->B;
  if (!c->h_fs && hipHostMalloc(&c->h_fs, B * (sizeof(double) + sizeof(int32_t))) != hipSuccess) {
    c->h_fs = nullptr;
    (void)hipGetLastError();
    int rc;
    if ((rc = download(c, f_host, c->d_f, B))) return rc;
    return check_status(c);
  }
  double* hf = static_cast<double*>(c->h_fs);
  int32_t* hs = reinterpret_cast<int32_t*>(hf + B);
  HIP_TRY(c, hipMemcpyAsync(hf, c->d_f, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hs, c->d_status, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::memcpy(f_host, hf, B * sizeof(double));
  return report_status(c, hs);
}

static int finish_gradient(vgpa_ctx* c, double* g_dev);

// F and the gradient in one go (df(x, eval_fun=True)): the streamed context folds both into one chunked pass
static int enqueue_sweep(vgpa_ctx* c, double* g_dev) {
  if (c->stream_ld) return enqueue_stream_sweep(c, g_dev);
  if (c->plan.lane_pass) return enqueue_lane_sweep(c, g_dev);
  int rc = enqueue_free_energy(c);
  return rc ? rc : finish_gradient(c, g_dev);
}

static int finish_gradient(vgpa_ctx* c, double* g_dev) {
  // cached state = (m, S): the chunked pass recomputes the energy terms on its way back
  if (c->stream_ld) return prof_end(c, stream_pass(c, g_dev));
  // gradient(x, eval_fun=False) behind a fused F: the pass again, now with the recursion
  if (c->plan.lane_pass && !c->res.terms) return prof_end(c, run_lane_pass(c, g_dev));
  int rc = VGPA_OK;
  if (c->plan.grad_in_bwd_now && c->res.S == Resident::SLayout::Packed) {   // backward recursion + gradient assembly in one kernel (phase "bwd"; "grad" is empty)
    for (int r = diag_repeat("bwd"); r > 0 && rc == VGPA_OK; r--) rc = run_bwd(c, false, c->plan.sym_inputs, g_dev);
    prof_mark(c, 3);
    return prof_end(c, rc);
  }
  if (c->res.bwd == Resident::Bwd::None) {   // (F-only evaluation before: the recursion now, with Q''_t for the assembly kernel)
    for (int r = diag_repeat("bwd"); r > 0 && rc == VGPA_OK; r--) rc = run_bwd(c, false, c->plan.sym_inputs);
    prof_mark(c, 3);
  }
  for (int r = diag_repeat("grad"); r > 0 && rc == VGPA_OK; r--) rc = run_grad(c, g_dev);
  return prof_end(c, rc);
}

int vgpa_gradient(vgpa_ctx* c, const double* x_or_null, double* g) {
  if (!c || !g) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = ensure(c, &c->d_g, (size_t)c->B * c->len_x))) return rc;
  if (x_or_null) {
    if ((rc = ingest_x(c, x_or_null, false))) return rc;
    if ((rc = enqueue_sweep(c, c->d_g))) return rc;
  } else if (!c->res.cached) {
    return fail(c, VGPA_ERR_STATE, "gradient(x, eval_fun=False) needs the state cached by a previous free_energy");
  } else if ((rc = finish_gradient(c, c->d_g))) return rc;
  if ((rc = download(c, g, c->d_g, (size_t)c->B * c->len_x))) return rc;
  return check_status(c);
}

int vgpa_sweep(vgpa_ctx* c, const double* x, double* f, double* g) {
  if (!c || !x || !f || !g) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = ensure(c, &c->d_g, (size_t)c->B * c->len_x))) return rc;
  if ((rc = ingest_x(c, x, false))) return rc;
  if ((rc = enqueue_sweep(c, c->d_g))) return rc;
  if ((rc = download(c, g, c->d_g, (size_t)c->B * c->len_x))) return rc;
  return vgpa_fetch_f(c, f);
}

int vgpa_sweep_enqueue(vgpa_ctx* c, const double* x_dev, double* g_dev) {
  if (!c || !x_dev || !g_dev) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = ingest_x(c, x_dev, true))) return rc;
  return enqueue_sweep(c, g_dev);
}

int vgpa_sweep_dev(vgpa_ctx* c, const double* x_dev, double* f_host, double* g_dev) {
  if (!c || !f_host) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = vgpa_sweep_enqueue(c, x_dev, g_dev))) return rc;
  return vgpa_fetch_f(c, f_host);
}

int vgpa_energy_parts(vgpa_ctx* c, double* e0, double* esde, double* eobs) {
  if (!c) return VGPA_ERR_ARG;
  if (!c->res.cached) return fail(c, VGPA_ERR_STATE, "no cached state");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if (e0) for (int p = 0; p < c->B; p++) e0[p] = e0_of(c, p);
  if (esde && (rc = download(c, esde, c->d_esde, (size_t)c->B))) return rc;
  if (eobs && (rc = download(c, eobs, c->d_eobs, (size_t)c->B))) return rc;
  return vgpa_synchronize(c);
}

// dF/dtheta at fixed (A_t, b_t) from the cached state.  In all four models the drift is affine in theta and E_sde takes the diagonal of
// Sigma^-1 only, so dF/dtheta_k = sum_i (Sigma^-1)_ii int <(f - g)_i d f_i / d theta_k> dt: the residuals the energy kernels form, summed
// before squaring.  OU / double well / Lorenz-63: the closed forms of <model>.energy (dEsde_dth).  Lorenz-96: the UNSCENTED mean of the
// residual with the flat roll of the energy itself -- not the reference's dEsde_dth, which is built from the closed-form mean drift and
// is not the derivative of the F computed here.  Nothing of the cached state is written.
int vgpa_theta_gradient(vgpa_ctx* c, double* out) {
  if (!c || !out) return fail(c, VGPA_ERR_ARG, "null argument");
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  if (c->stream_ld) return fail(c, VGPA_ERR_UNSUPPORTED, "dF/dtheta is not built for the time-chunked large-D sweep");
  if (!c->res.cached) return fail(c, VGPA_ERR_STATE, "no cached state: theta_gradient needs the state cached by a previous free_energy / sweep");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int D = c->D, B = c->B, Np = c->Np, nth = c->cfg.n_theta;
  const size_t BN = (size_t)B * Np;
  int rc, H = 1;                       // H: doubles per problem in the result buffer
  const double* res = nullptr;
  if ((rc = ensure(c, &c->d_thT, (size_t)B * kMaxTheta))) return rc;
  if (c->plan.lane_pass) {             // one lane per problem over x and the time-major moments; nothing per grid point is written
    ThetaLaneArgs q{};
    q.model = c->cfg.model; q.D = D; q.Np = Np; q.batch = B; q.bpad = c->bpad; q.dt = c->cfg.dt; q.stride_x = c->len_x;
    q.A = ctx_A(c); q.b = ctx_b(c); q.msT = c->d_msT;
    copy_theta(c, q.theta);
    q.theta_v = c->in.theta.rows; q.out = c->d_thT;
    LAUNCH_TRY(c, "theta lane kernel launch", launch_theta_lane(q, c->stream));
    H = D; res = c->d_thT;
  } else if (c->cfg.model == VGPA_MODEL_L96) {
    if ((rc = ensure(c, &c->d_tg, BN))) return rc;
    if (D > kMaxSmallD) {
      if ((rc = ensure_lde_ws(c))) return rc;
      const size_t NpD = (size_t)Np * D, NpDD = (size_t)Np * c->DD;
      for (int p = 0; p < B; p++)
        LAUNCH_TRY(c, "large-D theta integrand", ld::lde_theta_integrand(D, Np, theta_of(c, p)[0], c->in.isg.of(p), ctx_A(c) + p * c->len_x,
                                                                         ctx_b(c) + p * c->len_x, c->d_m + p * NpD, c->d_S + p * NpDD,
                                                                         c->d_tg + (size_t)p * Np, c->d_status + p, c->d_lde_ws, c->lde_nb, c->stream));
    } else {                           // the energy kernel over the resident (m_t, S_t) in the layout they are in, integrand only
      EnergyArgs a = energy_args(c, nullptr);
      a.hyp = nullptr; a.tg = c->d_tg;
      LAUNCH_TRY(c, "theta integrand launch", launch_energy(a, c->stream));
    }
    LAUNCH_TRY(c, "trapezoid launch", launch_trapz_multi(c->d_tg, Np, 1, B, c->cfg.dt, c->d_thT, c->stream));
    H = 1; res = c->d_thT;
  } else {                             // wave / workgroup contexts of the small models: the hyp integrands of the energy kernels
    H = c->single ? 1 : 2 * D;
    if ((rc = materialize_moments(c))) return rc;
    if ((rc = ensure(c, &c->d_hyp, BN * H))) return rc;
    if ((rc = ensure(c, &c->d_hypT, (size_t)B * H))) return rc;
    EnergyArgs a = energy_args(c, nullptr);
    a.hyp = c->d_hyp; a.hyp_only = 1;
    LAUNCH_TRY(c, "theta integrand launch", launch_energy(a, c->stream));
    LAUNCH_TRY(c, "trapezoid launch", launch_trapz_multi(c->d_hyp, Np, H, B, c->cfg.dt, c->d_hypT, c->stream));
    res = c->d_hypT;
  }
  std::vector<double> T((size_t)B * H);
  if ((rc = download(c, T.data(), res, T.size()))) return rc;
  // the status words of the resident state (set by the sweep that cached it, and by the Lorenz-96 integrand kernels above, which end at a
  // bad pivot without writing their integrand): behind an evaluation that failed with VGPA_ERR_NOT_PD this fails the same way
  if ((rc = check_status(c))) return rc;
  for (int p = 0; p < B; p++) {
    const double* Tp = T.data() + (size_t)p * H;
    if (c->single) out[p] = (c->cfg.model == VGPA_MODEL_DW ? 4.0 : 1.0) * Tp[0] / sigma1_of(c, p);      // (the factors of vgpa_energy_full)
    else if (c->cfg.model == VGPA_MODEL_L96) out[p] = Tp[0];                                              // (Sigma^-1 is in the integrand)
    else for (int i = 0; i < nth; i++) out[(size_t)p * nth + i] = isig_of(c, p)[(size_t)i * D + i] * Tp[i];
  }
  return VGPA_OK;
}

// a buffer of vgpa_sample_paths that grows on demand: at least `count` doubles behind *p
static int grow(vgpa_ctx* c, double** p, size_t* have, size_t count) {
  if (*p && *have >= count) return VGPA_OK;
  if (*p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(*p); *p = nullptr; *have = 0; }
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(double));
  if (e != hipSuccess) return fail(c, VGPA_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s", count * sizeof(double), hipGetErrorString(e));
  *p = static_cast<double*>(q); *have = count;
  return VGPA_OK;
}

// The lower Cholesky factors of `scale` times n host matrices D x D (n = 1: shared by the batch, else one per problem), uploaded into *buf;
// *diag: every factor is diagonal.  VGPA_ERR_NOT_PD names the row.
static int factor_rows(vgpa_ctx* c, const double* src, int n, double scale, const char* what, double** buf, size_t* have, Rows<double>* out, bool* diag) {
  const int D = c->D;
  const size_t DD = c->DD;
  std::vector<double> a(DD), l((size_t)n * DD);
  int rc;
  *diag = true;
  for (int p = 0; p < n; p++) {
    for (size_t e = 0; e < DD; e++) a[e] = src[p * DD + e] * scale;
    if (!host_cholesky_lower(D, a.data(), l.data() + p * DD)) return fail(c, VGPA_ERR_NOT_PD, "problem %d: %s is not positive definite.", p, what);
    for (int i = 0; i < D; i++)
      for (int j = 0; j < i; j++) *diag = *diag && l[p * DD + (size_t)i * D + j] == 0.0;
  }
  if ((rc = grow(c, buf, have, l.size()))) return rc;
  HIP_TRY(c, hipMemcpyAsync(*buf, l.data(), l.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the host rows live on this stack frame)
  *out = {*buf, n > 1 ? DD : 0};
  return VGPA_OK;
}

// The lower factors of Sigma dt of the rows in force into a.R / R_stride / R_diag; a dense Sigma is the caller's to refuse
static int factor_noise(vgpa_ctx* c, SampleArgs* a) {
  const bool own_Sigma = !c->in.h_Sigma.empty();     // (the host copy of the rows in force)
  Rows<double> R;
  bool diag = true;
  int rc;
  if ((rc = factor_rows(c, own_Sigma ? c->in.h_Sigma.data() : c->h_sigma.data(), own_Sigma ? c->B : 1, c->cfg.dt, "noise matrix times dt",
                        &c->d_sp_R, &c->sp_R_n, &R, &diag))) return rc;
  a->R = R.rows; a->R_stride = R.stride; a->R_diag = diag ? 1 : 0;
  return VGPA_OK;
}

// every one of the B x k slots lies in [0, n_paths); the caller's nouns: a "final slot" of a "trajectory", a "slot" of a "member"
static int check_slots(vgpa_ctx* c, const int32_t* slots, int32_t k, int32_t n_paths, const char* slot, const char* of) {
  for (size_t e = 0; e < (size_t)c->B * k; e++)
    if (slots[e] < 0 || slots[e] >= n_paths)
      return fail(c, VGPA_ERR_ARG, "problem %zu: %s %d of %s %zu does not lie in [0, %d)", e / k, slot, slots[e], of, e % k, n_paths);
  return VGPA_OK;
}

// Euler-Maruyama paths of the posterior process or of the model SDE (see vgpa_hip.h), and -- logw set: vgpa_sample_paths_weighted,
// DESIGN.md s.4.9 -- the weights of the posterior paths against the model SDE and the data, with `out` optional and every x_0 to `start`.  Reads x
// and the inputs in force; of the cached state nothing is written.  The arguments have been checked by the entry points.
// sample_args: everything of SampleArgs but the result buffers -- the factors, the start, x ingested and, weighted, the model's theta and the
// observation model in force; shared with vgpa_particle_filter.
static int sample_args(vgpa_ctx* c, int kind, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, bool weighted,
                       SampleArgs* args) {
  if (c->D > kMaxSmallD) return fail(c, VGPA_ERR_UNSUPPORTED, "sample paths are built for D <= %d (D = %d)", kMaxSmallD, c->D);
  if (kind == VGPA_PATHS_POSTERIOR && !x && !c->res.cached)
    return fail(c, VGPA_ERR_STATE, "no cached state: sample_paths without x needs the state cached by a previous free_energy / sweep");
  if (!x0 && !(c->cfg.m0 && c->cfg.s0)) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0: the paths need a start x0");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const int D = c->D, B = c->B;
  int rc;
  SampleArgs& a = *args;
  a = SampleArgs{};
  a.kind = kind; a.model = c->cfg.model; a.D = D; a.Np = c->Np; a.batch = B; a.n_paths = n_paths; a.stride = stride;
  a.n_keep = (c->Np - 1) / stride + 1; a.dt = c->cfg.dt; a.seed = seed;
  Rows<double> L0;
  bool l0_diag = true;
  const bool own_S0 = !c->in.h_S0.empty();     // (the host copy of the rows in force)
  if ((rc = factor_noise(c, &a))) return rc;
  if (weighted && !a.R_diag) return fail(c, VGPA_ERR_UNSUPPORTED, "the weights of sampled paths are built for a diagonal Sigma (a dense Sigma is in force)");
  if (x0) {
    if ((rc = grow(c, &c->d_sp_x0, &c->sp_x0_n, (size_t)B * D))) return rc;
    if ((rc = upload(c, c->d_sp_x0, x0, (size_t)B * D))) return rc;
    a.x0 = c->d_sp_x0;
  } else {
    if ((rc = factor_rows(c, own_S0 ? c->in.h_S0.data() : c->h_s0.data(), own_S0 ? B : 1, 1.0, "initial covariance", &c->d_sp_L0, &c->sp_L0_n,
                          &L0, &l0_diag))) return rc;
    a.m0 = c->in.m0.rows; a.m0_stride = c->in.m0.stride; a.L0 = L0.rows; a.L0_stride = L0.stride;
  }
  if (kind == VGPA_PATHS_POSTERIOR) {
    if (x) {
      if ((rc = ingest_x(c, x, false))) return rc;
      c->res.cache_dropped();           // (d_x no longer holds the x of the cached state)
    }
    a.A = ctx_A(c); a.b = ctx_b(c); a.stride_x = c->len_x;
  } else {
    copy_theta(c, a.theta);
    a.theta_v = c->in.theta.rows;
  }
  if (weighted) {      // both drifts, and the observation model in force as obs_args hands it to the E_obs kernels
    copy_theta(c, a.theta);
    a.theta_v = c->in.theta.rows;
    const ObsArgs o = obs_args(c);
    a.obs_t = o.obs_t; a.obs_t_stride = o.obs_t_stride; a.obs_y = o.obs_y; a.obs_y_stride = o.obs_y_stride;
    a.Q = o.Q; a.Q_stride = o.Q_stride; a.Q_diag = o.diag; a.n_obs = o.n_obs; a.n_obs_v = o.n_obs_v;
    a.obs_const = o.obs_const; a.obs_const_v = o.obs_const_v; a.obs_const_scale = c->single ? 1.0 : 0.5;
  }
  return VGPA_OK;
}

static int sample_paths(vgpa_ctx* c, int kind, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double* out,
                        double* start, double* logw) {
  SampleArgs a;
  int rc;
  if ((rc = sample_args(c, kind, x, x0, n_paths, stride, seed, logw != nullptr, &a))) return rc;
  const int D = c->D, B = c->B;
  const size_t n_out = (size_t)B * n_paths * a.n_keep * D, n_start = (size_t)B * n_paths * D, n_logw = (size_t)B * n_paths * 2;
  if (out) {
    if ((rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_out))) return rc;
    a.out = c->d_sp_out;
  }
  if (logw) {
    if ((rc = grow(c, &c->d_sp_logw, &c->sp_logw_n, n_logw)) || (rc = grow(c, &c->d_sp_start, &c->sp_start_n, n_start))) return rc;
    a.logw = c->d_sp_logw; a.start = c->d_sp_start;
  }
  LAUNCH_TRY(c, "sample paths launch", launch_sample_walk(logw ? Walk::Weighted : Walk::Plain, a, c->stream));
  if (out && (rc = download(c, out, c->d_sp_out, n_out))) return rc;
  if (logw && (rc = download(c, logw, c->d_sp_logw, n_logw))) return rc;
  if (logw && start && (rc = download(c, start, c->d_sp_start, n_start))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}

int vgpa_sample_paths(vgpa_ctx* c, int kind, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double* out) {
  if (!c) return VGPA_ERR_ARG;
  if (!out) return fail(c, VGPA_ERR_ARG, "null argument");
  if (kind != VGPA_PATHS_POSTERIOR && kind != VGPA_PATHS_MODEL) return fail(c, VGPA_ERR_ARG, "unknown kind of paths -> %d", kind);
  if (n_paths < 1 || stride < 1) return fail(c, VGPA_ERR_ARG, "n_paths and stride must be at least 1 (n_paths = %d, stride = %d)", n_paths, stride);
  if (kind == VGPA_PATHS_MODEL && x) return fail(c, VGPA_ERR_ARG, "paths of the model SDE take no x");
  if (kind == VGPA_PATHS_MODEL && c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_ARG, "context has no stochastic model (ODE-only): no model SDE to sample");
  return sample_paths(c, kind, x, x0, n_paths, stride, seed, out, nullptr, nullptr);
}

// Posterior paths with their importance weights against the model SDE and the data (see vgpa_hip.h)
int vgpa_sample_paths_weighted(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double* out,
                               double* start, double* logw) {
  if (!c) return VGPA_ERR_ARG;
  if (!logw) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_paths < 1 || stride < 1) return fail(c, VGPA_ERR_ARG, "n_paths and stride must be at least 1 (n_paths = %d, stride = %d)", n_paths, stride);
  if (c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_ARG, "context has no stochastic model: no model SDE to weigh the paths against");
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  return sample_paths(c, VGPA_PATHS_POSTERIOR, x, x0, n_paths, stride, seed, out, start, logw);
}

// The weighted cross moments of trajectories on the device (particle_lag.hip): what vgpa_particle_lag_covariance and
// vgpa_path_cross_moments share.  d_paths [B][n][n_keep][D] and d_w [B][n] (or nullptr) are on the device, h_rows [n_anchor] on the host
// and alive until the stream has been synchronised, which is the caller's; mean and cross are the caller's host arrays.
static bool cross_moments_fit(int B, int n_keep, int D, int n_anchor) {      // (one array of cross: at most 2^39 - 256 entries)
  return (double)B * (double)n_anchor * (double)n_keep * (double)D * (double)D <= 549755813632.0;
}
static int cross_moments(vgpa_ctx* c, const double* d_paths, const double* d_w, int n, int n_keep, int n_anchor, const int32_t* h_rows, double* mean,
                         double* cross) {
  const int D = c->D, B = c->B;
  const size_t n_mean = (size_t)B * n_keep * D, n_cross = n_mean * D * (size_t)n_anchor;
  int rc;
  if ((rc = grow(c, &c->d_pf[vgpa_ctx::PF_LAGR], &c->pf_n[vgpa_ctx::PF_LAGR], ((size_t)n_anchor + 1) / 2)) ||
      (rc = grow(c, &c->d_pf[vgpa_ctx::PF_LAG], &c->pf_n[vgpa_ctx::PF_LAG], n_mean + n_cross))) return rc;
  int32_t* d_rows = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_LAGR]);
  double* d_mean = c->d_pf[vgpa_ctx::PF_LAG];
  if ((rc = upload(c, d_rows, h_rows, (size_t)n_anchor))) return rc;
  PathMomentArgs g{};
  g.D = D; g.batch = B; g.n_paths = n; g.n_keep = n_keep; g.n_anchor = n_anchor;
  g.paths = d_paths; g.weights = d_w; g.anchor_rows = d_rows; g.mean = d_mean; g.cross = d_mean + n_mean;
  LAUNCH_TRY(c, "path cross moments launch", launch_path_cross_moments(g, c->stream));
  if ((rc = download(c, mean, d_mean, n_mean)) || (rc = download(c, cross, d_mean + n_mean, n_cross))) return rc;
  return VGPA_OK;
}

// The guided particle filter (see vgpa_hip.h): the weighted walk of vgpa_sample_paths_weighted cut at the observation
// indices of the batch, the particles resident between the cuts, a resampling step behind every cut that is an observation of some problem.
// ParticleRequest: what one of the entry points wants from it and where the results go (nullptr: not wanted).
// Its two choices: the rows the filter's slots carry along their lineages, and the pass that runs behind the filter.  A forecast behind
// the filter is "fc_moments is set"; it goes with Carry::None and Behind::None alone.
// (Carry -- nothing; the path statistics (Q, G, H); the event records (X, T, N) -- is vgpa_internal.h's: the walks carry by the same word)
// (the order matters: table() below takes every enumerator from Trajectories on as a pass with a slot table; a new pass of sums goes before it)
enum class Behind { None, Moments, Covariance, BackwardMoments, Marginals, LagCovariance, Trajectories, Backward, Conditional };
struct ParticleRequest {
  const double* x; const double* x0; int32_t n_paths; uint64_t seed; double ess_fraction; const double* prior_mu; const double* prior_tau;
  double* logw; double* state; double* ess; int32_t* resampled;      // (up to here: what every entry point has, filled in this order)
  int32_t* ancestors; double* clouds;                                // vgpa_particle_filter, vgpa_particle_conditional: the histories
  Carry rows; double* stats; double* mean;                            // the final rows, their weighted mean
  const double* levels; const int32_t* sides; double* cdf;           // Carry::Events: levels and sides [B][D]; the first-passage distribution
  int32_t stride = 1;                                                // of the grid indices the smoothers, the events and the forecast keep
  Behind behind;
  double* moments; double* lineage_ess;                              // Behind::Moments (lineage_ess: Covariance too)
  double* smooth_weights;                                            // Behind::BackwardMoments: moments; lineage_ess: the smoothing ESS; the table [B][M + 1][n]
  double* cov_mean; double* cov_second;                              // Behind::Covariance
  const double* mg_levels; int32_t n_levels; uint64_t* mass; uint64_t* qfinal;      // Behind::Marginals (lineage_ess too): ladders [B][D][L]
  // Behind::LagCovariance (lineage_ess too): anchor_rows [n_anchor] = anchors / stride; n_draw = n_paths: every final slot's trajectory,
  // walked as Behind::Trajectories walks it and kept on the device
  int32_t n_anchor; const int32_t* anchor_rows; double* lag_mean; double* lag_cross;
  // Behind::Trajectories / Backward (the table is drawn, not traced) / Conditional (slot 0 pinned to ref [B][Np][D]; n_draw = 1, paths: the
  // drawn trajectory); slots_out: where the table goes
  int32_t n_draw; const int32_t* final_slots; double* paths; int32_t* slots_out; const double* ref;
  // vgpa_particle_forecast: horizon steps behind the filter, or from `cloud` at index0; stride, n_draw, final_slots, slots_out as above
  int32_t horizon; const double* cloud; const double* cloud_logw; int32_t index0;
  double* fc_moments; double* members; double* state_end;
  bool sums() const { return behind == Behind::Moments || behind == Behind::Covariance || behind == Behind::BackwardMoments; }      // the replay with its weighted sums
  bool smoothed() const { return behind == Behind::BackwardMoments; }                          // ... under the backward smoother's weights
  bool lag() const { return behind == Behind::LagCovariance; }                                 // every final slot's trajectory and their contraction
  bool table() const { return behind >= Behind::Trajectories; }                                // a slot table and the walk of its trajectories
};

// One run: the filter, then what the request puts behind it.  The passes share the kernels' arguments, the cuts and where the particles are.
struct ParticleRun {
  vgpa_ctx* c; const ParticleRequest& q;
  SampleArgs a; PfArgs f;              // of the filter's segments; of the start and the steps between the segments
  std::vector<char> is_obs;            // [Np] the grid index is an observation of some problem
  std::vector<int> count;              // [B] each problem's own observation count
  double* cur; double* other;          // the particles: where they are, where the next step puts them
  double* st_cur; double* st_other;    // ... and their rows (Carry::Stats, Carry::Events)
  int n_keep, rows, slot_rows, n_blocks; size_t mom_len, n_table, n_traj;
  int k0 = 0;                          // the forecast: the absolute grid index of the cloud
  WalkOwn own;                         // what the filter's segments read alone: the events' levels and sides, the reference, on the device
  // what follows from the request, derived once in setup(): the histories the device keeps (ancestors, clouds, replaced log-weights),
  // the walk of the filter's segments and whether the step between them is the conditional filter's
  bool keep_anc = false, keep_clouds = false, keep_lw = false, pinned = false;
  Walk segment = Walk::Segment;

  int buf(int which, size_t count) { return grow(c, &c->d_pf[which], &c->pf_n[which], count); }      // d_pf[which]: at least `count` doubles

  // For each cut -- an observation index of some problem, and the last grid index --: the segment launch up to it, then, at an
  // observation, the step between two segments (from cur to other), and the particle buffers swap.
  int cuts(Walk walk, const char* what, SampleArgs& s, const char* step_what, const std::function<hipError_t(int)>& step, const WalkOwn& walk_own = {}) {
    int prev = 0;
    for (int k = 0; k < c->Np; k++) {
      if (!is_obs[k] && k != c->Np - 1) continue;
      s.k_begin = prev; s.k_end = k; s.pf_x = cur;
      hipError_t e = launch_sample_walk(walk, s, c->stream, walk_own);
      if (e != hipSuccess) return fail(c, VGPA_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
      s.seg_first = 0; prev = k;
      if (!is_obs[k]) continue;
      if ((e = step(k)) != hipSuccess) return fail(c, VGPA_ERR_DEVICE, "%s failed: %s", step_what, hipGetErrorString(e));
      std::swap(cur, other);
    }
    return VGPA_OK;
  }

  // The arguments of the kernels, the buffers of d_pf[] the request needs, the prior, the cuts
  int setup() {
    const int D = c->D, B = c->B, M = c->M, M1 = M > 0 ? M : 1;
    int rc;
    if ((rc = sample_args(c, VGPA_PATHS_POSTERIOR, q.x, q.x0, q.n_paths, 1, q.seed, true, &a))) return rc;
    const size_t n = (size_t)q.n_paths, BnD = (size_t)B * n * D, Bn = (size_t)B * n, BM = (size_t)B * M1;
    keep_anc = q.ancestors || q.behind != Behind::None;      // (every pass behind the filter reads the ancestors)
    keep_clouds = q.clouds || q.behind == Behind::Backward || q.smoothed() || q.behind == Behind::Conditional;      // (their pass reads the clouds on the device)
    keep_lw = q.behind == Behind::Backward || q.smoothed(); pinned = q.behind == Behind::Conditional;
    segment = pinned ? Walk::Conditional : q.rows == Carry::Events ? Walk::SegmentEvents : q.rows == Carry::Stats ? Walk::SegmentStats : Walk::Segment;
    const bool covariance = q.behind == Behind::Covariance, carried = q.rows != Carry::None;
    auto ints = [](size_t count) { return (count + 1) / 2; };      // int32 entries in a buffer of doubles
    if ((rc = buf(vgpa_ctx::PF_XA, BnD)) || (rc = buf(vgpa_ctx::PF_XB, BnD)) || (rc = buf(vgpa_ctx::PF_LW, Bn)) || (rc = buf(vgpa_ctx::PF_CUM, Bn)) ||
        (rc = buf(vgpa_ctx::PF_ANC, ints(Bn))) || (rc = buf(vgpa_ctx::PF_ESS, BM)) || (rc = buf(vgpa_ctx::PF_FLAG, ints(BM)))) return rc;
    if (keep_anc && (rc = buf(vgpa_ctx::PF_HANC, ints(BM * n)))) return rc;
    n_keep = (c->Np - 1) / q.stride + 1; slot_rows = M + 1; rows = M1 + 1; n_blocks = sample_segment_blocks(D, q.n_paths);
    n_table = (size_t)B * slot_rows * (size_t)q.n_draw; n_traj = (size_t)B * (size_t)q.n_draw * ((size_t)n_keep * D); mom_len = (size_t)n_keep * (covariance ? sample_cov_len(D) : (size_t)2 * D);
    if (q.table() && ((rc = buf(vgpa_ctx::PF_SLOTS, ints(n_table))) || (rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_traj)))) return rc;
    if (q.sums() && ((rc = buf(vgpa_ctx::PF_WTAB, (size_t)B * rows * n)) || (rc = buf(vgpa_ctx::PF_LESS, (size_t)B * rows)) ||
                      (rc = buf(vgpa_ctx::PF_PART, (size_t)B * n_blocks * mom_len)) || (rc = buf(vgpa_ctx::PF_MOM, (size_t)B * mom_len)))) return rc;
    if (q.smoothed() && ((rc = buf(vgpa_ctx::PF_SMX, BnD)) || (rc = buf(vgpa_ctx::PF_SMR, 2 * Bn + (size_t)B * kMaxSmallD)) ||
                         (rc = buf(vgpa_ctx::PF_SMP, (size_t)B * rows * smooth_column_blocks(q.n_paths))))) return rc;
    if (covariance && (rc = buf(vgpa_ctx::PF_COV, (size_t)B * n_keep * D * ((size_t)D + 1)))) return rc;
    if (q.behind == Behind::Marginals &&
        ((rc = buf(vgpa_ctx::PF_WTAB, (size_t)B * rows * n)) || (rc = buf(vgpa_ctx::PF_LESS, (size_t)B * rows)) || (rc = buf(vgpa_ctx::PF_QTAB, (size_t)B * rows * n)) || (rc = buf(vgpa_ctx::PF_QFIN, Bn)) ||
         (rc = buf(vgpa_ctx::PF_MGL, (size_t)B * D * q.n_levels)) || (rc = buf(vgpa_ctx::PF_MASS, (size_t)B * n_keep * D * ((size_t)q.n_levels + 1))))) return rc;
    // (the trajectories of all n final slots stay in d_sp_out, batch n n_keep D doubles; the normalised final weights behind the descendant ones)
    if (q.lag() && ((rc = buf(vgpa_ctx::PF_SLOTS, ints(n_table))) || (rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_traj)) ||
                    (rc = buf(vgpa_ctx::PF_WTAB, (size_t)B * rows * n + Bn)) || (rc = buf(vgpa_ctx::PF_LESS, (size_t)B * rows)))) return rc;
    if (keep_clouds && (rc = buf(vgpa_ctx::PF_CLOUDS, BM * n * D))) return rc;
    if (keep_lw && (rc = buf(vgpa_ctx::PF_HLW, BM * n))) return rc;
    if (carried && ((rc = buf(vgpa_ctx::PF_STA, 3 * BnD)) || (rc = buf(vgpa_ctx::PF_STB, 3 * BnD)) || (rc = buf(vgpa_ctx::PF_MEAN, (size_t)B * 3 * D)))) return rc;
    f = PfArgs{};
    f.D = D; f.batch = B; f.n_paths = q.n_paths; f.M = M1; f.seed = q.seed; f.ess_fraction = q.ess_fraction;
    f.x0 = a.x0; f.m0 = a.m0; f.L0 = a.L0; f.m0_stride = a.m0_stride; f.L0_stride = a.L0_stride;
    f.obs_const = a.obs_const; f.obs_const_v = a.obs_const_v; f.obs_const_scale = a.obs_const_scale;
    f.obs_t = a.obs_t; f.obs_t_stride = a.obs_t_stride; f.n_obs = a.n_obs; f.n_obs_v = a.n_obs_v;
    if (q.prior_mu && !q.x0) {
      Rows<double> Lt;
      bool lt_diag = true;
      if ((rc = factor_rows(c, q.prior_tau, B, 1.0, "prior covariance", &c->d_pf[vgpa_ctx::PF_LT], &c->pf_n[vgpa_ctx::PF_LT], &Lt, &lt_diag))) return rc;
      if ((rc = buf(vgpa_ctx::PF_MU, (size_t)B * D)) || (rc = upload(c, c->d_pf[vgpa_ctx::PF_MU], q.prior_mu, (size_t)B * D))) return rc;
      f.mu0 = c->d_pf[vgpa_ctx::PF_MU]; f.Lt = c->d_pf[vgpa_ctx::PF_LT];
    }
    cur = c->d_pf[vgpa_ctx::PF_XA]; other = c->d_pf[vgpa_ctx::PF_XB];
    st_cur = carried ? c->d_pf[vgpa_ctx::PF_STA] : nullptr; st_other = carried ? c->d_pf[vgpa_ctx::PF_STB] : nullptr;
    f.x = cur; f.ws = other; f.lw = c->d_pf[vgpa_ctx::PF_LW]; f.cum = c->d_pf[vgpa_ctx::PF_CUM];
    f.anc = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_ANC]);
    f.h_ess = c->d_pf[vgpa_ctx::PF_ESS]; f.h_flag = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_FLAG]);
    f.h_anc = keep_anc ? reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_HANC]) : nullptr;
    f.h_clouds = keep_clouds ? c->d_pf[vgpa_ctx::PF_CLOUDS] : nullptr;
    f.h_lw = keep_lw ? c->d_pf[vgpa_ctx::PF_HLW] : nullptr;
    if (q.rows == Carry::Events) {      // the levels and sides: uploaded once per call, read from global memory at every segment's entry
      const size_t BD = (size_t)B * D;
      if ((rc = buf(vgpa_ctx::PF_EVC, BD)) || (rc = buf(vgpa_ctx::PF_EVS, ints(BD))) || (q.cdf && (rc = buf(vgpa_ctx::PF_CDF, (size_t)B * n_keep * D)))) return rc;
      int32_t* d_side = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_EVS]);
      if ((rc = upload(c, c->d_pf[vgpa_ctx::PF_EVC], q.levels, BD)) || (rc = upload(c, d_side, q.sides, BD))) return rc;
      own.ev_level = c->d_pf[vgpa_ctx::PF_EVC]; own.ev_side = d_side;
    }
    if (pinned) {      // the reference trajectories: uploaded once per call, read from global memory by the walk and the steps
      const size_t n_ref = (size_t)B * c->Np * D;
      if ((rc = buf(vgpa_ctx::PF_REF, n_ref)) || (rc = upload(c, c->d_pf[vgpa_ctx::PF_REF], q.ref, n_ref))) return rc;
      f.ref = own.pf_ref = c->d_pf[vgpa_ctx::PF_REF]; f.Np = c->Np;
    }
    // the cuts: the observation indices the kernels will see (each problem's own row and count in force), and the last grid index
    is_obs.assign((size_t)c->Np, 0);
    count.assign((size_t)B, M);
    const bool own_t = c->in.obs_t.stride != 0;
    for (int p = 0; p < B; p++) {
      if (!c->h_nobs.empty()) count[p] = c->h_nobs[p];
      const int64_t* t = own_t ? c->h_pp_obs_t.data() + (size_t)p * M : c->h_obs_t.data();
      for (int m = 0; m < count[p]; m++) is_obs[(size_t)t[m]] = 1;
    }
    return VGPA_OK;
  }

  // The filter: the start, then the segments with the resampling step between them.  with_stats: the same walk, counters
  // and resampling decisions, every slot's [3][D] row of path statistics carried along its lineage.  events: with_stats
  // with the rows of event records, which start from the particles' states at grid index 0 and not from zero.
  int filter() {
    const size_t n = (size_t)q.n_paths, BM = (size_t)c->B * f.M;
    HIP_TRY(c, hipMemsetAsync(f.h_ess, 0, BM * sizeof(double), c->stream));
    HIP_TRY(c, hipMemsetAsync(f.h_flag, 0, BM * sizeof(int32_t), c->stream));
    if (f.h_anc) HIP_TRY(c, hipMemsetAsync(f.h_anc, 0xff, BM * n * sizeof(int32_t), c->stream));      // (-1 beyond a problem's own count)
    LAUNCH_TRY(c, "particle start launch", launch_pf_start(f, c->stream));
    if (pinned) LAUNCH_TRY(c, "pinned start launch", launch_pf_pin(f, c->stream));
    a.pf_lw = f.lw; a.seg_first = 1; a.pf_stats = st_cur;
    if (pinned)      // (the segment with slot 0 pinned, the step with ancestor sampling)
      return cuts(segment, "conditional segment launch", a, "conditional resampling launch", [&](int k) {
        f.k = k; f.last = k == c->Np - 1 ? 1 : 0; f.x_in = cur; f.x_out = other;
        return launch_pf_cresample(f, a, c->stream);
      }, own);
    if (q.rows == Carry::Events) LAUNCH_TRY(c, "event start rows launch", launch_pf_events_start(c->D, c->B, q.n_paths, c->Np, cur, own.ev_level, own.ev_side, st_cur, c->stream));
    else if (q.rows == Carry::Stats) HIP_TRY(c, hipMemsetAsync(st_cur, 0, 3 * (size_t)c->B * n * c->D * sizeof(double), c->stream));
    return cuts(segment, "particle segment launch", a, "particle resampling launch", [&](int k) {
      f.k = k; f.last = k == c->Np - 1 ? 1 : 0; f.x_in = cur; f.x_out = other; f.st_in = st_cur; f.st_out = st_other;
      std::swap(st_cur, st_other);      // (the next segment carries the rows the step is about to write)
      a.pf_stats = st_cur;
      return launch_pf_resample(f, c->stream);
    }, own);
  }

  // The smoothing moments, behind the filter, whose ancestor history stays on the device: the descendant weights, then
  // the walk once more from the same counters (the stored ancestors in place of the resampling decisions) with the weighted sums taken at
  // every stride-th grid index, their sum over the workgroups, the downloads; `state` is then what the replay arrived at.
  // The covariance request is the same pass with Walk::ReplayCov: the sums are the mean and the packed lower triangle,
  // which one more launch spreads to mean [D] and second [D][D] before they leave.
  int moments() {
    const int B = c->B, M = c->M;
    int rc;
    double* wtab = c->d_pf[vgpa_ctx::PF_WTAB];
    double* less = c->d_pf[vgpa_ctx::PF_LESS];
    if (q.smoothed()) HIP_TRY(c, hipMemsetAsync(wtab, 0, (size_t)B * rows * q.n_paths * sizeof(double), c->stream));      // (the rows beyond a problem's own count + 1)
    HIP_TRY(c, hipMemsetAsync(less, 0, (size_t)B * rows * sizeof(double), c->stream));
    LAUNCH_TRY(c, "descendant weights launch", launch_pf_descend(f, rows, wtab, less, c->stream));
    if (q.smoothed() && (rc = backward_weights(wtab, less))) return rc;
    // the replay: the start and the segments once more; the start's log-weights go to the prefix sums' buffer, which nothing reads any more
    cur = c->d_pf[vgpa_ctx::PF_XA]; other = c->d_pf[vgpa_ctx::PF_XB];
    PfArgs g = f;
    g.x = cur; g.ws = other; g.lw = c->d_pf[vgpa_ctx::PF_CUM]; g.st_in = nullptr; g.st_out = nullptr;
    LAUNCH_TRY(c, "particle start launch", launch_pf_start(g, c->stream));
    SampleArgs w = a;
    w.stride = q.stride; w.n_keep = n_keep; w.seg_first = 1; w.pf_stats = nullptr;
    w.pf_wtab = wtab; w.pf_part = c->d_pf[vgpa_ctx::PF_PART]; w.pf_rows = rows;
    const bool covariance = q.behind == Behind::Covariance;
    if ((rc = cuts(covariance ? Walk::ReplayCov : Walk::Replay, "replay segment launch", w, "replay gather launch", [&](int k) {
          g.k = k; g.x_in = cur; g.x_out = other;
          return launch_pf_gather(g, c->stream);
        }))) return rc;
    LAUNCH_TRY(c, "moments sum launch", launch_pf_moments_sum(B, n_blocks, mom_len, w.pf_part, c->d_pf[vgpa_ctx::PF_MOM], c->stream));
    if (covariance) {
      const size_t kept = (size_t)B * n_keep, n_mean = kept * c->D;
      double* d_mean = c->d_pf[vgpa_ctx::PF_COV];
      LAUNCH_TRY(c, "covariance unpack launch", launch_pf_cov_unpack(c->D, kept, c->d_pf[vgpa_ctx::PF_MOM], d_mean, d_mean + n_mean, c->stream));
      if ((rc = download(c, q.cov_mean, d_mean, n_mean)) || (rc = download(c, q.cov_second, d_mean + n_mean, n_mean * c->D))) return rc;
    } else if ((rc = download(c, q.moments, c->d_pf[vgpa_ctx::PF_MOM], (size_t)B * mom_len))) return rc;
    if (q.lineage_ess)      // (the device's rows are M1 + 1 = M + 1, but for a context of capacity 0)
      for (int p = 0; p < (rows == M + 1 ? 1 : B); p++)
        if ((rc = download(c, q.lineage_ess + (size_t)p * (M + 1), less + (size_t)p * rows, rows == M + 1 ? (size_t)B * rows : (size_t)M + 1))) return rc;
    return VGPA_OK;
  }

  // The smoothing weights of the marginal backward smoother in the descendant weights' place: row c and its ESS are
  // launch_pf_descend's, which moments() has just run; the union of the batch's cuts is walked backwards, one launch_smooth_cut per cut --
  // every problem looks up its own observation there and copies or recurses by its own flag --, then the ESS of the rows below c.  The
  // table leaves here where it is asked for; the replay behind it is moments()' own.
  int backward_weights(double* wtab, double* less) {
    const int B = c->B, M = c->M;
    const size_t Bn = (size_t)B * q.n_paths;
    int rc;
    SmoothArgs sm{};
    sm.rows = rows; sm.xt = c->d_pf[vgpa_ctx::PF_SMX]; sm.rmax = c->d_pf[vgpa_ctx::PF_SMR]; sm.rsum = sm.rmax + Bn; sm.centre = sm.rsum + Bn;
    sm.wtab = wtab; sm.part = c->d_pf[vgpa_ctx::PF_SMP]; sm.less = less;
    PfArgs g = f;
    for (int k = c->Np - 1; k >= 0; k--) {
      if (!is_obs[k]) continue;
      g.k = k;
      LAUNCH_TRY(c, "backward smoothing launch", launch_smooth_cut(g, a, sm, c->stream));
    }
    LAUNCH_TRY(c, "smoothing ESS launch", launch_smooth_ess(g, sm, c->stream));
    if (q.smooth_weights)      // (the device's rows are M1 + 1 = M + 1, but for a context of capacity 0)
      for (int p = 0; p < (rows == M + 1 ? 1 : B); p++)
        if ((rc = download(c, q.smooth_weights + (size_t)p * (M + 1) * q.n_paths, wtab + (size_t)p * rows * q.n_paths,
                           (rows == M + 1 ? (size_t)B * rows : (size_t)M + 1) * q.n_paths))) return rc;
    return VGPA_OK;
  }

  // The smoothing marginals, behind the filter: the descendant weights of moments() -- its lineage ESS is this call's --,
  // their final row as integers, the integer recursion through the same ancestors, the masses zeroed, then the replay with
  // Walk::ReplayMarginals, which adds every slot's integer weight to the bin of each of its components at every kept grid index.
  int marginals() {
    const int B = c->B, M = c->M, L = q.n_levels;
    int rc;
    double* wtab = c->d_pf[vgpa_ctx::PF_WTAB];
    double* less = c->d_pf[vgpa_ctx::PF_LESS];
    uint64_t* qtab = reinterpret_cast<uint64_t*>(c->d_pf[vgpa_ctx::PF_QTAB]);
    uint64_t* qfin = reinterpret_cast<uint64_t*>(c->d_pf[vgpa_ctx::PF_QFIN]);
    unsigned long long* mass = reinterpret_cast<unsigned long long*>(c->d_pf[vgpa_ctx::PF_MASS]);
    const size_t n_mass = (size_t)B * n_keep * c->D * ((size_t)L + 1);
    if ((rc = upload(c, c->d_pf[vgpa_ctx::PF_MGL], q.mg_levels, (size_t)B * c->D * L))) return rc;
    HIP_TRY(c, hipMemsetAsync(less, 0, (size_t)B * rows * sizeof(double), c->stream));
    LAUNCH_TRY(c, "descendant weights launch", launch_pf_descend(f, rows, wtab, less, c->stream));
    LAUNCH_TRY(c, "weight quantisation launch", launch_pf_quantise(f, rows, wtab, qtab, qfin, c->stream));
    LAUNCH_TRY(c, "integer descendant weights launch", launch_pf_descend_q(f, rows, qtab, c->stream));
    HIP_TRY(c, hipMemsetAsync(mass, 0, n_mass * sizeof(uint64_t), c->stream));
    cur = c->d_pf[vgpa_ctx::PF_XA]; other = c->d_pf[vgpa_ctx::PF_XB];
    PfArgs g = f;
    g.x = cur; g.ws = other; g.lw = c->d_pf[vgpa_ctx::PF_CUM]; g.st_in = nullptr; g.st_out = nullptr;
    LAUNCH_TRY(c, "particle start launch", launch_pf_start(g, c->stream));
    SampleArgs w = a;
    w.stride = q.stride; w.n_keep = n_keep; w.seg_first = 1; w.pf_stats = nullptr; w.pf_rows = rows;
    const MarginalArgs mg{c->d_pf[vgpa_ctx::PF_MGL], L, qtab, mass};
    WalkOwn replay_own;
    replay_own.mg = &mg;
    if ((rc = cuts(Walk::ReplayMarginals, "marginals replay launch", w, "replay gather launch", [&](int k) {
          g.k = k; g.x_in = cur; g.x_out = other;
          return launch_pf_gather(g, c->stream);
        }, replay_own))) return rc;
    if ((rc = download(c, q.mass, reinterpret_cast<const uint64_t*>(mass), n_mass))) return rc;
    if (q.qfinal && (rc = download(c, q.qfinal, reinterpret_cast<const uint64_t*>(qfin), (size_t)B * q.n_paths))) return rc;
    if (q.lineage_ess)      // (as in moments())
      for (int p = 0; p < (rows == M + 1 ? 1 : B); p++)
        if ((rc = download(c, q.lineage_ess + (size_t)p * (M + 1), less + (size_t)p * rows, rows == M + 1 ? (size_t)B * rows : (size_t)M + 1))) return rc;
    return VGPA_OK;
  }

  // The two-time moments of the lineages, behind the filter: the identity slot table, its
  // trace through the ancestors, the lineage walk of all n_paths trajectories into d_sp_out -- Behind::Trajectories' steps, the paths staying
  // on the device --, the normalised final weights, the descendant weights for the lineage ESS as in moments(), then the contraction.
  int lag_covariance() {
    const int B = c->B, M = c->M;
    int rc;
    int32_t* table = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_SLOTS]);
    std::vector<int32_t> every((size_t)B * q.n_paths);      // (final_slots() is done with it when it returns)
    for (size_t e = 0; e < every.size(); e++) every[e] = (int32_t)(e % (size_t)q.n_paths);
    if ((rc = final_slots(table, every.data()))) return rc;
    LAUNCH_TRY(c, "genealogy launch", launch_pf_trace(f, q.n_draw, slot_rows, table, c->stream));
    if ((rc = walk_lanes(Walk::Lineage, "lineage walk launch", table))) return rc;
    double* wtab = c->d_pf[vgpa_ctx::PF_WTAB];
    double* wfin = wtab + (size_t)B * rows * q.n_paths;
    double* less = c->d_pf[vgpa_ctx::PF_LESS];
    LAUNCH_TRY(c, "final weights launch", launch_pf_normalise(B, q.n_paths, f.lw, wfin, c->stream));
    HIP_TRY(c, hipMemsetAsync(less, 0, (size_t)B * rows * sizeof(double), c->stream));
    LAUNCH_TRY(c, "descendant weights launch", launch_pf_descend(f, rows, wtab, less, c->stream));
    if ((rc = cross_moments(c, c->d_sp_out, wfin, q.n_paths, n_keep, q.n_anchor, q.anchor_rows, q.lag_mean, q.lag_cross))) return rc;
    if (q.lineage_ess)      // (as in moments())
      for (int p = 0; p < (rows == M + 1 ? 1 : B); p++)
        if ((rc = download(c, q.lineage_ess + (size_t)p * (M + 1), less + (size_t)p * rows, rows == M + 1 ? (size_t)B * rows : (size_t)M + 1))) return rc;
    return VGPA_OK;
  }

  // The trajectories behind the filter, whose histories stay on the device: the final slots of n_draw trajectories (final_slots, or drawn
  // from the final weights), the table of their slots in every stretch made in one launch, one launch of the walk over the n_draw
  // trajectories alone, the downloads.
  //   Behind::Trajectories: the table traced back through the ancestors, the lineage walk.
  //   Behind::Backward (s.4.17): the table drawn backwards through the clouds and the replaced log-weights, the backward walk.
  //   Behind::Conditional (s.4.18): the table traced (slot 0's ancestors are the ancestor-sampled ones), the backward walk on this run's
  //   histories -- it goes on from the true particle, the reference's where the ancestor is slot 0, behind every observation --, and the
  //   stretches spent in slot 0, where that walk drew with slot 0's counters, overwritten with the reference before the download.
  int trajectories() {
    int rc;
    int32_t* table = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_SLOTS]);
    if ((rc = final_slots(table, q.final_slots))) return rc;
    if (q.behind == Behind::Backward) LAUNCH_TRY(c, "backward simulation launch", launch_pf_backward(f, a, q.n_draw, slot_rows, table, c->stream));
    else LAUNCH_TRY(c, "genealogy launch", launch_pf_trace(f, q.n_draw, slot_rows, table, c->stream));
    if (q.behind == Behind::Trajectories) return walk_table(Walk::Lineage, "lineage walk launch", table);
    return walk_table(Walk::Backward, "backward walk launch", table);
  }

  // row c of the slot table: the given final slots [B][n_draw], or (nullptr) drawn from the final weights; every other row -1
  int final_slots(int32_t* table, const int32_t* given) {
    const int B = c->B, n_draw = q.n_draw;
    int rc;
    if (given) {                     // rows beyond a problem's own count: -1; row c: the caller's slots
      std::vector<int32_t> h_table(n_table, -1);      // (the table as it is uploaded, alive until the stream has been synchronised)
      for (int p = 0; p < B; p++)
        for (int m = 0; m < n_draw; m++) h_table[((size_t)p * slot_rows + count[p]) * n_draw + m] = given[(size_t)p * n_draw + m];
      if ((rc = upload(c, table, h_table.data(), n_table))) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
      HIP_TRY(c, hipMemsetAsync(table, 0xff, n_table * sizeof(int32_t), c->stream));
      LAUNCH_TRY(c, "final slots launch", launch_pf_pick(f, c->Np, n_draw, slot_rows, table, c->stream));
    }
    return VGPA_OK;
  }

  // the walk of the table's n_draw trajectories alone, into d_sp_out
  int walk_lanes(Walk walk, const char* what, int32_t* table) {
    SampleArgs w = a;                // the unweighted walk of n_draw lanes per problem from the same start, factors and counters
    w.n_paths = q.n_draw; w.stride = q.stride; w.n_keep = n_keep; w.out = c->d_sp_out;
    w.pf_x = nullptr; w.pf_lw = nullptr; w.pf_stats = nullptr; w.pf_slots = table; w.pf_slot_rows = slot_rows;
    if (walk == Walk::Backward) { w.pf_clouds = f.h_clouds; w.pf_hanc = f.h_anc; w.pf_M = f.M; w.pf_n = q.n_paths; }
    hipError_t e = launch_sample_walk(walk, w, c->stream);
    if (e != hipSuccess) return fail(c, VGPA_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
    return VGPA_OK;
  }

  // ... and the downloads
  int walk_table(Walk walk, const char* what, int32_t* table) {
    int rc;
    if ((rc = walk_lanes(walk, what, table))) return rc;
    if (pinned) LAUNCH_TRY(c, "reference stretches launch", launch_pf_ref_fill(f, slot_rows, table, c->d_sp_out, c->stream));
    if ((rc = download(c, q.paths, c->d_sp_out, n_traj))) return rc;
    if (q.slots_out) HIP_TRY(c, hipMemcpyAsync(q.slots_out, table, n_table * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return VGPA_OK;
  }

  // The forecast from a given cloud in place of setup() and filter(): of the kernels' arguments the model's -- the factors
  // of Sigma dt and theta in force --, the cloud and its log-weights (none given: equal) uploaded to where the filter would have left them.
  // No x, no observation and nothing of the cached state is read or written.
  int given_cloud() {
    const int D = c->D, B = c->B;
    int rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    a = SampleArgs{};
    a.model = c->cfg.model; a.D = D; a.Np = c->Np; a.batch = B; a.n_paths = q.n_paths; a.dt = c->cfg.dt; a.seed = q.seed;
    if ((rc = factor_noise(c, &a))) return rc;
    if (!a.R_diag) return fail(c, VGPA_ERR_UNSUPPORTED, "the particle forecast is built for a diagonal Sigma (a dense Sigma is in force)");
    copy_theta(c, a.theta);
    a.theta_v = c->in.theta.rows;
    const size_t Bn = (size_t)B * q.n_paths;
    if ((rc = buf(vgpa_ctx::PF_XA, Bn * D)) || (rc = buf(vgpa_ctx::PF_LW, Bn)) || (rc = buf(vgpa_ctx::PF_CUM, Bn))) return rc;
    f = PfArgs{};
    f.D = D; f.batch = B; f.n_paths = q.n_paths; f.M = 1; f.seed = q.seed;
    cur = c->d_pf[vgpa_ctx::PF_XA]; other = nullptr; st_cur = nullptr; st_other = nullptr;
    f.lw = c->d_pf[vgpa_ctx::PF_LW]; f.cum = c->d_pf[vgpa_ctx::PF_CUM];
    if ((rc = upload(c, cur, q.cloud, Bn * D))) return rc;
    if (q.cloud_logw) { if ((rc = upload(c, f.lw, q.cloud_logw, Bn))) return rc; }
    else HIP_TRY(c, hipMemsetAsync(f.lw, 0, Bn * sizeof(double), c->stream));
    k0 = q.index0;
    return VGPA_OK;
  }

  // The forecast behind the filter or behind given_cloud(): the particles in `cur` at grid index k0 with the log-weights
  // f.lw.  The n_draw members first -- their slots (final_slots, or drawn from the weights as trajectories() draws them, the uniform from
  // grid index k0 + 1), one launch of the forecast walk over them alone --, then the walk of the whole cloud with the weighted sums at every
  // stride-th step, which leaves the cloud of k0 + horizon in `cur`; the sum over the workgroups, the downloads.
  int forecast() {
    const int D = c->D, B = c->B, n_draw = q.n_draw, h_keep = q.horizon / q.stride + 1;
    const size_t n = (size_t)q.n_paths, n_slots = (size_t)B * n_draw, n_mem = n_slots * h_keep * D, len = (size_t)h_keep * 2 * D;
    const int blocks = sample_segment_blocks(D, q.n_paths);
    int rc;
    if ((rc = buf(vgpa_ctx::PF_WTAB, (size_t)B * n)) || (rc = buf(vgpa_ctx::PF_PART, (size_t)B * blocks * len)) || (rc = buf(vgpa_ctx::PF_MOM, (size_t)B * len))) return rc;
    SampleArgs w = SampleArgs{};      // the model's walk: of the filter's arguments the factors and theta
    w.kind = VGPA_PATHS_MODEL; w.model = a.model; w.D = D; w.Np = a.Np; w.batch = B; w.dt = a.dt; w.seed = q.seed;
    w.R = a.R; w.R_stride = a.R_stride; w.R_diag = a.R_diag; w.theta_v = a.theta_v;
    for (int i = 0; i < kMaxTheta; i++) w.theta[i] = a.theta[i];
    w.stride = q.stride; w.n_keep = h_keep; w.k_begin = k0; w.k_end = k0 + q.horizon; w.pf_x = cur; w.pf_n = q.n_paths;
    if (n_draw > 0) {
      if ((rc = buf(vgpa_ctx::PF_SLOTS, (n_slots + 1) / 2)) || (rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_mem))) return rc;
      int32_t* table = reinterpret_cast<int32_t*>(c->d_pf[vgpa_ctx::PF_SLOTS]);
      if (q.final_slots) {
        if ((rc = upload(c, table, q.final_slots, n_slots))) return rc;
      } else {
        PfArgs g = f;      // (one row: the table of a problem without observations)
        g.n_obs = 0; g.n_obs_v = nullptr;
        LAUNCH_TRY(c, "forecast slots launch", launch_pf_pick(g, k0 + 1, n_draw, 1, table, c->stream));
      }
      SampleArgs m = w;
      m.n_paths = n_draw; m.out = c->d_sp_out; m.pf_slots = table; m.pf_slot_rows = 1;
      LAUNCH_TRY(c, "forecast members launch", launch_sample_walk(Walk::Forecast, m, c->stream));
      if (q.members && (rc = download(c, q.members, c->d_sp_out, n_mem))) return rc;
      if (q.slots_out) HIP_TRY(c, hipMemcpyAsync(q.slots_out, table, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    LAUNCH_TRY(c, "forecast weights launch", launch_pf_normalise(B, q.n_paths, f.lw, c->d_pf[vgpa_ctx::PF_WTAB], c->stream));
    w.n_paths = q.n_paths; w.pf_wtab = c->d_pf[vgpa_ctx::PF_WTAB]; w.pf_part = c->d_pf[vgpa_ctx::PF_PART];
    LAUNCH_TRY(c, "forecast launch", launch_sample_walk(Walk::Forecast, w, c->stream));
    LAUNCH_TRY(c, "moments sum launch", launch_pf_moments_sum(B, blocks, len, w.pf_part, c->d_pf[vgpa_ctx::PF_MOM], c->stream));
    if ((rc = download(c, q.fc_moments, c->d_pf[vgpa_ctx::PF_MOM], (size_t)B * len))) return rc;
    if (q.state_end && (rc = download(c, q.state_end, cur, (size_t)B * n * D))) return rc;
    return VGPA_OK;
  }
};

// Two limits the smoothers and the forecast share, in the caller's nouns.  check_sums: k_pf_moments_sum takes [B][kept][2][D] in one launch;
// check_stored: k lanes per problem stored as vgpa_sample_paths stores them, [B][k][kept][D], are at most 2^35 entries
static int check_sums(vgpa_ctx* c, int kept, const char* what, const char* points) {
  if (pf_flat_grid_fits((size_t)c->B * ((size_t)kept * 2 * c->D))) return VGPA_OK;
  return fail(c, VGPA_ERR_UNSUPPORTED, "the %s moments are built for at most 2^39 entries (batch %d, %d kept %s, D = %d): use a larger stride",
              what, c->B, kept, points, c->D);
}
static int check_stored(vgpa_ctx* c, int k, int kept, const char* what, const char* lanes, const char* points) {
  if ((double)c->B * (double)k * (double)kept * (double)c->D <= 34359738368.0) return VGPA_OK;
  return fail(c, VGPA_ERR_UNSUPPORTED, "the %s are built for at most 2^35 entries (batch %d, %d %s, %d kept %s, D = %d): use a larger stride",
              what, c->B, k, lanes, kept, points, c->D);
}

static int particle_run(vgpa_ctx* c, const ParticleRequest& q) {
  if (!c) return VGPA_ERR_ARG;
  if (!q.logw || !q.state) return fail(c, VGPA_ERR_ARG, "null argument");
  if (q.stride < 1) return fail(c, VGPA_ERR_ARG, "stride must be at least 1 (stride = %d)", q.stride);
  if (q.rows == Carry::Stats && !q.stats && !q.mean) return fail(c, VGPA_ERR_ARG, "at least one of stats and mean must be given");
  const int32_t n_paths = q.n_paths, n_draw = q.n_draw, stride = q.stride;
  if (n_paths < 1) return fail(c, VGPA_ERR_ARG, "n_paths must be at least 1 (n_paths = %d)", n_paths);
  int rc;
  if (q.table() && q.final_slots && (rc = check_slots(c, q.final_slots, n_draw, n_paths, "final slot", "trajectory"))) return rc;
  if (!(q.ess_fraction >= 0.0 && q.ess_fraction <= 1.0)) return fail(c, VGPA_ERR_ARG, "ess_fraction must lie in [0, 1] (ess_fraction = %g)", q.ess_fraction);
  if ((q.prior_mu == nullptr) != (q.prior_tau == nullptr)) return fail(c, VGPA_ERR_ARG, "the prior is a mean and a covariance: both or neither");
  if (c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_ARG, "context has no stochastic model: no model SDE to weigh the particles against");
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  const int D = c->D, B = c->B, M = c->M, Np = c->Np;
  const int kept = (Np - 1) / stride + 1;
  const bool moments = q.behind == Behind::Moments || q.smoothed(), covariance = q.behind == Behind::Covariance, carried = q.rows != Carry::None;
  if (D <= kMaxSmallD) {      // the launch limits and the sizes of the results, before any work
    if (q.sums() && n_paths > sample_max_paths(D))      // (the replay)
      return fail(c, VGPA_ERR_UNSUPPORTED, "the smoothing %s are built for at most %d particles per problem at D = %d (n_paths = %d)",
                  moments ? "moments" : "covariances", sample_max_paths(D), D, n_paths);
    if (moments && (rc = check_sums(c, kept, "smoothing", "grid indices"))) return rc;
    if (q.smoothed() && !smooth_grid_fits(D, n_paths))      // (the launches of one cut: the successors, the row pass)
      return fail(c, VGPA_ERR_UNSUPPORTED, "backward smoothing is built for at most %d particles per problem at D = %d (n_paths = %d)",
                  std::min(kMaxGridY * kSmoothRowBlock, kMaxGridY * 256 / D), D, n_paths);
    // (the sum of the covariance replay's packed partial sums and the unpacking launch)
    if (covariance && !(pf_flat_grid_fits((size_t)B * kept * D * D) && pf_flat_grid_fits((size_t)B * kept * sample_cov_len(D))))
      return fail(c, VGPA_ERR_UNSUPPORTED, "the smoothing covariances are built for at most 2^39 - 256 entries (batch %d, %d kept grid indices, D = %d): use a larger stride",
                  B, kept, D);
    if (q.behind == Behind::Marginals) {      // (the replay; one launch-sized array of masses)
      if (n_paths > sample_max_paths(D))
        return fail(c, VGPA_ERR_UNSUPPORTED, "the smoothing marginals are built for at most %d particles per problem at D = %d (n_paths = %d)", sample_max_paths(D), D, n_paths);
      if (!pf_flat_grid_fits((size_t)B * kept * D * ((size_t)q.n_levels + 1)))
        return fail(c, VGPA_ERR_UNSUPPORTED, "the smoothing marginals are built for at most 2^39 - 256 entries of mass (batch %d, %d kept grid indices, D = %d, %d levels): use a larger stride",
                    B, kept, D, q.n_levels);
    }
    if (q.lag()) {      // (the trajectories' own limits with n_paths of them, then the contraction's)
      if (!sample_lineages_fit(D, B, n_paths))
        return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariance walks every particle's trajectory, at most %d per problem at D = %d (n_paths = %d)", sample_max_paths(kMaxSmallD), D, n_paths);
      if ((rc = check_stored(c, n_paths, kept, "lag covariance's trajectories", "particles", "grid indices"))) return rc;
      if (!path_moments_grid_fits(D, B, kept, q.n_anchor))
        return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariance is built for at most %d anchors and a batch of at most %d (batch %d, %d anchors, %d kept grid indices)",
                    kMaxGridY, kMaxGridY, B, q.n_anchor, kept);
      if (!cross_moments_fit(B, kept, D, q.n_anchor))
        return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariance is built for at most 2^39 - 256 entries of cross (batch %d, %d anchors, %d kept grid indices, D = %d): "
                    "use a larger stride or fewer anchors", B, q.n_anchor, kept, D);
    }
    if (q.table() && !sample_lineages_fit(D, B, n_draw))      // (the lineage walk; the number is the matrix-core walk's, above D = 4)
      return fail(c, VGPA_ERR_UNSUPPORTED, "the smoothing trajectories are built for at most %d per problem at D = %d (n_draw = %d)", sample_max_paths(kMaxSmallD), D, n_draw);
    if (q.behind == Behind::Backward && !pf_backward_fits(n_draw))      // (the one launch of the backward simulation)
      return fail(c, VGPA_ERR_UNSUPPORTED, "backward simulation is built for at most %d trajectories per problem (n_draw = %d)", kMaxGridY * kBackwardBlock, n_draw);
    if (q.table() && (rc = check_stored(c, n_draw, kept, "smoothing trajectories", "trajectories", "grid indices"))) return rc;
  }
  c->pf_hlw_paths = 0;      // (the histories of the call before are about to be overwritten)
  ParticleRun r{c, q};
  if ((rc = r.setup()) || (rc = r.filter()) || (q.sums() && (rc = r.moments())) || (q.behind == Behind::Marginals && (rc = r.marginals())) ||
      (q.lag() && (rc = r.lag_covariance())) || (q.table() && (rc = r.trajectories()))) return rc;
  const size_t n = (size_t)n_paths, BnD = (size_t)B * n * D;
  if (q.fc_moments) {      // (the filter's final cloud leaves before the forecast carries it on in place)
    if ((rc = download(c, q.state, r.cur, BnD))) return rc;
    r.k0 = Np - 1;
    if ((rc = r.forecast())) return rc;
  }
  if (carried && q.mean) {
    LAUNCH_TRY(c, "path statistics mean launch", launch_pf_stats_mean(D, B, n_paths, r.f.lw, r.st_cur, c->d_pf[vgpa_ctx::PF_MEAN], c->stream));
    if ((rc = download(c, q.mean, c->d_pf[vgpa_ctx::PF_MEAN], (size_t)B * 3 * D))) return rc;
  }
  if (carried && q.stats && (rc = download(c, q.stats, r.st_cur, 3 * BnD))) return rc;
  if (q.rows == Carry::Events && q.cdf) {
    LAUNCH_TRY(c, "first-passage distribution launch", launch_pf_events_cdf(D, B, n_paths, Np, stride, r.f.lw, r.st_cur, c->d_pf[vgpa_ctx::PF_CDF], c->stream));
    if ((rc = download(c, q.cdf, c->d_pf[vgpa_ctx::PF_CDF], (size_t)B * kept * D))) return rc;
  }
  if ((rc = download(c, q.logw, r.f.lw, (size_t)B * n)) || (!q.fc_moments && (rc = download(c, q.state, r.cur, BnD)))) return rc;
  if (q.ess && (rc = download(c, q.ess, r.f.h_ess, (size_t)B * M))) return rc;
  if (q.resampled && M > 0) HIP_TRY(c, hipMemcpyAsync(q.resampled, r.f.h_flag, (size_t)B * M * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (q.ancestors && M > 0) HIP_TRY(c, hipMemcpyAsync(q.ancestors, r.f.h_anc, (size_t)B * M * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (q.clouds)      // (only the rows below a problem's own count: the rest of the caller's array stays as it is)
    for (int p = 0; p < B; p++)
      if (r.count[p] > 0 && (rc = download(c, q.clouds + (size_t)p * M * n * D, r.f.h_clouds + (size_t)p * M * n * D, (size_t)r.count[p] * n * D))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (r.keep_lw) c->pf_hlw_paths = n_paths;
  return VGPA_OK;
}

// The log-weights the resamplings of the last backward call replaced, as its kernels read them (see vgpa_hip.h)
int vgpa_particle_replaced_logw(vgpa_ctx* c, int32_t n_paths, double* hlw) {
  if (!c) return VGPA_ERR_ARG;
  if (!hlw) return fail(c, VGPA_ERR_ARG, "null argument");
  if (c->pf_hlw_paths == 0 || c->pf_hlw_paths != n_paths)
    return fail(c, VGPA_ERR_STATE, "the last particle call kept no replaced log-weights of %d particles: call vgpa_particle_backward_paths or "
                "vgpa_particle_backward_moments first", n_paths);
  const size_t B = (size_t)c->B, M = (size_t)c->M, n = (size_t)n_paths;
  if (M == 0) return VGPA_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  std::vector<int32_t> flags(B * M);
  int rc;
  if ((rc = download(c, hlw, c->d_pf[vgpa_ctx::PF_HLW], B * M * n))) return rc;
  HIP_TRY(c, hipMemcpyAsync(flags.data(), c->d_pf[vgpa_ctx::PF_FLAG], B * M * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t e = 0; e < B * M; e++)      // (the device writes the rows of the resampled observations alone)
    if (!flags[e]) std::fill(hlw + e * n, hlw + (e + 1) * n, std::numeric_limits<double>::quiet_NaN());
  return VGPA_OK;
}

int vgpa_particle_filter(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, uint64_t seed, double ess_fraction,
                         const double* prior_mu, const double* prior_tau, double* logw, double* state, double* ess, int32_t* resampled,
                         int32_t* ancestors, double* clouds) {
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.ancestors = ancestors; q.clouds = clouds;
  return particle_run(c, q);
}

// The path statistics of the particle filter's lineages (see vgpa_hip.h)
int vgpa_particle_statistics(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, uint64_t seed, double ess_fraction,
                             const double* prior_mu, const double* prior_tau, double* logw, double* state, double* stats, double* mean,
                             double* ess, int32_t* resampled) {
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.rows = Carry::Stats; q.stats = stats; q.mean = mean;
  return particle_run(c, q);
}

// Path events of the particle filter's lineages: extremes, first passage, occupation (see vgpa_hip.h)
int vgpa_particle_events(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                         const double* prior_mu, const double* prior_tau, const double* levels, const int32_t* sides, double* logw, double* state,
                         double* rows, double* mean, double* cdf, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!levels || !sides) return fail(c, VGPA_ERR_ARG, "null argument");
  if (!rows && !mean && !cdf) return fail(c, VGPA_ERR_ARG, "at least one of rows, mean and cdf must be given");
  if (stride < 1) return fail(c, VGPA_ERR_ARG, "stride must be at least 1 (stride = %d)", stride);
  for (size_t e = 0; e < (size_t)c->B * c->D; e++) {
    if (!std::isfinite(levels[e])) return fail(c, VGPA_ERR_ARG, "levels must be finite (problem %zu, component %zu)", e / c->D, e % c->D);
    if (sides[e] != 1 && sides[e] != -1) return fail(c, VGPA_ERR_ARG, "sides must be +1 or -1 (problem %zu, component %zu: %d)", e / c->D, e % c->D, sides[e]);
  }
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.rows = Carry::Events; q.stats = rows; q.mean = mean;
  q.levels = levels; q.sides = sides; q.cdf = cdf;
  return particle_run(c, q);
}

// The smoothing moments on the grid under the particles' genealogy (see vgpa_hip.h)
int vgpa_particle_moments(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                          const double* prior_mu, const double* prior_tau, double* logw, double* state, double* moments, double* lineage_ess,
                          double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!moments) return fail(c, VGPA_ERR_ARG, "null argument");
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.behind = Behind::Moments; q.moments = moments; q.lineage_ess = lineage_ess;
  return particle_run(c, q);
}

// The smoothing moments on the grid under the marginal backward smoother's weights (see vgpa_hip.h)
int vgpa_particle_backward_moments(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                                   const double* prior_mu, const double* prior_tau, double* logw, double* state, double* moments,
                                   double* smoothing_ess, double* weights, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!moments) return fail(c, VGPA_ERR_ARG, "null argument");
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.behind = Behind::BackwardMoments; q.moments = moments; q.lineage_ess = smoothing_ess; q.smooth_weights = weights;
  return particle_run(c, q);
}

// The smoothing mean and the full second-moment matrices on the grid under the particles' genealogy (see vgpa_hip.h)
int vgpa_particle_covariance(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                             const double* prior_mu, const double* prior_tau, double* logw, double* state, double* mean, double* second,
                             double* lineage_ess, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!mean || !second) return fail(c, VGPA_ERR_ARG, "null argument");
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.behind = Behind::Covariance; q.cov_mean = mean; q.cov_second = second; q.lineage_ess = lineage_ess;
  return particle_run(c, q);
}

// The smoothing marginals on the grid as exact integer histograms over a ladder of levels (see vgpa_hip.h)
int vgpa_particle_marginals(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                            const double* prior_mu, const double* prior_tau, const double* levels, int32_t n_levels, double* logw, double* state,
                            uint64_t* mass, uint64_t* qfinal, double* lineage_ess, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!levels || !mass) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_levels < 1 || n_levels > kMaxMarginalLevels) return fail(c, VGPA_ERR_ARG, "n_levels must lie in [1, %d] (n_levels = %d)", kMaxMarginalLevels, n_levels);
  if (stride < 1) return fail(c, VGPA_ERR_ARG, "stride must be at least 1 (stride = %d)", stride);
  for (size_t e = 0; e < (size_t)c->B * c->D; e++) {
    const double* lad = levels + e * n_levels;
    for (int l = 0; l < n_levels; l++) {
      if (!std::isfinite(lad[l])) return fail(c, VGPA_ERR_ARG, "levels must be finite (problem %zu, component %zu, level %d)", e / c->D, e % c->D, l);
      if (l > 0 && !(lad[l - 1] < lad[l]))
        return fail(c, VGPA_ERR_ARG, "levels must be strictly increasing (problem %zu, component %zu, level %d)", e / c->D, e % c->D, l);
    }
  }
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.behind = Behind::Marginals; q.mg_levels = levels; q.n_levels = n_levels; q.mass = mass; q.qfinal = qfinal; q.lineage_ess = lineage_ess;
  return particle_run(c, q);
}

// The two-time moments of the particle filter's lineages against a set of anchors (see vgpa_hip.h)
int vgpa_particle_lag_covariance(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction,
                                 const double* prior_mu, const double* prior_tau, int32_t n_anchor, const int64_t* anchors, double* logw, double* state,
                                 double* mean, double* cross, double* lineage_ess, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!mean || !cross || !anchors) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_anchor < 1 || stride < 1) return fail(c, VGPA_ERR_ARG, "n_anchor and stride must be at least 1 (n_anchor = %d, stride = %d)", n_anchor, stride);
  if (n_paths < 1) return fail(c, VGPA_ERR_ARG, "n_paths must be at least 1 (n_paths = %d)", n_paths);
  std::vector<int32_t> rows((size_t)n_anchor);      // (alive until particle_run has synchronised the stream)
  for (int32_t i = 0; i < n_anchor; i++) {
    if (anchors[i] < 0 || anchors[i] >= c->Np || (i > 0 && anchors[i] <= anchors[i - 1]))
      return fail(c, VGPA_ERR_ARG, "anchor %d -> %lld: the anchors are strictly increasing grid indices in [0, %d)", i, (long long)anchors[i], c->Np);
    if (anchors[i] % stride != 0)
      return fail(c, VGPA_ERR_ARG, "anchor %d -> %lld is no multiple of the stride %d: the anchors lie on the kept grid", i, (long long)anchors[i], stride);
    rows[(size_t)i] = (int32_t)(anchors[i] / stride);
  }
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.behind = Behind::LagCovariance; q.lineage_ess = lineage_ess;
  q.n_anchor = n_anchor; q.anchor_rows = rows.data(); q.lag_mean = mean; q.lag_cross = cross;
  q.n_draw = n_paths;      // (every final slot's trajectory: the pass makes the identity table itself)
  return particle_run(c, q);
}

// The contraction of vgpa_particle_lag_covariance alone on given trajectories and weights (see vgpa_hip.h).  Reads the
// context's D and batch and nothing of the cached state; writes nothing to it.
int vgpa_path_cross_moments(vgpa_ctx* c, const double* paths, const double* weights, int32_t n_paths, int32_t n_keep, int32_t n_anchor,
                            const int32_t* anchor_rows, double* mean, double* cross) {
  if (!c) return VGPA_ERR_ARG;
  if (!paths || !anchor_rows || !mean || !cross) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_paths < 1 || n_keep < 1 || n_anchor < 1)
    return fail(c, VGPA_ERR_ARG, "n_paths, n_keep and n_anchor must be at least 1 (n_paths = %d, n_keep = %d, n_anchor = %d)", n_paths, n_keep, n_anchor);
  for (int32_t i = 0; i < n_anchor; i++)
    if (anchor_rows[i] < 0 || anchor_rows[i] >= n_keep)
      return fail(c, VGPA_ERR_ARG, "anchor row %d -> %d does not lie in [0, %d)", i, anchor_rows[i], n_keep);
  const int D = c->D, B = c->B;
  if (D > kMaxSmallD) return fail(c, VGPA_ERR_UNSUPPORTED, "the path cross moments are built for D <= %d (D = %d)", kMaxSmallD, D);
  int rc;
  if ((rc = check_stored(c, n_paths, n_keep, "paths", "paths", "rows"))) return rc;
  if (!path_moments_grid_fits(D, B, n_keep, n_anchor))
    return fail(c, VGPA_ERR_UNSUPPORTED, "the path cross moments are built for at most %d anchors and a batch of at most %d (batch %d, %d anchors, %d kept rows)",
                kMaxGridY, kMaxGridY, B, n_anchor, n_keep);
  if (!cross_moments_fit(B, n_keep, D, n_anchor))
    return fail(c, VGPA_ERR_UNSUPPORTED, "the path cross moments are built for at most 2^39 - 256 entries of cross (batch %d, %d anchors, %d kept rows, D = %d): "
                "use fewer rows or fewer anchors", B, n_anchor, n_keep, D);
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t Bn = (size_t)B * n_paths, n_traj = Bn * n_keep * D;
  if ((rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_traj)) || (weights && (rc = grow(c, &c->d_pf[vgpa_ctx::PF_WTAB], &c->pf_n[vgpa_ctx::PF_WTAB], Bn)))) return rc;
  if ((rc = upload(c, c->d_sp_out, paths, n_traj)) || (weights && (rc = upload(c, c->d_pf[vgpa_ctx::PF_WTAB], weights, Bn)))) return rc;
  if ((rc = cross_moments(c, c->d_sp_out, weights ? c->d_pf[vgpa_ctx::PF_WTAB] : nullptr, n_paths, n_keep, n_anchor, anchor_rows, mean, cross))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}

// Whole smoothing trajectories on the grid from the particles' genealogy (see vgpa_hip.h)
int vgpa_particle_paths(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t n_draw, const int32_t* final_slots, int32_t stride,
                        uint64_t seed, double ess_fraction, const double* prior_mu, const double* prior_tau, double* logw, double* state,
                        double* paths, int32_t* slots, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!paths) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_draw < 1) return fail(c, VGPA_ERR_ARG, "n_draw must be at least 1 (n_draw = %d)", n_draw);
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.n_draw = n_draw; q.final_slots = final_slots; q.paths = paths; q.slots_out = slots; q.behind = Behind::Trajectories;
  return particle_run(c, q);
}

// Whole smoothing trajectories on the grid by backward simulation through the filter's clouds (see vgpa_hip.h)
int vgpa_particle_backward_paths(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, int32_t n_draw, const int32_t* final_slots,
                                 int32_t stride, uint64_t seed, double ess_fraction, const double* prior_mu, const double* prior_tau, double* logw,
                                 double* state, double* paths, int32_t* slots, double* ess, int32_t* resampled) {
  if (!c) return VGPA_ERR_ARG;
  if (!paths) return fail(c, VGPA_ERR_ARG, "null argument");
  if (n_draw < 1) return fail(c, VGPA_ERR_ARG, "n_draw must be at least 1 (n_draw = %d)", n_draw);
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.n_draw = n_draw; q.final_slots = final_slots; q.paths = paths; q.slots_out = slots; q.behind = Behind::Backward;
  return particle_run(c, q);
}

// The conditional particle filter with ancestor sampling: one sweep of particle Gibbs (see vgpa_hip.h)
int vgpa_particle_conditional(vgpa_ctx* c, const double* x, const double* x0, const double* ref, int32_t n_paths, uint64_t seed,
                              double ess_fraction, const double* prior_mu, const double* prior_tau, double* logw, double* state,
                              double* trajectory, int32_t* slots, double* ess, int32_t* resampled, int32_t* ancestors, double* clouds) {
  if (!c) return VGPA_ERR_ARG;
  if (!ref || !trajectory) return fail(c, VGPA_ERR_ARG, "null argument");
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.ancestors = ancestors; q.clouds = clouds;
  q.n_draw = 1; q.paths = trajectory; q.slots_out = slots; q.behind = Behind::Conditional; q.ref = ref;
  return particle_run(c, q);
}

// The filtered cloud, or a given one, carried forward under the model SDE (see vgpa_hip.h)
int vgpa_particle_forecast(vgpa_ctx* c, const double* x, const double* x0, int32_t n_paths, uint64_t seed, double ess_fraction,
                           const double* prior_mu, const double* prior_tau, const double* cloud, const double* cloud_logw, int32_t index0,
                           int32_t horizon, int32_t stride, int32_t n_draw, const int32_t* final_slots, double* logw, double* state, double* ess,
                           int32_t* resampled, double* moments, double* members, int32_t* slots, double* state_end) {
  if (!c) return VGPA_ERR_ARG;
  if (!moments) return fail(c, VGPA_ERR_ARG, "null argument");
  if (c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_ARG, "context has no stochastic model: no model SDE to carry the particles forward");
  if (horizon < 0 || stride < 1) return fail(c, VGPA_ERR_ARG, "horizon must be at least 0 and stride at least 1 (horizon = %d, stride = %d)", horizon, stride);
  if (n_draw < 0) return fail(c, VGPA_ERR_ARG, "n_draw must be at least 0 (n_draw = %d)", n_draw);
  if (n_paths < 1) return fail(c, VGPA_ERR_ARG, "n_paths must be at least 1 (n_paths = %d)", n_paths);
  if (cloud && index0 < 0) return fail(c, VGPA_ERR_ARG, "index0 must be at least 0 (index0 = %d)", index0);
  const int D = c->D;
  const int64_t k0 = cloud ? (int64_t)index0 : (int64_t)c->Np - 1;
  // (the uniform of drawn slots comes from grid index k0 + 1, which must be one as well)
  if (k0 + (int64_t)horizon > 0x7fffffffLL || (n_draw > 0 && !final_slots && k0 + 1 > 0x7fffffffLL))
    return fail(c, VGPA_ERR_ARG, "the forecast ends beyond grid index 2^31 - 1 (it starts at %lld, horizon = %d)", (long long)k0, horizon);
  int rc;
  if (n_draw > 0 && final_slots && (rc = check_slots(c, final_slots, n_draw, n_paths, "slot", "member"))) return rc;
  if (D > kMaxSmallD) return fail(c, VGPA_ERR_UNSUPPORTED, "the particle forecast is built for D <= %d (D = %d)", kMaxSmallD, D);
  const int h_keep = horizon / stride + 1;      // the launch limits of the two walks and of the final sum, the size of the members: before any work
  if (n_paths > sample_max_paths(D) || n_draw > sample_max_paths(D))
    return fail(c, VGPA_ERR_UNSUPPORTED, "the particle forecast is built for at most %d particles and members per problem at D = %d (n_paths = %d, n_draw = %d)",
                sample_max_paths(D), D, n_paths, n_draw);
  if ((rc = check_sums(c, h_keep, "forecast", "steps")) || (rc = check_stored(c, n_draw, h_keep, "forecast members", "members", "steps"))) return rc;
  ParticleRequest q{x, x0, n_paths, seed, ess_fraction, prior_mu, prior_tau, logw, state, ess, resampled};
  q.stride = stride; q.n_draw = n_draw; q.final_slots = final_slots; q.slots_out = slots;
  q.horizon = horizon; q.cloud = cloud; q.cloud_logw = cloud_logw; q.index0 = index0;
  q.fc_moments = moments; q.members = members; q.state_end = state_end;
  if (!cloud) return particle_run(c, q);
  ParticleRun r{c, q};      // a given cloud: no filter runs
  if ((rc = r.given_cloud()) || (rc = r.forecast())) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}

// The two-time covariance K(k, s) = Phi(k, s) S_s of the posterior process, or the propagator Phi(k, s) itself, from every anchor s to the
// end of the grid (see vgpa_hip.h; lag_cov.hip).  Reads x and, for the covariance, the resident S_t in the layout it is
// in; of the cached state nothing is written.
int vgpa_lag_covariance(vgpa_ctx* c, int kind, const double* x, int32_t n_anchor, const int64_t* anchors, int32_t stride, double* out) {
  if (!c) return VGPA_ERR_ARG;
  if (!out || !anchors) return fail(c, VGPA_ERR_ARG, "null argument");
  if (kind != VGPA_LAG_COVARIANCE && kind != VGPA_LAG_PROPAGATOR) return fail(c, VGPA_ERR_ARG, "unknown kind of lag covariance -> %d", kind);
  if (n_anchor < 1 || stride < 1) return fail(c, VGPA_ERR_ARG, "n_anchor and stride must be at least 1 (n_anchor = %d, stride = %d)", n_anchor, stride);
  for (int32_t i = 0; i < n_anchor; i++)
    if (anchors[i] < 0 || anchors[i] >= c->Np || (i > 0 && anchors[i] <= anchors[i - 1]))
      return fail(c, VGPA_ERR_ARG, "anchor %d -> %lld: the anchors are strictly increasing grid indices in [0, %d)", i, (long long)anchors[i], c->Np);
  if (kind == VGPA_LAG_COVARIANCE && x) return fail(c, VGPA_ERR_ARG, "the covariance kind reads the cached S_t: it takes no x");
  if (c->D > kMaxSmallD) return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariance is built for D <= %d (D = %d)", kMaxSmallD, c->D);
  const int D = c->D, B = c->B, kept = (c->Np - 1) / stride + 1;
  int rc;
  if ((double)B * (double)n_anchor * (double)kept * (double)c->DD > 34359738368.0)      // (the limit of check_stored)
    return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariances are built for at most 2^35 entries (batch %d, %d anchors, %d kept grid indices, D = %d): "
                "use a larger stride or fewer anchors", B, n_anchor, kept, D);
  if (!lag_grid_fits(D, B, n_anchor))
    return fail(c, VGPA_ERR_UNSUPPORTED, "the lag covariance is built for at most 2^31 - 1 workgroups (batch %d, %d anchors)", B, n_anchor);
  if (kind == VGPA_LAG_COVARIANCE && !c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  if (!x && !c->res.cached)
    return fail(c, VGPA_ERR_STATE, "no cached state: lag_covariance without x needs the state cached by a previous free_energy / sweep");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  if (x) {
    if ((rc = ingest_x(c, x, false))) return rc;
    c->res.cache_dropped();           // (d_x no longer holds the x of the cached state)
  }
  const size_t n_start = (size_t)B * n_anchor * c->DD, n_out = n_start * kept;
  if ((rc = grow(c, &c->d_lag_start, &c->lag_start_n, n_start + (size_t)(n_anchor + 1) / 2)) || (rc = grow(c, &c->d_sp_out, &c->sp_out_n, n_out))) return rc;
  int32_t* d_anchors = reinterpret_cast<int32_t*>(c->d_lag_start + n_start);      // (behind the starting matrices, in the same block)
  std::vector<int32_t> h_anchors(anchors, anchors + n_anchor);
  HIP_TRY(c, hipMemcpyAsync(d_anchors, h_anchors.data(), sizeof(int32_t) * n_anchor, hipMemcpyHostToDevice, c->stream));
  LagStartArgs s{};
  s.D = D; s.Np = c->Np; s.batch = B; s.n_anchor = n_anchor; s.anchors = d_anchors; s.start = c->d_lag_start;
  s.layout = LagStartArgs::Identity;
  if (kind == VGPA_LAG_COVARIANCE) {
    if (c->res.moments == Resident::Moments::TimeMajor) { s.layout = LagStartArgs::TimeMajor; s.S = c->d_msT; s.bpad = c->bpad; }
    else { s.layout = c->res.S == Resident::SLayout::Packed ? LagStartArgs::Packed : LagStartArgs::Whole; s.S = c->d_S; }
  }
  LAUNCH_TRY(c, "lag covariance start launch", launch_lag_start(s, c->stream));
  LagArgs a{};
  a.D = D; a.Np = c->Np; a.batch = B; a.n_anchor = n_anchor; a.stride = stride; a.n_keep = kept; a.method = c->cfg.method; a.dt = c->cfg.dt;
  a.A = ctx_A(c); a.stride_x = c->len_x; a.start = c->d_lag_start; a.anchors = d_anchors; a.out = c->d_sp_out;
  LAUNCH_TRY(c, "lag covariance launch", launch_lag(a, c->stream));
  if ((rc = download(c, out, c->d_sp_out, n_out))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (also: the host copy of the anchors lives on this stack frame)
  return VGPA_OK;
}

int vgpa_fetch(vgpa_ctx* c, int which, double* out) {
  if (!c || !out) return fail(c, VGPA_ERR_ARG, "null argument");
  if (!c->res.cached) return fail(c, VGPA_ERR_STATE, "no cached state: call free_energy first");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  const size_t BN = (size_t)c->B * c->Np;
  int rc = VGPA_OK;
  if ((rc = materialize_moments(c))) return rc;
  if (which != VGPA_FETCH_MT && which != VGPA_FETCH_ST && which != VGPA_FETCH_EDF && (rc = materialize_derived(c))) return rc;
  if ((which == VGPA_FETCH_LAMT || which == VGPA_FETCH_PSIT) && c->res.bwd == Resident::Bwd::None && !c->stream_ld && (rc = run_bwd(c, false, c->plan.sym_inputs))) return rc;
  switch (which) {
    case VGPA_FETCH_MT: rc = download(c, out, c->d_m, BN * c->D); break;
    case VGPA_FETCH_ST: {
      const double* full = nullptr;
      if ((rc = unpack_S(c, &full))) return rc;
      rc = download(c, out, full, BN * c->DD);
      break;
    }
    case VGPA_FETCH_LAMT: rc = download(c, out, c->d_lam, BN * c->D); break;
    case VGPA_FETCH_PSIT:
      if (!c->d_psi || c->stream_ld) return fail(c, VGPA_ERR_UNSUPPORTED, "Psi_t is not kept by the time-chunked large-D sweep");
      if (c->res.bwd == Resident::Bwd::Q) {   // recover Psi_t = (Sigma^-1 A_t - Q''_t) / 2 in place: from here on d_psi holds Psi_t again
        LAUNCH_TRY(c, "Psi_t recovery launch", launch_psi_from_q(c->B, c->Np, c->D, c->len_x, ctx_A(c), c->in.isg.rows, c->in.isg.stride, c->d_psi, c->stream));
        c->res.psi_recovered();
      }
      rc = download(c, out, c->d_psi, BN * c->DD); break;
    case VGPA_FETCH_EFX: rc = download(c, out, c->d_Ef, BN * c->D); break;
    case VGPA_FETCH_DESDE_DM: rc = download(c, out, c->d_dEm, BN * c->D); break;
    case VGPA_FETCH_DESDE_DS:
      if (!c->d_dEs || c->stream_ld) return fail(c, VGPA_ERR_UNSUPPORTED, "dEsde_dS is not kept by the time-chunked large-D sweep");
      if (c->res.dEs == Resident::DesLayout::Packed) {   // whole matrices into the scratch copy the unpacked S_t uses too (the packed stream stays as it is)
        if ((rc = ensure(c, &c->d_Sfull, BN * c->DD))) return rc;
        LAUNCH_TRY(c, "unpack launch", launch_unpack_lower(BN, c->D, c->d_dEs, c->d_Sfull, c->stream));
        rc = download(c, out, c->d_Sfull, BN * c->DD);
        break;
      }
      if (c->res.dEs == Resident::DesLayout::Upper) {
        LAUNCH_TRY(c, "mirror launch", launch_mirror_upper(BN, c->D, c->d_dEs, c->stream));
        c->res.des_mirrored();
      }
      rc = download(c, out, c->d_dEs, BN * c->DD); break;
    case VGPA_FETCH_ESDE_T: rc = download(c, out, c->d_et, BN); break;
    case VGPA_FETCH_EDF: {
      if ((rc = ensure(c, &c->d_Edf, BN * c->DD))) return rc;
      EnergyArgs a = energy_args(c, c->d_Edf);
      LAUNCH_TRY(c, "edf launch", launch_edf(a, c->stream));
      rc = download(c, out, c->d_Edf, BN * c->DD);
      break;
    }
    default: return fail(c, VGPA_ERR_ARG, "unknown fetch selector %d", which);
  }
  if (rc) return rc;
  return vgpa_synchronize(c);
}

int vgpa_gradient_dev(vgpa_ctx* c, double* g_dev) {
  if (!c || !g_dev) return fail(c, VGPA_ERR_ARG, "null argument");
  if (!c->res.cached) return fail(c, VGPA_ERR_STATE, "gradient(x, eval_fun=False) needs the state cached by a previous free_energy");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = finish_gradient(c, g_dev))) return rc;
  return check_status(c);
}

// The *_dev entry points consume the caller's x in place: the cached state refers to that memory until the next
// evaluation.  A caller about to free or overwrite it says so here; gradient(x, eval_fun=False) then fails loudly
// instead of reading freed memory.
int vgpa_release_x(vgpa_ctx* c) {
  if (!c) return VGPA_ERR_ARG;
  if (c->xcur != c->d_x) { c->xcur = nullptr; c->res.cache_dropped(); }
  return VGPA_OK;
}

static int vec_scratch(vgpa_ctx* c, uint64_t seglen) {
  const size_t need = (size_t)c->B * (3 + (size_t)vec_blocks_per_seg((long long)seglen, c->B));
  if (c->vec_scratch_n >= need) return VGPA_OK;
  c->vec_scratch_n = (size_t)c->B * (3 + 256);
  return dev_alloc(c, &c->d_vec_scratch, c->vec_scratch_n);
}
static int vec_reduce_host(vgpa_ctx* c, int mode, const double* a, const double* b, uint64_t seglen, double* out) {
  if (!c || !a || !out || seglen == 0) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = vec_scratch(c, seglen))) return rc;
  double* red = c->d_vec_scratch + 2 * (size_t)c->B;    // [0,2B) holds the axpby coefficients
  LAUNCH_TRY(c, "vector reduction", vec_reduce(mode, a, b, c->B, (long long)seglen, red, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, red, sizeof(double) * c->B, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}
int vgpa_vec_dot(vgpa_ctx* c, const double* a, const double* b, uint64_t seglen, double* out) {
  if (!b) return fail(c, VGPA_ERR_ARG, "null argument");
  return vec_reduce_host(c, 0, a, b, seglen, out);
}
int vgpa_vec_absmax(vgpa_ctx* c, const double* a, uint64_t seglen, double* out) { return vec_reduce_host(c, 1, a, nullptr, seglen, out); }
int vgpa_vec_asum(vgpa_ctx* c, const double* a, uint64_t seglen, double* out) { return vec_reduce_host(c, 2, a, nullptr, seglen, out); }
int vgpa_vec_axpby(vgpa_ctx* c, uint64_t seglen, const double* alpha, const double* x, const double* beta, const double* y, double* out) {
  if (!c || !alpha || !x || !out || seglen == 0 || ((y != nullptr) != (beta != nullptr))) return fail(c, VGPA_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  if ((rc = vec_scratch(c, seglen))) return rc;
  // The caller's coefficient arrays may be gone when this returns: copy them into a pinned ring slot first.  A slot is
  // reused only after the upload that read it has completed (its event); the device-side slots are stream-ordered
  // behind the previous axpby.
  const size_t B = (size_t)c->B;
  if (!c->h_coef) {
    HIP_TRY(c, hipHostMalloc((void**)&c->h_coef, sizeof(double) * 2 * B * vgpa_ctx::kCoefSlots, hipHostMallocDefault));
    for (auto& ev : c->ev_coef) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  const unsigned slot = c->coef_next % vgpa_ctx::kCoefSlots;
  if (c->coef_next >= (unsigned)vgpa_ctx::kCoefSlots) HIP_TRY(c, hipEventSynchronize(c->ev_coef[slot]));
  c->coef_next++;
  double* h = c->h_coef + (size_t)slot * 2 * B;
  std::memcpy(h, alpha, sizeof(double) * B);
  if (beta) std::memcpy(h + B, beta, sizeof(double) * B);
  HIP_TRY(c, hipMemcpyAsync(c->d_vec_scratch, h, sizeof(double) * (beta ? 2 * B : B), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_coef[slot], c->stream));
  LAUNCH_TRY(c, "axpby", vec_axpby(c->B, (long long)seglen, c->d_vec_scratch, x, c->d_vec_scratch + c->B, y, out, c->stream));
  return VGPA_OK;
}

int vgpa_set_option(vgpa_ctx* c, int option, int64_t value) {
  if (!c) return VGPA_ERR_ARG;
  if (option == VGPA_OPT_LD_CHUNK) {
    if (value < 1) return fail(c, VGPA_ERR_ARG, "chunk must be >= 1");
    if (value > c->Np - 1) value = c->Np > 1 ? c->Np - 1 : 1;
    if (c->d_dEs_c || c->d_psi_c) return fail(c, VGPA_ERR_STATE, "the chunk buffers exist already: set the option before the first sweep");
    c->ld_chunk = (int)value;
    return VGPA_OK;
  }
  return fail(c, VGPA_ERR_ARG, "unknown option %d", option);
}

// E0 = KL(q0||p0) is constant in x but not in the prior: the reference recomputes it on every free_energy call
// (variational.py:185) from kl0.mu0 / kl0.tau0, which are plain attributes.  The host mirror passes the current value.
int vgpa_set_prior_energy(vgpa_ctx* c, double e0) {
  if (!c) return VGPA_ERR_ARG;
  c->cfg.e0 = e0;
  c->in.e0 = {};                    // (every problem of the batch: per-problem values set earlier are gone)
  return VGPA_OK;
}

// The observation index maps [B][Np] of candidate inputs: obs_t rows [B][M] (null: the shared row for every problem) under counts [B] (null:
// M each).  Only the first counts[p] entries of a row are read.  model_rows: a per-problem observation model is (about to be) in force.
// *shared: every map equals the shared one, so that the shared-time kernels stay -- unless the stepper is the lane one and model_rows, whose
// kernels take a per-problem model on their per-problem-times instantiations.  false: the context's message names the row.
static bool index_batch_times(vgpa_ctx* c, const int64_t* rows, const int32_t* counts, bool model_rows, std::vector<int32_t>* idx, bool* shared) {
  const int M = c->M, Np = c->Np, B = c->B;
  const bool lane_rows = model_rows && stepper(c, false, true) == Stepper::Lane;
  *shared = !lane_rows;
  idx->clear();
  if (!rows && !counts && !lane_rows) return true;
  idx->resize((size_t)B * Np);
  for (int p = 0; p < B; p++) {
    int32_t* row = idx->data() + (size_t)p * Np;
    if (!index_obs_times(rows ? rows + (size_t)p * M : c->h_obs_t.data(), counts ? counts[p] : M, Np, row)) {
      fail(c, VGPA_ERR_ARG, "problem %d: obs_t must be strictly increasing indices in [0, Np)", p);
      return false;
    }
    *shared = *shared && std::memcmp(row, c->h_obs_idx.data(), sizeof(int32_t) * Np) == 0;
  }
  return true;
}

// ... and what index_batch_times found, put in force: the per-problem maps (and the rows of c->h_pp_obs_t, if any) unless shared.  Synchronous.
static int commit_times(vgpa_ctx* c, const std::vector<int32_t>& idx, bool shared) {
  BatchInputs& in = c->in;
  int rc;
  in.obs_t = {c->d_obs_t, 0}; in.obs_idx = {c->d_obs_idx, 0};
  if (shared) return VGPA_OK;
  if (!c->h_pp_obs_t.empty() && (rc = upload_rows(c, &c->d_pp_obs_t, c->h_pp_obs_t.data(), c->M, &in.obs_t))) return rc;
  if ((rc = upload_rows(c, &c->d_pp_obs_idx, idx.data(), c->Np, &in.obs_idx))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));          // (idx lives on the caller's stack frame)
  return VGPA_OK;
}

// Per-problem inputs of a batched context (see vgpa_hip.h).  Everything is validated before anything is uploaded.
int vgpa_set_problem_data(vgpa_ctx* c, const int64_t* obs_t, const double* obs_y, const double* m0, const double* s0, const double* e0) {
  if (!c) return VGPA_ERR_ARG;
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  if (c->stream_ld) return fail(c, VGPA_ERR_UNSUPPORTED, "the time-chunked large-D sweep holds one problem: no per-problem data");
  const int D = c->D, M = c->M, B = c->B;
  std::vector<int32_t> idx;
  bool shared_t = true;             // every row at the shared times: keep the shared-time kernels (the same results, bit for bit)
  if (obs_t && M > 0 && D > kMaxSmallD)
    return fail(c, VGPA_ERR_UNSUPPORTED, "per-problem observation times exist for D <= %d (D = %d shares the times of vgpa_config)", kMaxSmallD, D);
  // (only the prefix that the counts in force select is read: vgpa_set_problem_obs_model)
  if (M > 0 && !index_batch_times(c, obs_t, c->h_nobs.empty() ? nullptr : c->h_nobs.data(), c->obs_model_rows, &idx, &shared_t)) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  // every call states the whole per-problem set: an input passed as NULL is the shared one of vgpa_config again
  BatchInputs& in = c->in;
  in.obs_y = {c->d_obs_y, 0}; in.m0 = {c->d_m0, 0}; in.S0 = {c->d_S0, 0};
  in.e0 = {};
  if (obs_t && M > 0) c->h_pp_obs_t.assign(obs_t, obs_t + (size_t)B * M); else c->h_pp_obs_t.clear();
  if ((rc = commit_times(c, idx, shared_t))) return rc;
  if (obs_y && M > 0 && (rc = upload_rows(c, &c->d_pp_obs_y, obs_y, (size_t)M * D, &in.obs_y))) return rc;
  if (m0 && (rc = upload_rows(c, &c->d_pp_m0, m0, D, &in.m0))) return rc;
  if (s0 && (rc = upload_rows(c, &c->d_pp_S0, s0, c->DD, &in.S0))) return rc;
  if (s0) in.h_S0.assign(s0, s0 + (size_t)B * c->DD); else in.h_S0.clear();
  if (e0) {
    in.h_e0.assign(e0, e0 + B);
    if ((rc = upload_rows(c, &c->d_pp_e0, in.h_e0.data(), 1, &in.e0))) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->s0_rows_sym = !s0 || stack_symmetric(s0, (size_t)B, D);       // (a non-symmetric s0 row: both products literally)
  make_plan(c);
  c->pt_dense_zeroed = false;
  c->res.cache_dropped();           // (like vgpa_release_x: the cached state belongs to the old inputs)
  return VGPA_OK;
}

// Per-problem parameters of a batched context (see vgpa_hip.h).  Every row is validated and its constants computed on the host, as
// vgpa_create computes the shared ones, before anything changes: after an error the previous parameters stay in force.
int vgpa_set_problem_params(vgpa_ctx* c, const double* theta, const double* sigma) {
  if (!c) return VGPA_ERR_ARG;
  if (c->cfg.model == VGPA_MODEL_NONE) return fail(c, VGPA_ERR_STATE, "context has no stochastic model (ODE-only): no parameters to set");
  if (c->stream_ld && (theta || sigma))
    return fail(c, VGPA_ERR_UNSUPPORTED, "the time-chunked large-D sweep holds one problem: no per-problem parameters");
  const int D = c->D, B = c->B, nth = c->cfg.n_theta;
  const size_t DD = c->DD;
  std::vector<double> th((size_t)B * kMaxTheta), sg((size_t)B * DD), is((size_t)B * DD), ig((size_t)B * D), s1(B), qs(B);
  bool same_theta = true, same_sigma = true;
  SigmaForm rows;                   // the conjunction over the rows
  for (int p = 0; p < B; p++) {
    double* tp = th.data() + (size_t)p * kMaxTheta;
    for (int i = 0; i < kMaxTheta; i++) tp[i] = (theta && i < nth) ? theta[(size_t)p * nth + i] : c->theta[i];
    same_theta = same_theta && std::memcmp(tp, c->theta, sizeof(double) * kMaxTheta) == 0;
    double* sp = sg.data() + p * DD;
    std::memcpy(sp, sigma ? sigma + p * DD : c->h_sigma.data(), sizeof(double) * DD);
    same_sigma = same_sigma && std::memcmp(sp, c->h_sigma.data(), sizeof(double) * DD) == 0;
    SigmaForm f;
    const int rc = invert_sigma(D, c->single, sp, is.data() + p * DD, ig.data() + (size_t)p * D, &s1[p], &f);
    if (rc == VGPA_ERR_ARG) return fail(c, rc, "problem %d: the diffusion noise value: %g, should be strictly positive.", p, sp[0]);
    if (rc) return fail(c, rc, "problem %d: noise matrix is not positive definite.", p);
    rows.diag = rows.diag && f.diag; rows.iso = rows.iso && f.iso; rows.sym = rows.sym && f.sym;
    qs[p] = ig[(size_t)p * D];
  }
  if (D > kMaxSmallD && !same_sigma)
    return fail(c, VGPA_ERR_UNSUPPORTED, "per-problem Sigma exists for D <= %d (D = %d shares the Sigma of vgpa_config)", kMaxSmallD, D);
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  c->res.cache_dropped();           // (like vgpa_set_problem_data: the cached state belongs to the old parameters)
  BatchInputs& in = c->in;
  in.h_Sigma.clear();
  in.theta = in.sig1 = in.qs = {}; in.Sigma = {c->d_Sigma, 0}; in.isig = {c->d_isig, 0}; in.isg = {c->d_isg, 0};
  // every row at the shared parameters: the shared kernels (the same results, bit for bit); else every row is in force -- above D = 64
  // theta's only (Sigma is the shared one there)
  if (!same_theta || !same_sigma) {
    int rc;
    in.h_theta = std::move(th);
    if ((rc = upload_rows(c, &c->d_pp_theta, in.h_theta.data(), kMaxTheta, &in.theta))) return rc;
    if (D <= kMaxSmallD) {
      in.h_isig = std::move(is); in.h_sig1 = std::move(s1);
      if ((rc = upload_rows(c, &c->d_pp_Sigma, sg.data(), DD, &in.Sigma))) return rc;
      in.h_Sigma = sg;
      if ((rc = upload_rows(c, &c->d_pp_isig, in.h_isig.data(), DD, &in.isig))) return rc;
      if ((rc = upload_rows(c, &c->d_pp_isg, ig.data(), D, &in.isg))) return rc;
      if ((rc = upload_rows(c, &c->d_pp_sig1, in.h_sig1.data(), 1, &in.sig1))) return rc;
      if ((rc = upload_rows(c, &c->d_pp_qs, qs.data(), 1, &in.qs))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (the host rows live on this stack frame)
  }
  c->rows_form = rows;
  make_plan(c);
  return VGPA_OK;
}

// Per-problem observation model of a batched context (see vgpa_hip.h).  Every row's constants come from obs_constants, as vgpa_create computes
// the shared ones; everything is validated before anything changes: after an error the previous model stays in force.
int vgpa_set_problem_obs_model(vgpa_ctx* c, const int32_t* n_obs, const double* obs_noise, const double* obs_h) {
  if (!c) return VGPA_ERR_ARG;
  if (!c->full) return fail(c, VGPA_ERR_STATE, "context was created without m0/s0/observations (ODE-only)");
  if (c->D > kMaxSmallD || c->stream_ld)
    return fail(c, VGPA_ERR_UNSUPPORTED, "a per-problem observation model exists for D <= %d (D = %d shares the model of vgpa_config)", kMaxSmallD, c->D);
  const int D = c->D, M = c->M, B = c->B;
  const size_t DD = c->DD, RS = c->single ? 1 : DD;      // doubles per R row
  if (M < 1) return fail(c, VGPA_ERR_ARG, "the context has no observations");
  if (c->single && obs_h) return fail(c, VGPA_ERR_ARG, "1-D models take no observation operator");
  bool same = true;                 // every row at the shared model: the shared kernels and buffers (the same results, bit for bit)
  for (int p = 0; p < B; p++) {
    if (n_obs && (n_obs[p] < 1 || n_obs[p] > M)) return fail(c, VGPA_ERR_ARG, "problem %d: %d observations, outside [1, %d]", p, n_obs[p], M);
    same = same && (!n_obs || n_obs[p] == M) && (!obs_noise || std::memcmp(obs_noise + p * RS, c->h_R.data(), sizeof(double) * RS) == 0) &&
           (!obs_h || std::memcmp(obs_h + p * DD, c->h_H.data(), sizeof(double) * DD) == 0);
  }
  std::vector<double> Q, K, rinv, jsc, jscp, oc;
  bool all_diag = true, all_sym = true;
  if (!same) {
    Q.assign(B * DD, 0.0); K.assign(B * DD, 0.0); rinv.assign((size_t)B * D, 0.0); jsc.assign(B * DD, 0.0); jscp.assign(B * DD, 0.0); oc.assign(B, 0.0);
    for (int p = 0; p < B; p++) {
      const double* Rp = obs_noise ? obs_noise + p * RS : c->h_R.data();
      if (c->single && !(Rp[0] > 0.0)) return fail(c, VGPA_ERR_ARG, "problem %d: observation noise must be positive, got %g", p, Rp[0]);
      bool diag = false;
      double* jp = jsc.data() + p * DD;
      const int rc = obs_constants(D, n_obs ? n_obs[p] : M, c->single, Rp, obs_h ? obs_h + p * DD : c->h_H.data(), Q.data() + p * DD, K.data() + p * DD,
                                   rinv.data() + (size_t)p * D, jp, &oc[p], &diag);
      if (rc) return fail(c, rc, "problem %d: observation noise matrix is not positive definite", p);
      all_diag = all_diag && diag; all_sym = all_sym && is_symmetric(jp, D);
      for (int r = 0; r < D; r++)      // the packed-triangle copy, as vgpa_create makes the shared one
        for (int q = 0; q <= r; q++) jscp[p * DD + (size_t)r * (r + 1) / 2 + q] = jp[(size_t)r * D + q];
    }
  }
  // the index maps of the new counts over the observation times in force; a prefix that now reaches an invalid stored entry fails here
  std::vector<int32_t> idx;
  bool shared_t = true;
  if (!index_batch_times(c, c->h_pp_obs_t.empty() ? nullptr : c->h_pp_obs_t.data(), (same || !n_obs) ? nullptr : n_obs, !same, &idx, &shared_t)) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  int rc;
  BatchInputs& in = c->in;
  if (!same) {      // (uploads first: a failed allocation leaves the record on the previous rows)
    Rows<double> rQ, rK, rr, rj, rjp, roc; Rows<int32_t> rn;
    std::vector<int32_t> cnt(B, M);
    if (n_obs) cnt.assign(n_obs, n_obs + B);
    if ((rc = upload_rows(c, &c->d_pp_Q, Q.data(), DD, &rQ)) || (rc = upload_rows(c, &c->d_pp_K, K.data(), DD, &rK)) ||
        (rc = upload_rows(c, &c->d_pp_rinv, rinv.data(), D, &rr)) || (rc = upload_rows(c, &c->d_pp_jsc, jsc.data(), DD, &rj)) ||
        (rc = upload_rows(c, &c->d_pp_jscp, jscp.data(), DD, &rjp)) || (rc = upload_rows(c, &c->d_pp_obsc, oc.data(), 1, &roc)) ||
        (rc = upload_rows(c, &c->d_pp_nobs, cnt.data(), 1, &rn)))
      return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (the host rows live on this stack frame)
    in.Q = rQ; in.K = rK; in.rinv = rr; in.jsc = rj; in.jscp = rjp; in.obs_const = roc; in.n_obs = rn;
    c->h_nobs = n_obs ? cnt : std::vector<int32_t>();
  } else {
    in.Q = {c->d_Q, 0}; in.K = {c->d_K, 0}; in.rinv = {c->d_rinv, 0}; in.jsc = {c->d_jsc, 0}; in.jscp = {c->d_jscp, 0};
    in.obs_const = {}; in.n_obs = {};
    c->h_nobs.clear();
  }
  c->obs_model_rows = !same;
  c->obs_diag = same ? c->shared_obs_diag : all_diag;      // the kernel family every row allows
  c->jsc_rows_sym = same || all_sym;
  if ((rc = commit_times(c, idx, shared_t))) return rc;
  make_plan(c);
  c->pt_dense_zeroed = false;
  c->res.cache_dropped();           // (like the other setters: the cached state belongs to the old model)
  return VGPA_OK;
}

int vgpa_is_streaming(vgpa_ctx* c) { return (c && c->stream_ld) ? 1 : 0; }

// Plan and Resident as plain integers (tests, diagnostics): reads the two records and nothing else
int vgpa_path_info(vgpa_ctx* c, vgpa_path* out) {
  if (!c || !out) return VGPA_ERR_ARG;     // (no fail(): the context's error message is state too)
  static_assert((int)Stepper::LargeD == VGPA_STEPPER_LARGE_D && (int)Stepper::Lane == VGPA_STEPPER_LANE && (int)Stepper::Wave == VGPA_STEPPER_WAVE &&
                (int)Stepper::Mfma == VGPA_STEPPER_MFMA && (int)Stepper::Generic == VGPA_STEPPER_GENERIC, "Stepper and VGPA_STEPPER_*");
  static_assert((int)Resident::Moments::RowMajor == VGPA_MOMENTS_ROW_MAJOR && (int)Resident::Moments::TimeMajor == VGPA_MOMENTS_TIME_MAJOR, "VGPA_MOMENTS_*");
  static_assert((int)Resident::DesLayout::Whole == VGPA_LAYOUT_WHOLE && (int)Resident::DesLayout::Upper == VGPA_LAYOUT_UPPER &&
                (int)Resident::DesLayout::Packed == VGPA_LAYOUT_PACKED, "VGPA_LAYOUT_*");
  static_assert((int)Resident::Bwd::None == VGPA_BWD_NONE && (int)Resident::Bwd::Psi == VGPA_BWD_PSI && (int)Resident::Bwd::Q == VGPA_BWD_Q, "VGPA_BWD_*");
  const Plan& p = c->plan;
  const Resident& r = c->res;
  out->fwd = (int32_t)p.fwd; out->bwd = (int32_t)p.bwd;
  out->sym_units = p.sym_units; out->launch_sym_units = p.launch_sym_units; out->lane_pass = p.lane_pass;
  out->bwd_upper = p.bwd_upper; out->store_q = p.store_q; out->packed = p.packed;
  out->grad_in_bwd = p.grad_in_bwd; out->grad_in_bwd_now = p.grad_in_bwd_now;
  out->cached = r.cached; out->moments = (int32_t)r.moments;
  out->S = r.S == Resident::SLayout::Packed ? VGPA_LAYOUT_PACKED : VGPA_LAYOUT_WHOLE;
  out->dEs = (int32_t)r.dEs; out->bwd_holds = (int32_t)r.bwd; out->terms = r.terms;
  out->helper_roles = p.helper_roles;
  return VGPA_OK;
}

// ---- raw device memory ------------------------------------------------------------------------------
int vgpa_dev_alloc(vgpa_ctx* c, uint64_t bytes, void** out) {
  if (!c || !out) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipMalloc(out, bytes ? bytes : 8));
  c->user_allocs.push_back(*out);          // whatever the caller does not return is freed with the context
  return VGPA_OK;
}
int vgpa_dev_free(vgpa_ctx* c, void* ptr) {
  if (!c) return VGPA_ERR_ARG;
  if (!ptr) return VGPA_OK;
  // (may run from a garbage collector at any point of the calling thread: its current device is put back)
  int prev = -1;
  (void)hipGetDevice(&prev);
  struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{prev};
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (ptr == (const void*)c->xcur) { c->xcur = nullptr; c->res.cache_dropped(); }
  for (size_t i = 0; i < c->user_allocs.size(); i++)
    if (c->user_allocs[i] == ptr) { c->user_allocs[i] = c->user_allocs.back(); c->user_allocs.pop_back(); break; }
  HIP_TRY(c, hipFree(ptr));
  return VGPA_OK;
}
int vgpa_memcpy_h2d(vgpa_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}
int vgpa_memcpy_d2h(vgpa_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VGPA_OK;
}

// ---- device memory without a context (the row-sharded driver's callers: vgpa_amd/large_d.py keeps its buffers here) ----------------
// Plain hipMalloc / hipFree / synchronous hipMemcpy on `device`; the calling thread's current device is put back.
namespace {
struct DeviceScope {
  int prev = -1; bool ok = false;
  explicit DeviceScope(int device) { (void)hipGetDevice(&prev); ok = hipSetDevice(device) == hipSuccess; }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace
int vgpa_device_alloc(int device, uint64_t bytes, void** out) {
  if (!out) return VGPA_ERR_ARG;
  DeviceScope sc(device);
  if (!sc.ok) return VGPA_ERR_DEVICE;
  return hipMalloc(out, bytes ? bytes : 8) == hipSuccess ? VGPA_OK : VGPA_ERR_DEVICE;
}
int vgpa_device_free(int device, void* ptr) {
  if (!ptr) return VGPA_OK;
  DeviceScope sc(device);
  if (!sc.ok) return VGPA_ERR_DEVICE;
  return hipFree(ptr) == hipSuccess ? VGPA_OK : VGPA_ERR_DEVICE;
}
int vgpa_device_memcpy(int device, void* dst, const void* src, uint64_t bytes, int kind) {
  if ((!dst || !src) && bytes) return VGPA_ERR_ARG;
  if (kind < 1 || kind > 3) return VGPA_ERR_ARG;
  DeviceScope sc(device);
  if (!sc.ok) return VGPA_ERR_DEVICE;
  const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : (kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
  if (bytes == 0) return VGPA_OK;
  // (every stream of the library is non-blocking: the null-stream copy below does not wait for them by itself)
  if (kind != 1 && hipDeviceSynchronize() != hipSuccess) return VGPA_ERR_DEVICE;
  if (hipMemcpy(dst, src, bytes, k) != hipSuccess) return VGPA_ERR_DEVICE;
  return hipDeviceSynchronize() == hipSuccess ? VGPA_OK : VGPA_ERR_DEVICE;
}

// ---- profiling ----------------------------------------------------------------------------------------
int vgpa_profile_begin(vgpa_ctx* c) {
  if (!c) return VGPA_ERR_ARG;
  c->prof = true; c->prof_pending = false; c->prof_n = 0;
  for (auto& v : c->prof_ms) v = 0.0;
  return VGPA_OK;
}
int vgpa_profile_end(vgpa_ctx* c, double* fwd_ms, double* energy_ms, double* bwd_ms, double* grad_ms, int64_t* n_sweeps) {
  if (!c) return VGPA_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  c->prof = false;
  if (fwd_ms) *fwd_ms = c->prof_ms[0];
  if (energy_ms) *energy_ms = c->prof_ms[1];
  if (bwd_ms) *bwd_ms = c->prof_ms[2];
  if (grad_ms) *grad_ms = c->prof_ms[3];
  if (n_sweeps) *n_sweeps = c->prof_n;
  return VGPA_OK;
}

}  // extern "C"
