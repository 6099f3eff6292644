/*
 * vgpa_hip.h -- C ABI of libvgpa_hip.so: the MI355X (gfx950) implementation of VGPA's
 * forward-backward variational smoothing sweep.
 *
 * The reference (vrettasm/VGPA) is pure Python and has no FFI; its plugin boundary is the
 * duck-typed Python surface listed below.  Every entry point of this header names the reference
 * interface it stands behind (paths relative to the reference repository root):
 *
 *   vgpa_solve_fwd      <- FwdOde.__call__ -> <stepper>.solve_fwd   src/var_bayes/fwd_ode.py:45-65,
 *                          src/numerics/{euler.py:27,heun.py:28,runge_kutta2.py:25,runge_kutta4.py:25}
 *   vgpa_solve_bwd      <- BwdOde.__call__ -> <stepper>.solve_bwd   src/var_bayes/bwd_ode.py:45-65,
 *                          src/numerics/{euler.py:94,heun.py:113,runge_kutta2.py:104,runge_kutta4.py:115}
 *   vgpa_energy         <- <model>.energy(A, b, m, S, obs_t)        src/dynamics/ornstein_uhlenbeck.py:165,
 *                          double_well.py:169, lorenz_63.py:237, lorenz_96.py:316
 *   vgpa_obs_energy     <- GaussianLikelihood.__call__ / .gradients src/var_bayes/gaussian_like.py:69-243
 *   vgpa_free_energy    <- VarGP.free_energy(x)                     src/var_bayes/variational.py:141-200
 *   vgpa_gradient       <- VarGP.gradient(x, eval_fun=False)        src/var_bayes/variational.py:202-289
 *   vgpa_sweep          <- VarGP.gradient(x, eval_fun=True)  (what SCG calls, src/numerics/optim_scg.py:167)
 *   vgpa_fetch          <- VarGP.arg_out                            src/var_bayes/variational.py:292
 *
 * Conventions
 *   - plain C, no C++/torch types; all floating point data is IEEE fp64, C-contiguous;
 *   - every function returns VGPA_OK (0) or a negative vgpa_status; no exception crosses the
 *     boundary; vgpa_last_error() gives the message of the last failure on that context;
 *   - host-pointer entry points copy in/out and are synchronous on return;
 *     the *_dev entry points take DEVICE pointers (hipMalloc'ed by the caller, same device) and
 *     enqueue on the context's stream; call vgpa_synchronize() before reading results;
 *   - buffers are caller-owned; the context owns its device workspace; a context is not
 *     thread-safe (one host thread per context, like the reference's single-threaded use);
 *   - there is NO CPU fallback: without a HIP device vgpa_create fails with VGPA_ERR_DEVICE.
 *
 * Batching: a context may hold `batch` independent problems that share the configuration
 * (model, dt, Np, method) but have different variational parameters x.  By default they also share
 * theta, Sigma, R, H, the observation count M, the observations, m0, S0 and e0 of vgpa_config;
 * vgpa_set_problem_data gives each problem its own observations, m0, S0 and e0 (one dataset per problem),
 * vgpa_set_problem_params its own theta and Sigma (one parameter point per problem), and
 * vgpa_set_problem_obs_model its own observation count, R and H (one instrument per problem).  All per-problem
 * arrays are laid out problem-major: x[batch][len_x], mt[batch][Np][D], F[batch], ...
 */
#ifndef VGPA_HIP_H
#define VGPA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGPA_ABI_VERSION 2

/* ---- environment switches -------------------------------------------------------------------------------------------------------
   Every getenv() of the library, read ONCE per process (the first time the code path is reached) unless noted.  None of them changes a
   result beyond rounding; tests use them to reach paths the defaults take only at other sizes.  Nothing in vgpa_amd/ sets any of them.

   VGPA_ODE_KERNEL=pe|sym     33 <= D <= 44 / D <= 44: keep the role-specialised steppers (pe) / take the symmetric-unit ones (sym)
   VGPA_SYM_HELPERS=0|1|2     fragment-cover steppers: no helper waves / one helper role / two at every batch size (default: two up to
                              one problem per CU, none beyond); read by vgpa_create, like VGPA_ODE_KERNEL
   VGPA_FUSED_GRAD=0|1        backward RK4 fragment-cover kernel: never / always assemble the gradient on its third wave set
                              (default: from 64 problems per context on)
   VGPA_SHARD_CHUNKS=<n>      row-sharded recursion: sub-blocks of the pipelined gather (default 4; 0 = the serial schedule);
                              per shard: vgpa_shard_set_option
   VGPA_STAGE_FUSED=<n>       D > 64, one GPU: the latency version of the one-kernel Runge-Kutta stage up to D = n (0: never; default 512, and
                              only while a launch has at most 64 tile pairs)
   VGPA_STAGE_WIDE=<n>        ... the throughput version up to D = n (0: never; default 2048, and not where D >= 384 is a multiple of 64); with both 0: GEMM + stage
                              kernel as in rounds 1-4.  Read per call (tests run all three at one size)
   VGPA_DIAG_REPEAT=<phase>:<n>  launch one phase (fwd|energy|bwd|grad) of the fused sweep n times (clock / power samples under one
                              kernel, tools/power_per_kernel.sh); every phase is a pure function of its inputs
   Build and host side: VGPA_EXTRA_CFLAGS (vgpa_amd/build.py: extra compiler flags), VGPA_LIB (vgpa_amd/_lib.py: path of another
   build of this library).  */

typedef enum {
  VGPA_OK = 0,
  VGPA_ERR_ARG = -1,        /* bad argument / inconsistent configuration (Python: ValueError)      */
  VGPA_ERR_DEVICE = -2,     /* no usable HIP device, or a HIP runtime call failed (RuntimeError)   */
  VGPA_ERR_NOT_PD = -3,     /* a matrix that must be positive definite is not (LinAlgError)        */
  VGPA_ERR_STATE = -4,      /* call order violated, e.g. gradient before free_energy (RuntimeError) */
  VGPA_ERR_UNSUPPORTED = -5, /* valid request that this build does not implement (NotImplementedError) */
  VGPA_ERR_COMM = -6        /* a collective of the row-sharded path failed or timed out; the communicator has been aborted
                               and the shard is unusable (RuntimeError on every rank)                */
} vgpa_status;

/* model ids: dynamical_systems registry, src/var_bayes/simulation.py:20-21 */
enum { VGPA_MODEL_NONE = -1, /* ODE-only context: solve_fwd / solve_bwd, no energy terms */
       VGPA_MODEL_OU = 0, VGPA_MODEL_DW = 1, VGPA_MODEL_L63 = 2, VGPA_MODEL_L96 = 3 };
/* stepper ids: num_integration registry, src/numerics/utilities.py:12-13 */
enum { VGPA_ODE_EULER = 0, VGPA_ODE_HEUN = 1, VGPA_ODE_RK2 = 2, VGPA_ODE_RK4 = 3 };
/* vgpa_fetch selectors: keys of VarGP.output, src/var_bayes/variational.py:189-196 */
enum {
  VGPA_FETCH_MT = 0, VGPA_FETCH_ST = 1, VGPA_FETCH_LAMT = 2, VGPA_FETCH_PSIT = 3,
  VGPA_FETCH_EFX = 4, VGPA_FETCH_EDF = 5, VGPA_FETCH_DESDE_DM = 6, VGPA_FETCH_DESDE_DS = 7,
  VGPA_FETCH_ESDE_T = 8 /* per-grid-point E_sde(t) before the trapezoid, (Np,) */
};
/* config flags */
enum {
  VGPA_FLAG_FORCE_GENERIC = 1, /* use the generic (no symmetry assumption) stepping kernels */
  VGPA_FLAG_LIBRARY_GEMM = 8,  /* D > 64: rocBLAS dgemm (dlopen'ed) for the plain stage products W = A.X / A^T.Psi instead of the
                                  hand-written MFMA GEMM; everything fused stays hand-written.  Off by default. */
  VGPA_FLAG_STREAM_LARGE_D = 4, /* D > 64: time-chunked sweep that keeps only x, S_t and the gradient resident (Psi_t and
                                  dEsde_dS_t live in chunk buffers; VGPA_FETCH_PSIT is unavailable).  Chosen automatically
                                  when the resident arrays would not fit into free device memory. */
  VGPA_FLAG_SYM_UNITS = 16,    /* 5 <= D <= 44: the symmetric-unit stepping kernels (ode_sym_impl.h; two problems per CU, the
                                  default for 44 < D <= 64) instead of the role-specialised ones.  Same results to rounding. */
  VGPA_FLAG_KEEP_PSI = 32,     /* batched symmetric-unit sweeps (33 <= D <= 40, RK2 / RK4, Sigma = sigma^2 I): by default the backward
                                  kernel leaves Q''_t = Sigma^-1 A_t - 2 Psi_t where Psi_t would be -- all the gradient assembly
                                  needs of the two, one HBM stream less -- and VGPA_FETCH_PSIT recovers Psi_t from it
                                  ((Sigma^-1 A_t - Q''_t) / 2, equal to rounding).  This flag stores Psi_t itself. */
  VGPA_FLAG_MATERIALIZE = 64   /* lane-per-problem contexts of OU / double well / Lorenz-63 (D = 1 always, D = 3 from 512 problems):
                                  by default the fused objective runs as TWO kernels -- forward moments, then one backward pass
                                  that re-evaluates the closed-form E_sde terms in registers, steps (lam, Psi), assembles the
                                  gradient and sums F -- and dEsde_dm / dEsde_dS / <f> / E_sde(t) / lam_t / Psi_t reach HBM only
                                  when vgpa_fetch asks for them.  This flag keeps the four-kernel path that writes them all. */
};

typedef struct vgpa_ctx vgpa_ctx;

typedef struct {
  int32_t abi_version;   /* VGPA_ABI_VERSION */
  int32_t device;        /* HIP device ordinal */
  int32_t model;         /* VGPA_MODEL_* */
  int32_t method;        /* VGPA_ODE_* */
  int32_t dim_d;         /* state dimension D (1 for OU/DW, 3 for L63, >=4 for L96) */
  int32_t n_pts;         /* grid points Np = len(arange(t0, tf+dt, dt)) */
  int32_t batch;         /* independent problems held by this context (>= 1) */
  int32_t flags;         /* VGPA_FLAG_* */
  double dt;             /* time step (> 0) */
  int32_t n_theta;       /* 1 (OU, DW, L96) or 3 (L63) */
  int32_t n_obs;         /* number of observation times M (may be 0 for ODE-only contexts) */
  const double* theta;   /* [n_theta] drift parameters                                      */
  const double* sigma;   /* [D*D] system noise covariance (1-D models: one value)           */
  const double* m0;      /* [D]   initial mean       (NULL for ODE-only contexts)           */
  const double* s0;      /* [D*D] initial covariance (NULL for ODE-only contexts)           */
  const int64_t* obs_t;  /* [M]   observation indices into the grid, strictly increasing    */
  const double* obs_y;   /* [M*D] observation values                                        */
  const double* obs_noise; /* [D*D] observation noise covariance R (1-D models: one value)  */
  const double* obs_h;   /* [D*D] observation operator H, or NULL for the identity          */
  double e0;             /* KL(q0||p0), constant in x (src/var_bayes/prior_kl0.py:46-92)    */
} vgpa_config;

/* What the library does NOT build (VGPA_ERR_UNSUPPORTED; the reference's numpy handles these at its own speed):
 *   - D > 64 for OU / DW / L63 (their D is 1 / 1 / 3 by definition) -- D > 64 exists for Lorenz-96 and for the bare ODE
 *     operators (model NONE);
 *   - batch > 1 in the TIME-CHUNKED large-D sweep (a batch that does not fit resident).  Everything else of D > 64 is built:
 *     dense Sigma / S0 / R / H, several problems per context (the per-stage kernels take them in grid.z: what fills the chip
 *     for 64 < D <= 512), the hyper-parameter members, non-symmetric operator-level inputs (both products of the slope
 *     formed literally; the fused sweep and the row-sharded drivers assume the symmetric S0 / Sigma every real run has);
 *   - VGPA_FETCH_PSIT / VGPA_FETCH_DESDE_DS in the time-chunked large-D sweep (they are never resident there);
 *   - per-problem parameters (vgpa_set_problem_params): a per-problem Sigma at D > 64 (per-problem theta is built there), and
 *     any per-problem theta or Sigma in the time-chunked large-D sweep and the row-sharded drivers;
 *   - vgpa_theta_gradient in the time-chunked large-D sweep (and the row-sharded drivers have no such entry point);
 *   - a per-problem observation model (vgpa_set_problem_obs_model) at D > 64, in the time-chunked large-D sweep and in the
 *     row-sharded drivers: they share the observation count, R and H;
 *   - vgpa_sample_paths at D > 64 (the time-chunked large-D sweep included): the sampler keeps a block of paths of one problem
 *     next to A_t in one workgroup, which is what D <= 64 allows.
 * The matrix-core stepping kernels cover D <= 64 with symmetric inputs; non-symmetric operator-level inputs run on the
 * generic LDS kernels (same results, ~15x slower at D = 40). */

/* lifetime ------------------------------------------------------------------------------- */
int vgpa_create(vgpa_ctx** out, const vgpa_config* cfg);
void vgpa_destroy(vgpa_ctx* ctx);
const char* vgpa_last_error(const vgpa_ctx* ctx);   /* ctx == NULL: last error of vgpa_create */
int vgpa_abi_version(void);
int vgpa_device_count(void);                         /* 0 when no HIP device is visible */
int vgpa_synchronize(vgpa_ctx* ctx);
void* vgpa_stream(vgpa_ctx* ctx);                    /* the context's hipStream_t */

/* operator level (host pointers; problem-major when batch > 1) ------------------------------ */
/* (m_t, S_t) from (A, b, m0, S0, Sigma).  A:[Np,D,D] b:[Np,D] m0:[D] s0:[D,D] sigma:[D,D]
 * (the explicit m0 / s0 / sigma of this call serve every problem: per-problem data and parameters do not apply here) */
int vgpa_solve_fwd(vgpa_ctx* ctx, const double* lin_a, const double* off_b, const double* m0,
                   const double* s0, const double* sigma, double* mt, double* st);
/* (lam_t, Psi_t) from A, dEsde/dm [Np,D], dEsde/dS [Np,D,D] and the dense jump arrays of E_obs. */
int vgpa_solve_bwd(vgpa_ctx* ctx, const double* lin_a, const double* desde_dm, const double* desde_ds,
                   const double* deobs_dm, const double* deobs_ds, double* lam, double* psi);
/* E_sde and its per-grid-point terms.  Any output pointer may be NULL. */
int vgpa_energy(vgpa_ctx* ctx, const double* lin_a, const double* off_b, const double* mt,
                const double* st, double* esde, double* efx, double* edf, double* desde_dm,
                double* desde_ds);
/* E_obs and the dense jump arrays dEobs/dm [Np,D], dEobs/dS [Np,D,D] (zero off the obs rows). */
int vgpa_obs_energy(vgpa_ctx* ctx, const double* mt, const double* st, double* eobs,
                    double* deobs_dm, double* deobs_ds);

/* fused objective (state stays resident in HBM between calls) -------------------------------- */
int vgpa_free_energy(vgpa_ctx* ctx, const double* x, double* f);       /* f:[batch] */
int vgpa_gradient(vgpa_ctx* ctx, const double* x_or_null, double* g);  /* NULL: cached state */
int vgpa_sweep(vgpa_ctx* ctx, const double* x, double* f, double* g);  /* df(x, eval_fun=True) */
int vgpa_energy_parts(vgpa_ctx* ctx, double* e0, double* esde, double* eobs); /* each [batch] */
int vgpa_fetch(vgpa_ctx* ctx, int which, double* out);
/* dF/dtheta at fixed (A_t, b_t), from the state the last fused evaluation (free_energy, sweep, sweep_enqueue + fetch_f)
 * left resident.  out: [batch][n_theta], host.  Per-problem theta / Sigma / data in force are honoured.  The cached state
 * survives: vgpa_gradient(NULL), vgpa_gradient_dev, vgpa_fetch and vgpa_energy_parts return afterwards what they return
 * without this call.  (m_t, S_t, E0 and E_obs do not depend on theta, so this is the integral of
 * sum_i (Sigma^-1)_ii <(f - g)_i df_i/dtheta>.  OU, double well, Lorenz-63: equal to the reference's dEsde_dth.  Lorenz-96: the
 * unscented mean of the residual, with the flat roll of the energy -- the derivative of the F this library computes, which the
 * reference's dEsde_dth, built from the closed-form mean drift, is not.)  F is exactly quadratic in theta with a diagonal
 * Hessian at fixed (A_t, b_t): h = g(theta + 1) - g(theta) is the curvature, theta - g / h the minimiser.
 * VGPA_ERR_STATE: no cached state (also after vgpa_release_x, vgpa_set_problem_data, vgpa_set_problem_params), ODE-only
 * contexts; VGPA_ERR_UNSUPPORTED: the time-chunked large-D sweep; VGPA_ERR_NOT_PD: the evaluation that left the state failed with
 * it (an S_t of the named problem is not positive definite) -- nothing is written to out then. */
int vgpa_theta_gradient(vgpa_ctx* ctx, double* out);

/* The two-time covariance of the posterior process dx = (-A_t x + b_t) dt + Sigma^1/2 dW on the context's grid: for
 * t >= s, K(t, s) = Cov[x_t, x_s] = Phi(t, s) S_s with Phi the propagator of dPhi/dt = -A_t Phi, Phi(s, s) = I -- what autocorrelations, the
 * joint Gaussian over several times, the variance of an increment x_t - x_s or of a time average and the conditional law x_t | x_s are made
 * of.  For every anchor s and every grid index k >= s
 *   C_s = S_s (VGPA_LAG_COVARIANCE)  or  C_s = I (VGPA_LAG_PROPAGATOR),    C_{k+1} = step_k(C_k),
 * step_k the context's scheme for the MEAN equation applied to every column of C with b = 0 (the recursion m_t itself obeys, so that
 * m_k = Phi(k, s) m_s + the forcing's part holds for the library's m_t and not only in the limit dt -> 0), h = dt / 2, A_mid = (A_k + A_{k+1}) / 2:
 *   euler  C - dt A_k C;   heun  p = -A_k C, c = -A_{k+1} (C + dt p): C + h (p + c);   rk2  C - dt A_mid (C - h A_k C)  (no quirk: the mean's branch);
 *   rk4    the four stages with A_k, A_mid, A_mid, A_{k+1}: C + dt (k1 + 2 (k2 + k3) + k4) / 6.      1-D models: C and A_t are scalars.
 * K(k, s) for k < s is K(s, k)^T, with k as the anchor: only k >= s is computed.
 *   anchors    host, [n_anchor]: strictly increasing grid indices in [0, Np)
 *   out        host, [batch][n_anchor][n_keep][D][D] (1-D models: [batch][n_anchor][n_keep]), n_keep = (Np - 1) / stride + 1: the kept grid
 *              indices k = 0, stride, 2 stride, ...; the kept rows with k < anchor are zero.  The row k = s (when kept) is bit for bit the S_s
 *              of vgpa_fetch(VGPA_FETCH_ST), or I.  The block of an anchor does not depend on the other anchors of the call, the block of a
 *              problem not on the batch around it, a kept row not on the stride: bit for bit.
 *   VGPA_LAG_PROPAGATOR reads A_t only.  x_or_null as in vgpa_sample_paths: a given x (host, [batch][len_x]) is uploaded and the cached sweep
 *              state is dropped; NULL: the x of the cached evaluation.  Works on ODE-only contexts and on VGPA_MODEL_NONE (with an x).
 *   VGPA_LAG_COVARIANCE takes x NULL only and reads the S_t the last fused evaluation left resident, in the layout it is in.  Per-problem x
 *              is honoured; theta, Sigma and the data enter through S_s alone.
 * Nothing of the cached state is written: vgpa_gradient(NULL), vgpa_fetch, vgpa_energy_parts and vgpa_theta_gradient return afterwards bit
 * for bit what they return without this call.
 * VGPA_ERR_ARG: a null out or anchors, n_anchor < 1, stride < 1, an unknown kind, anchors outside [0, Np) or not strictly increasing, an x
 * with the covariance kind; VGPA_ERR_UNSUPPORTED, before any work: D > 64 (the time-chunked large-D sweep included), a result of more than
 * 2^35 entries; VGPA_ERR_STATE: no cached state where one is needed (x NULL; the covariance kind on an ODE-only context).  The context
 * stays usable after every error. */
enum { VGPA_LAG_COVARIANCE = 0, VGPA_LAG_PROPAGATOR = 1 };
int vgpa_lag_covariance(vgpa_ctx* ctx, int kind, const double* x_or_null, int32_t n_anchor, const int64_t* anchors, int32_t stride,
                        double* out);

/* Sample paths on the context's grid by Euler-Maruyama: n_paths independent paths of every problem, of the posterior process
 * dx = (-A_t x + b_t) dt + Sigma^1/2 dW (VGPA_PATHS_POSTERIOR: what the moments m_t, S_t are the moments of) or of the model SDE
 * dx = f_theta(x) dt + Sigma^1/2 dW (VGPA_PATHS_MODEL: what a data set is a noisy record of; the reference's
 * StochasticProcess.make_trajectory, src/dynamics/stochastic_process.py, one path at a time).
 *   x_k = x_{k-1} + dt drift_{k-1}(x_{k-1}) + R_p xi_k,   R_p = chol_lower(Sigma_p dt)   (1-D models: sqrt(sigma dt)),
 * with the Sigma in force (per-problem rows of vgpa_set_problem_params honoured).  For a dense Sigma the LOWER factor is used on purpose:
 * the reference's _noise_increments multiplies by scipy's upper factor, whose increments do not have covariance Sigma dt; for a diagonal
 * Sigma the two coincide.
 *   out        host, [batch][n_paths][n_keep][D]: the grid points k = 0, stride, 2 stride, ... < Np, n_keep = (Np - 1) / stride + 1
 *   x0_or_null host, [batch][D]: every path of problem p starts at x0[p].  NULL: x_0 = m0_p + chol_lower(S0_p) xi_0, from the problem's
 *              own row if vgpa_set_problem_data gave one (VGPA_ERR_STATE for a context created without m0 / s0)
 *   VGPA_PATHS_POSTERIOR: drift_k(x) = -A_k x + b_k of problem p's own x.  x_or_null given (host, [batch][len_x]): uploaded like every
 *              other x; the cached sweep state is dropped.  NULL: the x of the cached evaluation is read and nothing of the cached
 *              state is written -- vgpa_gradient(NULL), vgpa_fetch, vgpa_energy_parts and vgpa_theta_gradient return afterwards bit
 *              for bit what they return without this call (VGPA_ERR_STATE without a cached state)
 *   VGPA_PATHS_MODEL: the model's drift with the theta in force (per-problem rows honoured): OU -theta x (the mu = 0 the energy kernel
 *              assumes), double well 4 x (theta - x^2), Lorenz-63, Lorenz-96 (x_{i+1} - x_{i-2}) x_{i-1} - x_i + theta, circular on each
 *              path's own state vector.  x_or_null must be NULL.
 * The normals are counter-based -- a draw depends on (seed, problem, path, grid index, component) and on nothing else, so a result does
 * not change with the batch size, n_paths or the launch geometry: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
 * (k, path, problem, j) with k the grid index the draw arrives at (0: the initial draw) and j the component pair;
 * u1 = (((r0 >> 5) 2^26 + (r1 >> 6)) + 0.5) 2^-53, u2 likewise from r2, r3, each capped at 1 - 2^-53 (the one rounding of fp64 that
 * would reach 1); xi_2j = sqrt(-2 ln u1) cos(2 pi u2), xi_2j+1 = sqrt(-2 ln u1) sin(2 pi u2) (odd D: the last one is dropped).
 * VGPA_ERR_ARG: n_paths < 1, stride < 1, an unknown kind, a null out, an x for the model kind, the model kind on VGPA_MODEL_NONE;
 * VGPA_ERR_UNSUPPORTED: D > 64; VGPA_ERR_NOT_PD: a Sigma dt (or, for a drawn start, an S0) that has no Cholesky factor. */
enum { VGPA_PATHS_POSTERIOR = 0, VGPA_PATHS_MODEL = 1 };
int vgpa_sample_paths(vgpa_ctx* ctx, int kind, const double* x_or_null, const double* x0_or_null,
                      int32_t n_paths, int32_t stride, uint64_t seed, double* out);

/* The paths of vgpa_sample_paths(VGPA_PATHS_POSTERIOR) with the same arguments -- the same counters, the same recursion -- and, summed where each
 * path is made, the logarithm of its importance weight against the model SDE and the data: what turns draws from the approximation into an
 * estimate of log p(y | theta, Sigma), an effective sample size and reweighted smoothing expectations.  With g = -A_{k-1} x_{k-1} + b_{k-1},
 * f = f_theta(x_{k-1}) the model drift of VGPA_PATHS_MODEL, d = g - f and eta_k = R_p xi_k the step's noise increment, both chains have
 * Gaussian transitions of covariance Sigma dt, and the log-ratio of the discrete path densities is exactly
 *   path term = sum_{k=1}^{Np-1} [ -d^T Sigma^-1 eta_k - dt d^T Sigma^-1 d / 2 ]
 *   obs term  = sum_n [ -(y_n - x_{t_n})^T Q (y_n - x_{t_n}) / 2 ] - the additive constant of E_obs,   Q = H R^-1 H^T (1-D models: 1 / r)
 * with the theta, Sigma, observation times, values, count, R and H in force (per-problem rows honoured).  An observation at grid index 0
 * applies to x_0, one at Np - 1 to the last state.  The third term of log w = init + path + obs,
 *   init term = log N(x_0; mu0, tau0) - log N(x_0; m0, S0)   (0 for a given x0),
 * is the caller's: the prior (mu0, tau0) is not an input of the context, and `start` holds the x_0 it needs.  These are the true Gaussian
 * densities: the reference's quirks in E0 and E_obs are not reproduced, so -mean(log w) is not F (DESIGN.md s.4.9 says which parts differ).
 *   logw          host, [batch][n_paths][2]: the path term, the obs term
 *   start_or_null host, [batch][n_paths][D]: x_0 of every path
 *   out_or_null   as `out` of vgpa_sample_paths; NULL: no path is stored or copied (many paths, a tiny result)
 *   x_or_null, x0_or_null, n_paths, stride, seed: as in vgpa_sample_paths; with x NULL the cached state is read and not written
 * Sigma^-1 is 1 / Sigma_ii: built for an isotropic or diagonal Sigma, shared or per problem.
 * VGPA_ERR_ARG: a null logw, n_paths < 1, stride < 1, VGPA_MODEL_NONE; VGPA_ERR_STATE: an ODE-only context, no cached state with x NULL;
 * VGPA_ERR_UNSUPPORTED: D > 64, a dense Sigma in force; VGPA_ERR_NOT_PD: as in vgpa_sample_paths. */
int vgpa_sample_paths_weighted(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride,
                               uint64_t seed, double* out_or_null, double* start_or_null, double* logw);

/* A guided particle filter with the posterior process as its proposal: the walk of vgpa_sample_paths_weighted with the
 * weights taken in observation by observation and the particle cloud resampled whenever its effective sample size drops.  Per problem p, n =
 * n_paths particles in slots i = 0 .. n-1, each a state x_i and an unnormalised log-weight lw_i:
 *   start    x_i = x0[p], or m0_p + chol_lower(S0_p) xi_0 with the sampler's counter (0, i, p, j);  lw_i = init_i - c_p, c_p the additive
 *            constant of the obs term above, init_i = log N(x_i; mu0, tau0) - log N(x_i; m0, S0) when a prior is passed and the start is
 *            drawn, else 0
 *   steps    k = 1 .. Np-1 as in vgpa_sample_paths_weighted: the same recursion, slot i drawing with counter (k, i, p, j) whatever its
 *            ancestry, the step's path increment added to lw_i
 *   at every observation of the problem (grid index 0 applies to x_0): -(y - x_i)^T Q (y - x_i) / 2 is added to lw_i; then
 *            w_i = exp(lw_i - max lw), S = sum w_i, ESS = S^2 / sum w_i^2, and the cloud is resampled iff ESS < ess_fraction n and k < Np - 1
 *   systematic resampling: U = the first uniform of Philox counter (k, 0, p, 0xffffffff) under the seed's key (the normals use j < 32),
 *            u_i = (U + i) / n S, cum = the inclusive prefix sums of w in slot order, anc_i = min(#{m: cum_m <= u_i}, n - 1);
 *            x_i <- x_{anc_i}, every lw_i <- max lw + log S - log n
 * The mean weight is preserved, so logsumexp(lw) - log n of the final lw estimates log p(y | theta, Sigma) with or without resampling.
 * A problem's schedule depends on its own observation times, count, R, H, theta and Sigma (the rows in force are honoured as above); its
 * result does not change with the batch around it.  It does change with n_paths from the first resampling on.
 *   x_or_null, x0_or_null, n_paths, seed: as in vgpa_sample_paths_weighted; with x NULL the cached state is read and not written
 *   ess_fraction      in [0, 1]; 0: never resample (the weights of vgpa_sample_paths_weighted)
 *   prior_mu_or_null  host, [batch][D], and prior_tau_or_null, host, [batch][D][D]: both or neither
 *   logw    host, [batch][n_paths]: the final lw;  state  host, [batch][n_paths][D]: the final particles
 *   histories over the observation counter j < M (M the context's n_obs), each may be NULL:
 *   ess_or_null [batch][M];  resampled_or_null [batch][M] int32;  ancestors_or_null [batch][M][n_paths] int32 (the identity where the cloud
 *   was carried on);  clouds_or_null [batch][M][n_paths][D]: the states at observation j before the resampling decision.
 *   Rows j at or beyond a problem's own count: ess 0, flag 0, ancestors -1, clouds untouched.
 * VGPA_ERR_ARG: a null logw or state, n_paths < 1, ess_fraction outside [0, 1] or NaN, one prior pointer without the other, VGPA_MODEL_NONE;
 * VGPA_ERR_STATE: an ODE-only context, no cached state with x NULL, a drawn start without m0 / s0; VGPA_ERR_UNSUPPORTED: D > 64, a dense
 * Sigma in force; VGPA_ERR_NOT_PD: as in vgpa_sample_paths, and a prior covariance without a Cholesky factor. */
int vgpa_particle_filter(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed, double ess_fraction,
                         const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* ess_or_null,
                         int32_t* resampled_or_null, int32_t* ancestors_or_null, double* clouds_or_null);

/* The path statistics of the particle filter's lineages: the complete-data sufficient statistics of (theta, Sigma) of the
 * Euler-discretised model, whose weighted mean is, by Fisher's identity, the score and the exact EM step in theta under the smoothing
 * distribution of the particles.  The walk, the counters and the resampling decisions are those of vgpa_particle_filter; every slot i carries
 * a row [3][D] = (Q, G, H) that starts at 0 and to which every step k = 1 .. Np-1 adds, per component j < D,
 *   Q_j += r_j^2 / dt,   G_j += phi_j r_j,   H_j += dt phi_j^2
 *   r = x_k - x_{k-1} - dt f_theta(x_{k-1}) = dt (g - f_theta(x_{k-1})) + eta_k, with the g, f and eta of the weighted walk
 *   phi_j = d f_j / d theta_a(j) at x_{k-1}:  OU -x;  double well 4 x;  Lorenz-63 (y - x, x, -z) for (sigma, rho, beta);  Lorenz-96 1
 *            (5 <= D: H_j = dt (Np - 1) is a constant, written and not summed)
 * At a resampling slot i takes the row of its ancestor, as it takes x.  The observation and initial terms add nothing.  theta, Sigma, the
 * data and the observation model are the rows in force.
 *   stats_or_null  host, [batch][n_paths][3][D]: the final rows, in the order (Q, G, H)
 *   mean_or_null   host, [batch][3][D]: sum_i w_i row_i / sum_i w_i with w_i = exp(lw_i - max lw), reduced on the device
 *   at least one of the two must be given
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments; with x NULL the cached state is read and not written
 * Errors: as vgpa_particle_filter, and VGPA_ERR_ARG when stats and mean are both NULL. */
int vgpa_particle_statistics(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed, double ess_fraction,
                             const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state,
                             double* stats_or_null, double* mean_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* Path events of the particle filter's lineages: what no mean or variance on the grid expresses -- whether a component
 * crossed a level anywhere in the window, when it first did, how long it stayed beyond it and how far it went -- from all n_paths lineages,
 * with only per-problem summaries leaving the device.  The walk, the counters and the resampling decisions are those of vgpa_particle_filter.
 *   levels  host, [batch][D], finite: c[p][j];  sides  host, [batch][D] int32, each +1 or -1: s[p][j]
 *   g_j(x)  = s_j (x_j - c_j): one fp64 subtraction, then an exact change of sign.  Component j of a state is in the event iff g_j(x) > 0
 *   x_i(k)  the state of slot i as the walk arrives at grid index k, before a resampling decision at k (as for vgpa_particle_moments)
 * Every slot i carries a row [3][D] = (X, T, N) of records of its own lineage:
 *   k = 0             X_j = g_j(x_i(0));  T_j = 0 and N_j = 1 if in the event, else T_j = Np (the sentinel: never so far) and N_j = 0
 *   k = 1 .. Np-1     X_j = fmax(X_j, g_j(x_i(k)));  if in the event, T_j = min(T_j, k) and N_j += 1
 * At a resampling slot i takes the row of its ancestor, as it takes x -- also at an observation at grid index 0: the row of k = 0 is set
 * before that decision.  T and N are returned as doubles; they are exact integers.
 *   rows_or_null  host, [batch][n_paths][3][D]: the final rows, in the order (X, T, N)
 *   mean_or_null  host, [batch][3][D]: sum_i w_i row_i / sum_i w_i with w_i = exp(lw_i - max lw), reduced on the device as for
 *                 vgpa_particle_statistics: E[X] the mean extreme of g, E[N] dt the expected occupation time, E[T] with the sentinel in it
 *   cdf_or_null   host, [batch][n_keep][D], n_keep = (Np-1) / stride + 1: the first-passage distribution on the kept grid indices,
 *                 cdf[k'][j] = sum_i W_i 1[T_ij <= k' stride], W_i = w_i / sum w.  Non-decreasing in k' to the bit; two calls with the same
 *                 arguments give the same bits, and a problem's row does not depend on the batch around it
 *   at least one of the three must be given
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments; with x NULL the cached state is read and not written
 * The estimator is that of vgpa_particle_statistics: the final weights on the surviving lineages.  It is exact for the Euler-discretised
 * model as n_paths grows, and in early stretches of the window it rests on the few lineages the genealogy has left there, which
 * lineage_ess of vgpa_particle_moments reports.
 * Errors: as vgpa_particle_filter (D > 64 and a dense Sigma: VGPA_ERR_UNSUPPORTED), and VGPA_ERR_ARG for a NULL levels or sides, a side that
 * is not +1 or -1, a level that is not finite, stride < 1, or rows, mean and cdf all NULL. */
int vgpa_particle_events(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                         double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, const double* levels,
                         const int32_t* sides, double* logw, double* state, double* rows_or_null, double* mean_or_null, double* cdf_or_null,
                         double* ess_or_null, int32_t* resampled_or_null);

/* The smoothing moments on the time grid under the genealogy of the particle filter: E[x_k | y] and E[x_k^2 | y] of the
 * Euler-discretised model as the filter's surviving lineages estimate them, with O(n D) state per problem -- no path is stored or copied.
 * Three steps on the device: the filter of vgpa_particle_filter with its ancestors kept; the final weights pushed backwards through the
 * ancestors; the walk once more from the same counters, reduced where the states are made.
 *   stretches   problem p has its own observation indices t_0 < ... < t_{c-1} in force.  Stretch j = 0 .. c holds the grid indices
 *               t_{j-1} < k <= t_j with t_{-1} = -1 and t_c = Np-1 (stretch c is empty when t_{c-1} = Np-1)
 *   x_i(k)      the state of slot i as the walk arrives at k, before a resampling decision at k
 *   W^c_i       = w_i / sum w,  w_i = exp(lw_i - max lw) of the final log-weights
 *   W^j_a       for j = c-1 .. 0: where the cloud was resampled at observation j with ancestors anc, the sum of W^{j+1}_i over the slots i
 *               with anc_i = a, added in increasing i (anc is non-decreasing: a contiguous run; 0 for a slot without descendant); else W^{j+1}_a
 *   moments          host, [batch][n_keep][2][D], n_keep = (Np-1) / stride + 1: for the kept grid indices k = 0, stride, 2 stride, ... in
 *                    stretch j(k), M1[k][d] = sum_i W^{j(k)}_i x_i(k)[d] and M2[k][d] = sum_i W^{j(k)}_i x_i(k)[d]^2.  The raw moments: the
 *                    variance M2 - M1^2 is the caller's to form.  Two calls with the same arguments give the same bits
 *   lineage_ess_or_null  host, [batch][M+1]: 1 / sum_i (W^j_i)^2 for j = 0 .. c, the number of distinct lineages that carry stretch j's
 *                    estimate in effect; rows beyond a problem's own count + 1: 0
 *   logw, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with the
 *   same arguments.  state is copied behind the second walk and is bit-identical as well: the replay arrived at the filter's particles.
 *   With x NULL the cached state is read and not written
 * Errors: as vgpa_particle_filter, and VGPA_ERR_ARG for a NULL moments or stride < 1; VGPA_ERR_UNSUPPORTED, before any work, for more
 * than 65535 workgroups per problem (256 particles each at D <= 4, 64 above) or more than 2^39 - 256 entries of moments. */
int vgpa_particle_moments(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                          double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state,
                          double* moments, double* lineage_ess_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* The smoothing mean and the full second-moment matrices on the time grid under the genealogy of the particle filter:
 * what vgpa_particle_moments estimates, with every cross moment E[x_k x_k^T | y] in place of its diagonal -- the estimate the matrices S_t of
 * the variational posterior are held against.  The same three steps on the device; the second walk forms, per kept grid index, X diag(W) X^T
 * of the particle states (5 <= D <= 64: on the fp64 matrix cores).  Stretches, x_i(k), W^j_i and the kept grid indices are those of
 * vgpa_particle_moments.
 *   mean             host, [batch][n_keep][D], n_keep = (Np-1) / stride + 1: mean[k][a] = sum_i W^{j(k)}_i x_i(k)[a]
 *   second           host, [batch][n_keep][D][D]: second[k][a][b] = sum_i W^{j(k)}_i x_i(k)[a] x_i(k)[b], the raw moment -- the covariance
 *                    second - mean mean^T is the caller's to form.  One triangle is computed and mirrored: (a, b) and (b, a) hold the same
 *                    bits.  Two calls with the same arguments give the same bits
 *   lineage_ess_or_null  as in vgpa_particle_moments, and bit-identical to its result with the same arguments
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments.  With x NULL the cached state is read and not written
 * Device memory: the workgroups' partial sums take batch * G * n_keep * (D + D (D + 1) / 2) doubles, G = ceil(n_paths / 256) workgroups per
 * problem at D <= 4 and ceil(n_paths / 64) above; their sum batch * n_keep * (D + D (D + 1) / 2), the results batch * n_keep * D (D + 1).
 * The first grows with D^2 and with n_paths: a larger stride is the remedy.
 * Errors: as vgpa_particle_moments, with VGPA_ERR_ARG for a NULL mean or second; VGPA_ERR_UNSUPPORTED, before any work, for more than 65535
 * workgroups per problem or more than 2^39 - 256 entries of second; D > 64 and a dense Sigma are refused as in vgpa_particle_filter. */
int vgpa_particle_covariance(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                             double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state,
                             double* mean, double* second, double* lineage_ess_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* The smoothing marginals on the time grid under the genealogy of the particle filter: the law of x_k[d] | y itself, as a
 * histogram over a ladder of levels per component -- whether it is bimodal, where its quantiles lie, P(x_k[d] > c | y) along the window -- with
 * only the histograms leaving the device.  The steps on the device are those of vgpa_particle_moments; the second walk counts where that one
 * sums.  Stretches, x_i(k), j(k), W^c_i, the ancestors and the kept grid indices are those of vgpa_particle_moments.
 *   levels      host, [batch][D][L], L = n_levels in [1, 63]: the ladder c[p][d][0] < ... < c[p][d][L-1] of component d of problem p, finite,
 *               strictly increasing, the same for every grid index
 *   bin(x)      = #{ l : c_l < x }, fp64 compares alone: x <= c_0 gives bin 0, c_{b-1} < x <= c_b bin b, x > c_{L-1} bin L; a NaN falls into
 *               bin 0.  The index lies in [0, L] by construction and is never computed by arithmetic on x
 *   q_i         = (uint64) trunc(W^c_i 2^62) of the final slots, W^c_i with the very bits vgpa_particle_moments normalises to;  Q^c = q
 *   Q^j_a       for j = c-1 .. 0: where the cloud was resampled at observation j with ancestors anc, the sum of Q^{j+1}_i over the slots i with
 *               anc_i = a, in 64-bit integer arithmetic; else Q^{j+1}_a.  sum_i q_i <= 2^62 (1 + n 2^-53) < 2^64: nothing overflows, and the
 *               truncation loses less than 2^-62 per particle
 *   mass             host uint64, [batch][n_keep][D][L+1], n_keep = (Np-1) / stride + 1: for the kept grid indices k = k' stride in stretch
 *                    j(k), mass[k'][d][b] = sum_i Q^{j(k)}_i 1[bin(x_i(k)[d]) = b].  Integer addition is associative: the result does not
 *                    depend on the launch geometry, the batch or the order of any addition, and equals exactly the histogram of the n final
 *                    lineages' states at k weighted by q_i.  sum_b mass is the same for every d and every kept k of a stretch; the CDF on
 *                    the ladder, cdf[l] = sum_{b <= l} mass[b] / sum_b mass[b], is non-decreasing and lies in [0, 1] by construction
 *   qfinal_or_null   host uint64, [batch][n_paths]: q_i
 *   lineage_ess_or_null  as in vgpa_particle_moments, and bit-identical to its result with the same arguments
 *   logw, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with the
 *   same arguments.  state is copied behind the second walk and is bit-identical as well.  With x NULL the cached state is read and not
 *   written
 * The estimator is that of vgpa_particle_moments: the final weights on the surviving lineages.  It is exact for the Euler-discretised model
 * as n_paths grows, and in early stretches it rests on the few lineages the genealogy has left there, which lineage_ess reports.
 * Errors: as vgpa_particle_moments, and VGPA_ERR_ARG for a NULL levels or mass, n_levels outside [1, 63], a level that is not finite, a ladder
 * that is not strictly increasing (the message names the problem and the component), or stride < 1; VGPA_ERR_UNSUPPORTED, before any work,
 * for more than 65535 workgroups per problem or more than 2^39 - 256 entries of mass; D > 64 and a dense Sigma are refused as in
 * vgpa_particle_filter. */
int vgpa_particle_marginals(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                            double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, const double* levels,
                            int32_t n_levels, double* logw, double* state, uint64_t* mass, uint64_t* qfinal_or_null,
                            double* lineage_ess_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* The two-time moments of the smoothing law under the genealogy of the particle filter: the particle estimate of
 * Cov[x_k, x_s | y] for k != s -- what vgpa_lag_covariance's K(k, s) is held against --, with only the moments leaving the device.
 * The filter, its weights, the stretches and the kept grid indices k = k' stride, n_keep = (Np-1) / stride + 1, are those of
 * vgpa_particle_filter / vgpa_particle_paths.
 *   X_i(k)      the trajectory of final slot i, i = 0 .. n_paths-1: bit for bit the one vgpa_particle_paths returns for n_draw = n_paths and
 *               final_slots = 0 .. n_paths-1 (traced back through the ancestors, walked with the counter word of the slot its lineage sat
 *               in; at an observation index the state before the resampling decision)
 *   W_i         = w_i / sum w, w_i = exp(lw_i - max lw) of the final log-weights
 *   anchors     host int64, [n_anchor]: strictly increasing grid indices in [0, Np), each a multiple of stride; shared by the problems
 *   mean        host, [batch][n_keep][D]:                     mean[k'][a]        = sum_i W_i X_i(k' stride)[a]
 *   cross       host, [batch][n_anchor][n_keep][D][D]:        cross[q][k'][a][b] = sum_i W_i X_i(k' stride)[a] X_i(anchors[q])[b]
 *               (1-D models: [batch][n_anchor][n_keep]); every kept k' is filled, on both sides of the anchor
 *   lineage_ess_or_null  as in vgpa_particle_moments, and bit-identical to its result with the same arguments
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments.  With x NULL the cached state is read and not written
 * Raw moments: the covariance cross - mean[k'] mean[anchor]^T is the caller's subtraction, where its cancellation is visible.  The paths of
 * a problem are added in increasing i whatever the launch: a problem's block does not depend on the batch around it, an anchor's block not
 * on the other anchors, a kept row not on the stride.  The estimator is that of vgpa_particle_statistics: the final weights on the
 * surviving lineages; early stretches rest on the few lineages the genealogy has left there, which lineage_ess reports.
 * Memory: the trajectories stay on the device, batch n_paths n_keep D doubles; the stride is the lever.
 * Errors: as vgpa_particle_paths, and VGPA_ERR_ARG for a NULL mean, cross or anchors, n_anchor < 1, an anchor out of range, anchors not
 * strictly increasing or an anchor that is no multiple of stride; VGPA_ERR_UNSUPPORTED, before any work, beyond the limits of
 * vgpa_particle_paths with n_draw = n_paths, for more than 65535 anchors or problems, or more than 2^39 - 256 entries of cross; D > 64 and
 * a dense Sigma are refused as in vgpa_particle_filter. */
int vgpa_particle_lag_covariance(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                                 double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, int32_t n_anchor,
                                 const int64_t* anchors, double* logw, double* state, double* mean, double* cross, double* lineage_ess_or_null,
                                 double* ess_or_null, int32_t* resampled_or_null);

/* The contraction of vgpa_particle_lag_covariance alone, on trajectories and weights of the caller: for paths drawn
 * otherwise -- vgpa_particle_backward_paths' equally weighted draws, vgpa_sample_paths_weighted's paths with their weights.
 *   paths            host, [batch][n_paths][n_keep][D]
 *   weights_or_null  host, [batch][n_paths], used as given (their normalisation is the caller's); NULL: 1 / n_paths each
 *   anchor_rows      host int32, [n_anchor]: rows of the kept axis, each in [0, n_keep); any order, repeats allowed
 *   mean             host, [batch][n_keep][D]:               mean[k][a]        = sum_i W_i X_i(k)[a]
 *   cross            host, [batch][n_anchor][n_keep][D][D]:  cross[q][k][a][b] = sum_i W_i X_i(k)[a] X_i(anchor_rows[q])[b]
 * Every term is fma(X_i(k)[a], W_i X_i(r)[b], .), the paths in increasing i.  Works on any context with D <= 64 (batch and D are the
 * context's), ODE-only and VGPA_MODEL_NONE included; reads nothing of the cached state and writes nothing to it.
 * Errors: VGPA_ERR_ARG for a NULL paths, anchor_rows, mean or cross, a count below 1 or a row out of range; VGPA_ERR_UNSUPPORTED for
 * D > 64, more than 2^35 entries of paths, more than 65535 anchors or problems, or more than 2^39 - 256 entries of cross. */
int vgpa_path_cross_moments(vgpa_ctx* ctx, const double* paths, const double* weights_or_null, int32_t n_paths, int32_t n_keep, int32_t n_anchor,
                            const int32_t* anchor_rows, double* mean, double* cross);

/* Whole smoothing trajectories on the time grid, drawn from the genealogy of the particle filter: K = n_draw complete
 * paths of the Euler-discretised model as the filter's surviving lineages hold them, for path functionals that are no mean or variance.
 * Three steps on the device behind the filter of vgpa_particle_filter, which runs unchanged with its ancestors kept: the final slots; their
 * genealogy; one walk of the K trajectories alone.  The normals are counter-based and the state update is one instruction sequence, so a
 * lineage is re-walked by a single lane that draws with the counter word of the slot the lineage sat in; nothing else is replayed.
 *   stretches   as in vgpa_particle_moments: problem p has its own observation indices t_0 < ... < t_{c-1} in force; stretch j = 0 .. c
 *               holds the grid indices t_{j-1} < k <= t_j with t_{-1} = -1 and t_c = Np-1
 *   s_c[m]      the final slots, m = 0 .. K-1: final_slots_or_null (host int32, [batch][K], each in [0, n_paths)), or drawn by systematic
 *               resampling from the final weights: w_i = exp(lw_i - max lw), cum = the inclusive prefix sums in slot order (associated as
 *               the filter's resampling step associates them), S = cum_{n-1}, U = the first uniform of Philox counter (Np, 0, p, 0xffffffff)
 *               under the seed's key (the filter draws with grid indices <= Np-1), u_m = (U + m) / K S,
 *               s_c[m] = min(#{i: cum_i <= u_m}, n_paths-1).  Drawn trajectories are equally weighted; given ones carry the weights of
 *               their final slots, which are the caller's to apply
 *   s_j[m]      for j = c-1 .. 0: anc_j[s_{j+1}[m]] where the cloud was resampled at observation j, else s_{j+1}[m]
 *   the walk    trajectory m starts at x0[p], or at m0_p + chol_lower(S0_p) xi_0 drawn with counter (0, s_0[m], p, .), and runs the
 *               posterior recursion of vgpa_sample_paths(VGPA_PATHS_POSTERIOR) for k = 1 .. Np-1, the step to k drawing with counter
 *               (k, s_{j(k)}[m], p, .), j(k) the stretch of k (an observation at grid index 0 makes stretch 0 the single index 0)
 *   paths            host, [batch][K][n_keep][D], n_keep = (Np-1) / stride + 1, in the layout and with the stride of vgpa_sample_paths.
 *                    At stride 1, paths[p][m][t_j] is bit for bit the filter's clouds[p][j][s_j[m]] and paths[p][m][Np-1] is bit for bit
 *                    state[p][s_c[m]].  On collapsing clouds the early stretches of all K trajectories coincide (the rows of slots say so)
 *   slots_or_null    host int32, [batch][M+1][K]: s_j[m] for j = 0 .. c; rows beyond a problem's own count + 1: -1
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments.  K > n_paths is legal.  With x NULL the cached state is read and not written
 * Errors: as vgpa_particle_filter, and VGPA_ERR_ARG for n_draw < 1, a NULL paths, stride < 1 or a given slot outside [0, n_paths);
 * VGPA_ERR_UNSUPPORTED, before any work, for more than 65535 * 64 trajectories per problem above D = 4 (2^31 - 1 workgroups of 256 lanes
 * over the batch at D <= 4) or more than 2^35 entries of paths. */
int vgpa_particle_paths(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t n_draw,
                        const int32_t* final_slots_or_null, int32_t stride, uint64_t seed, double ess_fraction,
                        const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* paths,
                        int32_t* slots_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* Whole smoothing trajectories by backward simulation (forward filtering, backward simulation): the K trajectories of
 * vgpa_particle_paths, but at every observation where the cloud was resampled a trajectory does not follow its ancestor: it draws the slot
 * it came from among all n = n_paths particles of the filter's stored cloud, with probability proportional to (filter weight) x (model
 * transition density to the trajectory's next state).  The early stretches then do not rest on the few lineages that survive the
 * resamplings.  Lineages coalesce at the resampling steps only -- inside a stretch every slot carries its own path -- so the block state
 * z_j = x_{t_{j-1}+1 .. t_j} is backward-simulated: p(z_{j+1} | z_j) depends on z_j through x_{t_j} alone and on z_{j+1} through its first
 * point alone, one transition density per candidate and cut.
 * Stretches, t_j, c, x_i(k), clouds_j, anc_j, the resampling flags and the final slots s_c[m] (given, or drawn with the same counter) are
 * those of vgpa_particle_paths; the filter of vgpa_particle_filter runs unchanged.  Two more quantities:
 *   hlw_j[i]    the log-weight of slot i at the problem's observation j, that observation's term included, before the resampling decision
 *   R_dd        the diagonal factor of Sigma_p dt in force
 * For j = c-1 .. 0, per problem p and trajectory m:
 *   not resampled at observation j:  s_j[m] = s_{j+1}[m]
 *   resampled (so k = t_j < Np-1):
 *     1. x~ = (z + dt (-A_k z + b_k)) + R xi with z = clouds_j[anc_j[s]], s = s_{j+1}[m], xi the sampler's normals of counter (k+1, s, p, .):
 *        the state of slot s at grid index k+1, recomputed in plain fp64 -- equal to the walk's to rounding, not necessarily to the bit
 *        (above D = 4 the walk forms A z on the matrix cores)
 *     2. b_i = hlw_j[i] - 1/2 sum_d ((x~_d - mu_i,d) / R_dd)^2 for every slot i < n, mu_i = clouds_j[i] + dt f(clouds_j[i]; theta_p), f the
 *        model drift of vgpa_sample_paths(VGPA_PATHS_MODEL) with the theta in force (Lorenz-96 circular on the candidate's own state);
 *        the device multiplies by 1 / R_dd
 *     3. g_i = -log(-log u_i), u_i from Philox counter (k, m, p, 0x80000000 | (i >> 1)) under the seed's key: unit_open(r0, r1) for even
 *        i, unit_open(r2, r3) for odd i (the normals use fourth words below 32, the resamplings 0xffffffff: no collision while n < 2^32)
 *     4. s_j[m] = the smallest i that attains max_i (b_i + g_i): Gumbel-max, an exact draw from softmax(b), without a prefix sum -- the
 *        result depends on no summation order and not on the launch geometry
 *   the walk    as in vgpa_particle_paths: the start with counter word s_0[m], the step to k in stretch j with counter (k, s_j[m], p, .);
 *               and having completed an observation index t_j of its problem, after that point is stored, the state is replaced by
 *               clouds_j[anc_j[s_{j+1}[m]]] before the next step (where the cloud was carried on anc_j is the identity: no bit changes)
 *   paths            host, [batch][K][n_keep][D] as in vgpa_particle_paths.  At stride 1, paths[p][m][t_j] is bit for bit
 *                    clouds[p][j][s_j[m]] and paths[p][m][Np-1] is bit for bit state[p][s_c[m]].  Drawn trajectories are equally weighted.
 *                    With ess_fraction = 0, or n_paths = 1, nothing is resampled and paths and slots are vgpa_particle_paths' bit for bit.
 *                    Two calls with the same arguments give the same bits
 *   slots_or_null    host int32, [batch][M+1][K]: s_j[m]; rows beyond a problem's own count + 1: -1
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments.  With x NULL the cached state is read and not written
 * Within a stretch a trajectory is still its slot's own path: the distinct paths of a stretch are bounded by the distinct slots drawn.
 * Device memory: the two histories the draw reads stay on the device for the call, batch * M * n * (D + 1) doubles (the clouds and hlw),
 * beside the ancestors (batch * M * n int32) that vgpa_particle_paths keeps.  Work: n * K scores of D terms per resampled observation.
 * Errors and limits: those of vgpa_particle_paths (D > 64 and a dense Sigma are VGPA_ERR_UNSUPPORTED), and VGPA_ERR_UNSUPPORTED, before
 * any work, for more than 65535 * 8 trajectories per problem. */
int vgpa_particle_backward_paths(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t n_draw,
                                 const int32_t* final_slots_or_null, int32_t stride, uint64_t seed, double ess_fraction,
                                 const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* paths,
                                 int32_t* slots_or_null, double* ess_or_null, int32_t* resampled_or_null);

/* The smoothing moments on the time grid under the marginal backward smoother (Doucet, Godsill & Andrieu 2000): what
 * vgpa_particle_moments estimates, with the weights of every stretch taken from all n = n_paths particles of the filter's stored clouds and
 * not from the lineages that survive the resamplings -- the expectation of the draw vgpa_particle_backward_paths makes, with its block-state
 * argument: one n x n table of transition densities per resampled observation.  Stretches, t_j, c, x_i(k), clouds_j, anc_j, hlw_j, R_dd and
 * the resampling flags are those of vgpa_particle_backward_paths; the filter of vgpa_particle_filter runs unchanged.  Per problem p:
 *   W^c_i       = w_i / sum w,  w_i = exp(lw_i - max lw) of the final log-weights: vgpa_particle_moments' first row, bit for bit
 *   W^j         for j = c-1 .. 0, not resampled at observation j: W^{j+1}
 *               resampled (so k = t_j < Np-1), for every successor slot s < n and candidate i < n:
 *     1. x~_s = (z + dt (-A_k z + b_k)) + R xi with z = clouds_j[anc_j[s]], xi the sampler's normals of counter (k+1, s, p, .): step 1 of
 *        vgpa_particle_backward_paths with s in place of s_{j+1}[m], in plain fp64
 *     2. b_{s,i} = hlw_j[i] - 1/2 sum_d ((x~_{s,d} - mu_{i,d}) / R_dd)^2, mu_i = clouds_j[i] + dt f(clouds_j[i]; theta_p): step 2 there; the
 *        device multiplies by 1 / R_dd, and for Lorenz-96 with D >= 5 it evaluates the sum as (|a_s|^2 + |m_i|^2) - 2 <a_s, m_i> with
 *        a = (x~ - c) / R, m = (mu - c) / R and c the mean of clouds_j, the cross term on the fp64 matrix cores (equal
 *        within the rounding bound of the scores)
 *     3. P_{s,i} = exp(b_{s,i} - max_i b_{s,i}) / sum_i exp(b_{s,i} - max_i b_{s,i})
 *     4. W^j_i = sum_s W^{j+1}_s P_{s,i}, the terms added in an order n alone fixes: no atomics, nothing that depends on the launch
 *   With the indicator i = anc_j[s] in place of P this is vgpa_particle_moments' recursion; nothing else differs from that call.
 *   moments          host, [batch][n_keep][2][D] as in vgpa_particle_moments: M1[k][d] = sum_i W^{j(k)}_i x_i(k)[d] and M2 likewise, by the
 *                    same second walk.  With ess_fraction = 0, or n_paths = 1, nothing is resampled and moments are vgpa_particle_moments'
 *                    bit for bit.  Two calls with the same arguments give the same bits, and a problem's results do not depend on the
 *                    batch around it
 *   smoothing_ess_or_null  host, [batch][M+1]: 1 / sum_i (W^j_i)^2 for j = 0 .. c (at a carried cut: the entry of j + 1); rows beyond a
 *                    problem's own count + 1: 0, as lineage_ess of vgpa_particle_moments
 *   weights_or_null  host, [batch][M+1][n]: W^j_i, downloaded only when asked for; rows beyond a problem's own count + 1: 0
 *   logw, state, ess_or_null, resampled_or_null and every other argument: as in vgpa_particle_filter, and bit-identical to its results with
 *   the same arguments.  With x NULL the cached state is read and not written
 * Where the particles of a cloud lie many transition widths apart (the Lorenz-96 fixtures) P is one-hot on the ancestor and the result is
 * vgpa_particle_moments': the gain is on clouds that overlap, the 1-D and 3-D models with many observations.  It is no cure
 * for a filter that has lost the posterior: the clouds are the filter's.
 * Device memory: the histories of vgpa_particle_backward_paths, batch * M * n * (D + 1) doubles, the table batch * (M+1) * n, and batch *
 * (n * (D + 2) + 64 + (M+1) * ceil(n / 64)) of work space (the successors, their (max, sum), the centre, the partial sums of W^2); the n x n table of a cut is never stored.  Work: 2 n^2 scores of D terms per resampled observation.
 * Errors and limits: those of vgpa_particle_moments and of vgpa_particle_backward_paths (D > 64 and a dense Sigma are VGPA_ERR_UNSUPPORTED),
 * and VGPA_ERR_UNSUPPORTED, before any work, for more than 65535 * 16 particles per problem or more than 65535 * 256 / D. */
int vgpa_particle_backward_moments(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed,
                                   double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state,
                                   double* moments, double* smoothing_ess_or_null, double* weights_or_null, double* ess_or_null,
                                   int32_t* resampled_or_null);

/* hlw_j of the last vgpa_particle_backward_paths or vgpa_particle_backward_moments call on this context, as its kernels read them: the
 * log-weights its resamplings replaced.  What a caller needs, beside vgpa_particle_filter's ancestors and clouds, to recompute a backward
 * table on the host from the device's own histories.
 *   n_paths     that call's n_paths
 *   hlw         host, [batch][M][n_paths]: hlw_j[i] where the cloud of the problem's observation j was resampled; NaN in every other row
 * Errors: VGPA_ERR_ARG for a NULL hlw; VGPA_ERR_STATE unless the last call on this context that ran the particle filter (every
 * vgpa_particle_* entry point but a vgpa_particle_forecast from a given cloud) was one of the two, succeeded and had this n_paths.  Calls
 * that run no filter -- vgpa_path_cross_moments, the forecast from a given cloud, the sweeps -- leave these histories as they are, and
 * the accessor goes on returning them.  Reads nothing of the cached state and writes nothing to it. */
int vgpa_particle_replaced_logw(vgpa_ctx* ctx, int32_t n_paths, double* hlw);

/* The conditional particle filter with ancestor sampling: one sweep of particle Gibbs (Andrieu, Doucet & Holenstein 2010;
 * Lindsten, Jordan & Schoen 2014).  Given a reference trajectory per problem it returns a new trajectory whose law leaves the smoothing
 * distribution of the Euler-discretised model invariant for any n_paths >= 2 and any proposal (A_t, b_t).  It is vgpa_particle_filter with
 * the same seed and counters -- the stretches, t_j, c, the walk, the observation terms, ESS, the decision and lw_new are those -- but for:
 *   start     slot 0 of every problem is x_0 = ref[p][0] (also with x0 given); its lw is the start's formula at that state (init evaluated at
 *             ref[p][0] for a drawn start under a prior, else 0; minus c_p).  Slots 1 .. n-1 are the filter's
 *   steps     slots >= 1: the filter's, the same counters and bits.  Slot 0 draws nothing.  At step k it holds x_{k-1} = ref[p][k-1]; with
 *             g = -A_{k-1} x_{k-1} + b_{k-1} and f = f_theta(x_{k-1}) as every slot forms them, d = g - f, it takes the implied increment
 *               eta* = (ref[p][k] - ref[p][k-1]) - dt g
 *             in the place of R xi: lw_0 += -sum_i d_i (eta*_i + dt d_i / 2) / Sigma_ii, then the observation term at x = ref[p][k]; its
 *             state becomes ref[p][k] as given, not as recomputed: slot 0 follows the reference bit for bit
 *   at an observation j (k = t_j) where the cloud is resampled (ESS over all n slots, slot 0 included; k < Np-1):
 *             slots i >= 1  multinomial: anc_i = min(#{m: cum_m <= u_i S}, n - 1), u_i the first uniform of Philox counter (k, i, p, 0xfffffffe),
 *                           cum and S the filter's prefix sums.  (One forced slot of a systematic resampling is no valid conditional
 *                           resampling -- Chopin & Singh 2015 --; independent draws are.)
 *             slot 0        ancestor sampling against x~ = ref[p][k+1]: for every candidate i = 0 .. n-1, slot 0 itself included,
 *                           b_i = lw_i - 1/2 sum_d ((x~_d - mu_i,d) / R_dd)^2, lw_i before the reset, mu_i = x_i + dt f(x_i; theta_p), R_dd the
 *                           diagonal factor of Sigma_p dt (the device multiplies by 1 / R_dd); g_i = -log(-log u_i), u_i from Philox
 *                           counter (k, 0, p, 0x40000000 | (i >> 1)): unit_open(r0, r1) for even i, unit_open(r2, r3) for odd i;
 *                           anc_0 = the smallest i that attains max_i (b_i + g_i)
 *             x_i <- x_{anc_i} for i >= 1; x_0 stays (the reference's state): anc_0 goes into the ancestors' history alone;
 *             every lw_i <- max lw + log S - log n.  Where the cloud is carried on, anc is the identity
 *   the trajectory  s_c = the final slot by the rule of vgpa_particle_paths with n_draw = 1 (U from counter (Np, 0, p, 0xffffffff)),
 *             s_j = anc_j[s_{j+1}] where resampled, else s_{j+1}.  In stretch j with s_j != 0 the trajectory is the walk of
 *             vgpa_particle_backward_paths on this run's clouds and ancestors (the start with counter word s_0; behind the completed
 *             observation j-1 it goes on from clouds_{j-1}[anc_{j-1}[s_j]], the reference's state where that ancestor is slot 0); in a
 *             stretch with s_j = 0 it is ref[p][k], copied
 *   ref         host, [batch][Np][D]: the reference trajectory of every problem on the whole grid (stride 1)
 *   trajectory  host, [batch][Np][D].  Bit for bit: trajectory[p][k] = ref[p][k] wherever the slot of k's stretch is 0;
 *               trajectory[p][t_j] = clouds[p][j][s_j]; trajectory[p][Np-1] = state[p][s_c]; clouds[p][j][0] = ref[p][t_j]; with n_paths = 1
 *               the trajectory is ref.  With ess_fraction = 0 state and logw of the slots >= 1 are vgpa_particle_filter's bit for bit.
 *               Two calls with the same arguments give the same bits
 *   slots_or_null  host int32, [batch][M+1]: s_j for j = 0 .. c; rows beyond a problem's own count + 1: -1
 *   logw, state, ess_or_null, resampled_or_null, ancestors_or_null, clouds_or_null: as in vgpa_particle_filter, of this run
 *   x_or_null, x0_or_null, n_paths, seed, ess_fraction, the prior: as in vgpa_particle_filter; with x NULL the cached state is read and not
 *   written
 * Errors and limits: those of vgpa_particle_paths with n_draw = 1 (D > 64 and a dense Sigma are VGPA_ERR_UNSUPPORTED, an ODE-only context
 * VGPA_ERR_STATE, VGPA_MODEL_NONE VGPA_ERR_ARG), and VGPA_ERR_ARG for a NULL ref or trajectory.  The context stays usable. */
int vgpa_particle_conditional(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, const double* ref, int32_t n_paths,
                              uint64_t seed, double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null,
                              double* logw, double* state, double* trajectory, int32_t* slots_or_null, double* ess_or_null,
                              int32_t* resampled_or_null, int32_t* ancestors_or_null, double* clouds_or_null);

/* The particle forecast: a weighted cloud carried past the window under the model SDE, with its mean and spread on the
 * forecast grid and a handful of member trajectories; the cloud never leaves the device between the filter and the forecast.
 * Per problem p: n = n_paths particles x_i with log-weights lw_i at the absolute grid index k0.
 *   forecast steps   for h = 1 .. H (= horizon):  x_i <- (x_i + dt f(x_i; theta_p)) + R_p,jj xi_j,  R_p = chol_lower(Sigma_p dt), Sigma diagonal.
 *               f is the model drift of vgpa_sample_paths(VGPA_PATHS_MODEL) (Lorenz-96 circular on the particle's own state above D = 4),
 *               theta_p and Sigma_p the ones in force; the normals come from Philox counter (k0 + h, i, p, j) under the seed's key: the
 *               samplers' generator, the absolute grid index continuing past the window; the association is the one shown.  No
 *               observations, no resampling: the weights do not change
 *   kept steps  h = 0, stride, 2 stride, ... <= H: h_keep = H / stride + 1.  H = 0 is legal
 *   moments          host, [batch][h_keep][2][D]: M1 = sum_i W_i x_i and M2 = sum_i W_i x_i^2 at the kept steps, W_i = w_i / sum w with
 *                    w_i = exp(lw_i - max lw).  The raw moments, as in vgpa_particle_moments.  Two calls with the same arguments give the
 *                    same bits
 *   members_or_null  host, [batch][K][h_keep][D], K = n_draw >= 0: the trajectories of the slots s[m] in the layout of vgpa_sample_paths.
 *                    s = final_slots_or_null (host int32, [batch][K], each in [0, n)), or drawn by the rule of vgpa_particle_paths:
 *                    systematic resampling from lw with U from counter (k0 + 1, 0, p, 0xffffffff).  Member m draws with the counter word
 *                    of its slot: it is bit for bit what slot s[m] of the whole cloud does.  Behind the filter (k0 = Np-1) with the same
 *                    arguments, member m at h = 0 is bit for bit the last point of trajectory m of vgpa_particle_paths, which the
 *                    forecast continues
 *   slots_or_null    host int32, [batch][K]: s[m]
 *   state_end_or_null  host, [batch][n][D]: the cloud at k0 + H
 *   the cloud   cloud_or_null NULL: the filter of vgpa_particle_filter runs unchanged on x_or_null, x0_or_null, n_paths, seed, ess_fraction
 *               and the prior; logw, state, ess_or_null, resampled_or_null are bit-identical to that entry point's; its final particles
 *               are taken from the device buffer they are in, and k0 = Np-1.  With x NULL the cached state is read and not written.
 *               Otherwise cloud_or_null (host, [batch][n][D]), cloud_logw_or_null (host, [batch][n]; NULL: equal weights) and
 *               index0 >= 0 (= k0) give them: no filter runs; x, x0, ess_fraction, the prior, logw, state, ess and resampled are not
 *               touched, no cached evaluation is needed, and the context needs a stochastic model with theta, Sigma and dt only.
 *               A forecast of H steps equals one of H1 steps followed by one of H - H1 steps from its state_end with index0 + H1: the
 *               states are equal bit for bit
 * Errors: VGPA_ERR_ARG for a context without a stochastic model, horizon < 0, stride < 1, n_paths < 1, a NULL moments, n_draw < 0,
 * index0 < 0, a given slot outside [0, n), or k0 + H (slots drawn: k0 + 1) beyond 2^31 - 1; VGPA_ERR_UNSUPPORTED, before any work, for
 * D > 64, a dense Sigma in force, more than 65535 workgroups per problem (256 particles or members each at D <= 4, 64 above), more than
 * 2^39 - 256 entries of moments or more than 2^35 entries of members; the filter's errors as in vgpa_particle_filter. */
int vgpa_particle_forecast(vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed,
                           double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null,
                           const double* cloud_or_null, const double* cloud_logw_or_null, int32_t index0, int32_t horizon, int32_t stride,
                           int32_t n_draw, const int32_t* final_slots_or_null, double* logw, double* state, double* ess_or_null,
                           int32_t* resampled_or_null, double* moments, double* members_or_null, int32_t* slots_or_null,
                           double* state_end_or_null);

/* device-pointer variants (x, g on the context's device; f written to HOST after a sync) ------ */
int vgpa_sweep_dev(vgpa_ctx* ctx, const double* x_dev, double* f_host, double* g_dev);
int vgpa_free_energy_dev(vgpa_ctx* ctx, const double* x_dev, double* f_host);
/* enqueue-only form for benchmarking / pipelining: F stays on the device (vgpa_fetch_f). */
int vgpa_sweep_enqueue(vgpa_ctx* ctx, const double* x_dev, double* g_dev);
int vgpa_fetch_f(vgpa_ctx* ctx, double* f_host);    /* syncs, checks the device status word */

/* vgpa_energy plus the two hyper-parameter members of <model>.energy()'s return tuple, which the reference computes but
 * nothing consumes (ornstein_uhlenbeck.py:222-226, double_well.py:250-254, lorenz_63.py:329-342, lorenz_96.py:421-434).
 * dEsde_dth: [B] (OU, DW), [B][3] (L63), [B][D] (L96); dEsde_dsig: [B] (1-D) or [B][D][D]; both NULL or both given
 * (D <= 64).  Every output may be NULL. */
int vgpa_energy_full(vgpa_ctx* ctx, const double* lin_a, const double* off_b, const double* mt, const double* st,
                     double* Esde, double* Efx, double* Edf, double* dEsde_dm, double* dEsde_ds,
                     double* dEsde_dth, double* dEsde_dsig);

/* gradient from the cached state into a DEVICE buffer (df(x) of SCG, src/numerics/optim_scg.py:100,235) */
int vgpa_gradient_dev(vgpa_ctx* ctx, double* g_dev);
/* LIFETIME of x_dev: the *_dev entry points consume the caller's x in place (zero copy) and the cached state keeps
 * referring to it -- vgpa_gradient_dev / vgpa_gradient(NULL) read A_t, b_t from that memory.  The caller keeps x_dev
 * alive and unchanged until the next evaluation, or calls vgpa_release_x before freeing / overwriting it: the cached
 * state is then dropped and a gradient request without x fails with VGPA_ERR_STATE instead of reading freed memory.
 * (vgpa_dev_free of the very pointer does the same by itself.) */
int vgpa_release_x(vgpa_ctx* ctx);

/* device-resident vector algebra for the SCG driver (src/numerics/optim_scg.py:75-285):
 * x, d and the gradients stay in HBM, only scalars return.  Every vector is the context's batch of `batch` segments of
 * `seglen` doubles (seglen = len(x) of one problem for SCG); results / coefficients are host arrays of `batch` doubles,
 * one per problem, so that `batch` independent optimisations advance in lock step.  Deterministic reductions. */
int vgpa_vec_dot(vgpa_ctx* ctx, const double* a_dev, const double* b_dev, uint64_t seglen, double* out_host);
int vgpa_vec_absmax(vgpa_ctx* ctx, const double* a_dev, uint64_t seglen, double* out_host);
int vgpa_vec_asum(vgpa_ctx* ctx, const double* a_dev, uint64_t seglen, double* out_host);
/* out = alpha[p]*x + beta[p]*y per problem p; y/beta may be NULL (out = alpha*x); out may alias x or y; a zero
 * coefficient drops its operand entirely (0*inf = 0), which is how finished problems are frozen */
int vgpa_vec_axpby(vgpa_ctx* ctx, uint64_t seglen, const double* alpha_host, const double* x_dev,
                   const double* beta_host_or_null, const double* y_dev_or_null, double* out_dev);

/* tuning knobs (tests / benchmarks); returns VGPA_ERR_ARG for an unknown option or a value out of range */
enum vgpa_option {
  VGPA_OPT_LD_CHUNK = 1        /* grid points per chunk of the time-chunked large-D sweep (>= 1) */
};
int vgpa_set_option(vgpa_ctx* ctx, int option, int64_t value);
/* E0 = KL(q0||p0): constant in x, but the reference recomputes it from the prior's current attributes on EVERY free_energy
 * call (src/var_bayes/variational.py:185; prior_kl0.py:30-92 reads self.mu0 / self.tau0) -- the host mirror hands the
 * current value over before each objective call instead of baking it into the context. */
int vgpa_set_prior_energy(vgpa_ctx* ctx, double e0);   /* sets every problem of the batch to e0 */
/* Per-problem inputs of a batched context.  Each pointer may be NULL (= the shared value from vgpa_config): every call states
 * the whole set, so a NULL also takes back what an earlier call set for that input.
 *   obs_t [batch][M]      observation indices, each row strictly increasing in [0, Np); M is the context's n_obs
 *   obs_y [batch][M][D]   observation values
 *   m0    [batch][D]      initial mean
 *   s0    [batch][D][D]   initial covariance
 *   e0    [batch]         KL(q0||p0) of each problem
 * Rows that all equal the shared observation times keep the shared-time kernels.  On the 16-lane kernels (2 <= D <= 4, fewer than
 * 512 problems) per-problem times take dense jump arrays of batch * Np * (D + D*D) doubles.
 * Drops the cached state, like vgpa_release_x.  The additive constant of E_obs depends on M and R only and stays shared
 * (vgpa_set_problem_obs_model makes it per problem).  With per-problem observation counts in force only the first n_obs[p] entries of
 * problem p's obs_t / obs_y row are validated and read; with none in force every row is validated whole.  The context keeps a host
 * copy of the obs_t rows, so this call and vgpa_set_problem_obs_model give the same state in either order.
 * VGPA_ERR_ARG: an obs_t row out of order or out of range; VGPA_ERR_STATE: an ODE-only context; VGPA_ERR_UNSUPPORTED:
 * per-problem obs_t at D > 64, and any per-problem data in the time-chunked large-D sweep.  A non-positive-definite s0 row
 * is reported by the sweep (VGPA_ERR_NOT_PD), as a shared one is.  vgpa_solve_fwd keeps its explicit m0 / s0. */
int vgpa_set_problem_data(vgpa_ctx* ctx, const int64_t* obs_t, const double* obs_y, const double* m0, const double* s0,
                          const double* e0);
/* Per-problem drift parameters and system noise of a batched context, for parameter studies (one dataset at many (theta, Sigma)
 * points in one context).  theta: [batch][n_theta]; sigma: [batch][D][D] (1-D models: [batch]).  NULL keeps vgpa_config's value;
 * like vgpa_set_problem_data every call states the whole set, and neither call resets what the other one set.  Sigma^-1 of each
 * row is computed as vgpa_create computes the shared one.  The kernel family (diagonal / isotropic Sigma, symmetric inputs) is the
 * one every row allows; rows that all equal the shared parameters keep the shared kernels.  Drops the cached state.
 * Seen by the fused objective (free_energy, gradient, sweep, sweep_enqueue), vgpa_energy_parts, vgpa_fetch (VGPA_FETCH_PSIT
 * included) and the operator-level vgpa_energy / vgpa_energy_full (whose dEsde_dth / dEsde_dsig are then per problem).
 * VGPA_ERR_ARG: a 1-D sigma row <= 0; VGPA_ERR_NOT_PD: a Sigma row that is not positive definite (the message names the row; the
 * previous parameters stay in force after either); VGPA_ERR_STATE: an ODE-only context; VGPA_ERR_UNSUPPORTED: per-problem Sigma
 * at D > 64, and any per-problem parameter in the time-chunked large-D sweep. */
int vgpa_set_problem_params(vgpa_ctx* ctx, const double* theta, const double* sigma);
/* Per-problem observation model of a batched context.  Each pointer may be NULL (= vgpa_config's value); every call states the whole set.
 *   n_obs     [batch]        observations of problem p: 1 <= n_obs[p] <= M (M = vgpa_config.n_obs, now the CAPACITY of a row)
 *   obs_noise [batch][D][D]  R_p   (1-D models: [batch])
 *   obs_h     [batch][D][D]  H_p   (1-D models: NULL only)
 * Problem p uses entries 0 .. n_obs[p] - 1 of its obs_t / obs_y row (the shared row or its own one of vgpa_set_problem_data); the entries
 * from n_obs[p] on are never read and never validated -- callers may leave anything there (-1, NaN).  vgpa_set_problem_data validates
 * the prefixes the counts in force select; a call here that lengthens a prefix onto an invalid stored entry fails with VGPA_ERR_ARG.
 * Q = H R^-1 H^T, K, diag R^-1, the constant matrix jump H^T R^-1 H / 2 (whole and as a packed lower triangle) and the additive
 * constant of E_obs, which depends on n_obs[p] and R_p, become per problem; each row's are computed on the host as vgpa_create
 * computes the shared ones.  The kernel family is the one every row allows: diagonal R with H = I in every row takes the diagonal
 * observation kernels, anything else the dense ones.  Rows that all equal the shared values (counts all M, R rows bit-equal to R, H
 * rows bit-equal to H or NULL) keep the shared kernels and buffers: bit-identical to a context that never made the call.  Differing
 * counts take a per-problem observation index map [batch][Np] even with shared times; on the 16-lane kernels (2 <= D <= 4, fewer than
 * 512 problems) that is the dense-jump path of per-problem times, and the lane-per-problem kernels take the map for every per-problem model.
 * Drops the cached state.  Seen by the fused objective (free_energy, gradient, sweep, sweep_enqueue), vgpa_energy_parts, vgpa_fetch,
 * vgpa_theta_gradient and vgpa_obs_energy.  The reference's E_obs is kept per problem, its quirk included: the covariance diagonal of
 * observation n is taken at grid index n.
 * VGPA_ERR_ARG: a count outside [1, M], a 1-D obs_noise <= 0, an obs_h on a 1-D model; VGPA_ERR_NOT_PD: an R row that is not positive
 * definite (the message names the row); the previous model stays in force after either.  n_obs[p] = 0 is an error on purpose: the
 * multi-dimensional reference cannot evaluate it.  VGPA_ERR_STATE: an ODE-only context; VGPA_ERR_UNSUPPORTED: D > 64 (the time-chunked
 * sweep included; the row-sharded drivers have no such entry point). */
int vgpa_set_problem_obs_model(vgpa_ctx* ctx, const int32_t* n_obs, const double* obs_noise, const double* obs_h);
/* 1 if the context runs the time-chunked large-D sweep (VGPA_FLAG_STREAM_LARGE_D or chosen for lack of memory) */
int vgpa_is_streaming(vgpa_ctx* ctx);

/* Which kernels the context's fused sweep runs and what its device buffers hold right now -- for TESTS AND DIAGNOSTICS: a test
 * that names a kernel path asserts here that it is on it.  Read-only: the call changes nothing, launches nothing, and nothing on
 * the hot path calls it.  The fields are the library's host-side plan (decided in vgpa_create, again when vgpa_set_problem_data /
 * vgpa_set_problem_params / vgpa_set_problem_obs_model change the form of the inputs) and its record of the buffers (DESIGN.md s.4.0 has both tables). */
enum { VGPA_STEPPER_LARGE_D = 0,  /* D > 64: the per-stage drivers                                   */
       VGPA_STEPPER_LANE = 1,     /* D <= 4: one lane per problem                                    */
       VGPA_STEPPER_WAVE = 2,     /* 2 <= D <= 4: 16 lanes per problem                               */
       VGPA_STEPPER_MFMA = 3,     /* 5 <= D <= 64, symmetric inputs: the matrix-core kernels         */
       VGPA_STEPPER_GENERIC = 4   /* one workgroup per problem, no symmetry assumed                  */ };
enum { VGPA_MOMENTS_ROW_MAJOR = 0, VGPA_MOMENTS_TIME_MAJOR = 1 };   /* m_t / S_t: the [B][Np] arrays; the lane pass's own layout alone */
enum { VGPA_LAYOUT_WHOLE = 0,     /* whole D x D matrices                                            */
       VGPA_LAYOUT_UPPER = 1,     /* whole matrices of which only the upper triangle is written      */
       VGPA_LAYOUT_PACKED = 2     /* packed lower triangles, D (D + 1) / 2 each                      */ };
enum { VGPA_BWD_NONE = 0,         /* nothing of the cached state is in lam_t / Psi_t's buffers       */
       VGPA_BWD_PSI = 1,          /* lam_t and Psi_t                                                 */
       VGPA_BWD_Q = 2             /* lam_t and Q''_t = Sigma^-1 A_t - 2 Psi_t                        */ };
/* (The struct only ever grows at its end: a field added later follows the last one, whichever of the two groups it belongs to.) */
typedef struct {
  /* the plan: what a fused sweep WILL run */
  int32_t fwd, bwd;               /* VGPA_STEPPER_* of the two sweep directions                      */
  int32_t sym_units;              /* matrix-core family: symmetric-unit / fragment-cover kernels     */
  int32_t launch_sym_units;       /* ... what the launcher is told (sym_units, or VGPA_ODE_KERNEL=sym) */
  int32_t lane_pass;              /* the objective is the fused lane pass                            */
  int32_t bwd_upper;              /* the backward kernel reads the upper triangle of dEsde_dS only   */
  int32_t store_q;                /* ... and stores Q''_t where Psi_t would be                       */
  int32_t packed;                 /* ... S_t and dEsde_dS travel as packed lower triangles           */
  int32_t grad_in_bwd;            /* ... the backward kernel can assemble the gradient               */
  int32_t grad_in_bwd_now;        /* ... and does, at this batch size                                */
  /* the record: what the buffers DO hold */
  int32_t cached;                 /* a fused sweep's state is cached                                 */
  int32_t moments;                /* VGPA_MOMENTS_*                                                  */
  int32_t S;                      /* VGPA_LAYOUT_WHOLE or _PACKED: S_t                               */
  int32_t dEs;                    /* VGPA_LAYOUT_*: dEsde_dS                                         */
  int32_t bwd_holds;              /* VGPA_BWD_*                                                      */
  int32_t terms;                  /* dEsde_dm / dEsde_dS / <f> / E_sde(t) belong to the cached moments */
  /* the plan again (added at the end) */
  int32_t helper_roles;           /* fragment-cover steppers: sets of helper waves, 0 / 1 / 2 (0 on every other stepper) */
} vgpa_path;
int vgpa_path_info(vgpa_ctx* ctx, vgpa_path* out);   /* VGPA_ERR_ARG for a null argument */

/* raw device memory helpers so that hosts without a HIP binding can own device buffers; whatever has not been returned
 * through vgpa_dev_free when the context is destroyed is freed with it */
int vgpa_dev_alloc(vgpa_ctx* ctx, uint64_t bytes, void** out);
int vgpa_dev_free(vgpa_ctx* ctx, void* ptr);
int vgpa_memcpy_h2d(vgpa_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int vgpa_memcpy_d2h(vgpa_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);

/* large-D (D > 64) stage-level entry points on DEVICE pointers --------------------------------------------------
 * One RK stage of the symmetric recursions = vgpa_ld_gemm (W[I_p,:] = A[I_p,:] X forward, (A^T)[I_p,:] Psi backward;
 * fp64 MFMA) + vgpa_ld_stage (fused element-wise update of the row block I_p = [row0, row0+Mp) and of the vector
 * recursion).  They stand behind the same reference code as vgpa_solve_fwd / vgpa_solve_bwd
 * (src/numerics/{euler,heun,runge_kutta2,runge_kutta4}.py); the host driver vgpa_amd/large_d.py places the RCCL
 * all-to-all / all-gather of the row-sharded recursion between the two calls.
 * `stream` is a hipStream_t (NULL = default stream).  C is written in column-chunk packed layout
 * C[(j / cw) * M * cw + i * cw + (j % cw)] (cw = N: plain row-major). */
typedef struct {
  int32_t D, row0, Mp, cw;      /* problem size, first row / number of rows of this rank, chunk width of W */
  int32_t fwd;                  /* 1: moments (S, m); 0: Lagrange multipliers (Psi, lam) */
  int32_t kstore;               /* 0 none, 1: K1 = R, 2: K23 = R, 3: K23 += R */
  int32_t final_mode;           /* 0: out = base +/- cx R; 1: base +/- cf R; 2: +/- cf (K1+R); 3: +/- cf (K1+2 K23+R)/6 */
  int32_t lda;                  /* leading dimension of A0 / A1 (vector recursion) */
  double cx, cf;
  const double* W;              /* [D/cw][Mp][cw] */
  const double* Wcol;           /* [D][Mp] (== W with one rank) */
  const double* E0;             /* [Mp][D] Sigma rows (fwd) or dEsde_dS[t] rows (bwd) */
  const double* E1;             /* NULL, or second operand of the mid-point 0.5*(E1+E0) */
  const double* J;              /* NULL, or [Mp][D] jump rows added by a final backward stage */
  const double* base;           /* [Mp][D] */
  double* K1; double* K23;      /* [Mp][D] */
  double* out;                  /* [Mp][D] */
  const double* A0;             /* full A of the stage (vector recursion reads rows row0..row0+Mp) */
  const double* A1;             /* NULL, or second operand of the mid-point */
  const double* x;              /* [D] stage vector */
  const double* e0; const double* e1;   /* [Mp] b (fwd) / dEsde_dm (bwd) entries; e1 NULL or mid-point operand */
  const double* jv;             /* NULL or [Mp] vector jump */
  const double* vbase;          /* [Mp] */
  double* k1v; double* k23v; double* vout;   /* [Mp] */
} vgpa_ld_stage_args;

int vgpa_ld_gemm(void* stream, int transa, int M, int N, int K, const double* A0, const double* A1_or_null, int lda,
                 const double* B, int ldb, double* C, int cw);
/* (vgpa_ld_stage runs the general kernel: E0 / E1 / J / base need not be symmetric.  The drivers inside the library, whose
 * inputs are checked to be symmetric, use a kernel that touches only the tiles on and above the diagonal.) */
int vgpa_ld_stage(void* stream, const vgpa_ld_stage_args* args);
/* One K-CHUNK launch of the stage product (the pipelined row-sharded stage splits a product into launches that wait for
 * different parts of the operand): C (+)= op(A)[:, ks] . B[ks, :] over the k-set ks = seg_tiles consecutive 16-wide k-tiles out
 * of every seg_stride k, K k's in all, starting where A0 / B point; accumulate != 0 continues the fp64 sums stored in C. */
int vgpa_ld_gemm_chunk(void* stream, int transa, int M, int N, int K, const double* A0, int lda, const double* B, int ldb,
                       double* C, int cw, int seg_tiles, int seg_stride, int accumulate);

/* What the D > 64 drivers launched, counted on the host where each launch is issued (tests, diagnostics): one table per process,
 * never reset -- read it before and after a call and take the difference.  vgpa_ld_launch_counts copies the first min(n,
 * VGPA_LD_COUNT_N) counters to `out` and returns VGPA_LD_COUNT_N (VGPA_ERR_ARG for a null `out` or n < 0).  The hand-written stage
 * product has one counter per tile height and kernel form: VGPA_LD_COUNT_GEMM + 6 * (0: 32 rows, 1: 64, 2: 128) + VGPA_LD_GEMM_*. */
enum {
  VGPA_LD_COUNT_STAGE_PROD_FWD = 0,      /* k_stage_prod, forward, the stage's own A */
  VGPA_LD_COUNT_STAGE_PROD_FWD_MID = 1,  /* ... averaging the mid-point pair while staging */
  VGPA_LD_COUNT_STAGE_PROD_BWD = 2,
  VGPA_LD_COUNT_STAGE_PROD_BWD_MID = 3,
  VGPA_LD_COUNT_STAGE_WIDE_FWD = 4,      /* k_stage_wide */
  VGPA_LD_COUNT_STAGE_WIDE_BWD = 5,
  VGPA_LD_COUNT_STAGE_SYM = 6,           /* k_stage_sym: element-wise stage on tile pairs */
  VGPA_LD_COUNT_STAGE_ROWS = 7,          /* k_stage: element-wise stage on a row block */
  VGPA_LD_COUNT_MID = 8,                 /* k_mid: the mid-point operand of a step, single-rank drivers */
  VGPA_LD_COUNT_TRANSPOSE = 9,           /* k_transpose: literal non-symmetric path */
  VGPA_LD_COUNT_LIBRARY_GEMM = 10,       /* stage product through the vendor library */
  VGPA_LD_COUNT_MID_COLS = 11,           /* k_mid_cols: the mid-point operand of a rank's slab, row-sharded driver */
  VGPA_LD_COUNT_GEMM = 12,
  VGPA_LD_COUNT_N = 30
};
enum {
  VGPA_LD_GEMM_CHECKED = 0,              /* k_gemm with bounds checks */
  VGPA_LD_GEMM_FULL = 1,                 /* k_gemm, whole tiles */
  VGPA_LD_GEMM_VEC = 2,                  /* k_gemm_v: 16-byte loads, two register sets */
  VGPA_LD_GEMM_VEC4 = 3,                 /* k_gemm_v, four register sets */
  VGPA_LD_GEMM_SEG = 4,                  /* k_gemm_v, K-chunk launch */
  VGPA_LD_GEMM_SEG4 = 5                  /* k_gemm_v, K-chunk launch, four register sets */
};
int vgpa_ld_launch_counts(int64_t* out, int n);

/* row-sharded recursion for large D on the GPUs of one node (BASELINE configs[4]) ------------------
 * One vgpa_shard per process / GPU.  Rank p of `world` owns rows [p D/world, (p+1) D/world) of S_t / Psi_t inside every
 * Runge-Kutta stage and the contiguous slice [t_lo, t_hi) of the TIME grid of the results (vgpa_shard_time_slice): the
 * whole step / stage loop of src/numerics/{euler,heun,runge_kutta2,runge_kutta4}.py:solve_fwd / solve_bwd runs inside
 * vgpa_shard_solve_* with two collectives per stage and no host synchronisation: an all-to-all of the packed product
 * blocks on the compute stream and the gather of the next stage state's row blocks + vector entries -- either ONE grouped
 * all-gather on the compute stream (serial schedule) or, when the table has send / recv, C sub-blocks on a second stream
 * with the next stage's product split into C K-chunk launches that each wait for one sub-block only (pipelined schedule,
 * the default: VGPA_SHARD_OPT_GATHER_CHUNKS).  The collectives come through a vgpa_comm table: vgpa_rccl_comm_create fills
 * it from librccl (dlopen'ed; rank 0 calls vgpa_rccl_unique_id and the host runtime -- MPI, torch.distributed, a file --
 * hands the 128 bytes to the other ranks), tests inject their own.  All pointers are DEVICE pointers; the operator-level
 * calls take inputs replicated on every rank ([Np][D][D] / [Np][D], same meaning as vgpa_solve_fwd / vgpa_solve_bwd),
 * outputs hold only the rank's own grid points: m_own [t_hi - t_lo][D], S_own [t_hi - t_lo][D][D].  D must be a multiple
 * of `world`; symmetric S0 / Sigma / dEsde_dS / jumps as for every D > 64 path.  Calls return when the work is ENQUEUED
 * (vgpa_shard_synchronize waits, at most VGPA_SHARD_OPT_TIMEOUT_MS).
 * Errors are collective: a failing table entry, a launch failure or a time-out aborts the communicator (`abort`) and returns
 * VGPA_ERR_COMM / VGPA_ERR_DEVICE; the shard is unusable afterwards (every later call returns VGPA_ERR_COMM).  The host
 * runtime's restart policy is a fresh process or a non-zero exit -- never a re-exec of a process that holds the GPU. */
typedef struct vgpa_comm {
  void* user;
  /* recv[q * count .. (q+1) * count) = send of rank q; send may be recv + rank * count (in place) */
  int (*all_gather)(void* user, const double* send, double* recv, uint64_t count, void* stream);
  /* chunk q of send goes to rank q, chunk q of recv comes from rank q; count doubles per chunk */
  int (*all_to_all)(void* user, const double* send, double* recv, uint64_t count, void* stream);
  int (*group_begin)(void* user);      /* optional (may be NULL): fuse the calls up to group_end into one launch */
  int (*group_end)(void* user);
  /* optional point-to-point pair (both or neither; only between group_begin and group_end, which are then required): the
   * pipelined gather posts, per sub-block, one send to and one receive from every peer -- one xGMI link each */
  int (*send)(void* user, const double* buf, uint64_t count, int peer, void* stream);
  int (*recv)(void* user, double* buf, uint64_t count, int peer, void* stream);
  /* optional: tear the communicator down after a failure so that no rank stays inside a collective (ncclCommAbort) */
  int (*abort)(void* user);
} vgpa_comm;
typedef struct vgpa_shard vgpa_shard;
int vgpa_shard_create(vgpa_shard** out, int method, double dt, int dim_d, int n_pts, int rank, int world, int device,
                      const vgpa_comm* comm_or_null_if_world_1, void* stream_or_null);
void vgpa_shard_destroy(vgpa_shard* s);
int vgpa_shard_time_slice(const vgpa_shard* s, int* t_lo, int* t_hi);
/* the same rule without a shard: grid points [t_lo, t_hi) of `rank` out of `world` on a grid of n_pts (host arithmetic only) */
int vgpa_time_slice(int n_pts, int rank, int world, int* t_lo, int* t_hi);
void* vgpa_shard_stream(vgpa_shard* s);
int vgpa_shard_synchronize(vgpa_shard* s);
enum vgpa_shard_option {
  VGPA_SHARD_OPT_GATHER_CHUNKS = 1,  /* sub-blocks of the pipelined gather: 0 = serial schedule, 1..8 (reduced to what the
                                        row-block size allows: whole 16-row k-tiles per sub-block; 0 without send / recv).
                                        Default 4, or the environment's VGPA_SHARD_CHUNKS.  Same value on every rank. */
  VGPA_SHARD_OPT_TIMEOUT_MS = 2      /* bound of every host wait on the shard's streams (default 600000; <= 0: none) */
};
int vgpa_shard_set_option(vgpa_shard* s, int option, int64_t value);
int vgpa_shard_get_option(const vgpa_shard* s, int option, int64_t* value);
int vgpa_shard_solve_fwd(vgpa_shard* s, const double* lin_a, const double* off_b, const double* m0, const double* s0,
                         const double* sigma, double* m_own, double* s_own);
int vgpa_shard_solve_bwd(vgpa_shard* s, const double* lin_a, const double* desde_dm, const double* desde_ds,
                         const double* deobs_dm, const double* deobs_ds, double* lam_own, double* psi_own);
/* The fused sweep -- free energy AND gradient of VarGP (src/var_bayes/variational.py:141-288) -- of ONE Lorenz-96 problem
 * (diagonal system noise, diagonal R, H = I: the restrictions of every D > 64 path) on the row-sharded recursion:
 *   forward recursion, row-sharded, (m_t, S_t) time-sharded  ->  observation terms and E_sde terms of the rank's own grid
 *   points (time-parallel: lorenz_96.py:316-438 per grid point)  ->  a time -> row EXCHANGE of dEsde_dS (all-to-all: every
 *   rank receives rows I_p of every grid point, 1/world of an all-gather's bytes) + small all-gathers of dEsde_dm / E_sde(t)
 *   / the observation jumps  ->  backward recursion, row-sharded  ->  gradient of the own grid points.
 * vgpa_shard_sweep:         x_dev = [A_t (Np,D,D) | b_t (Np,D)] replicated on every rank (device).
 * vgpa_shard_sweep_sharded: x MEMORY-SHARDED like the gradient -- a_own [t_hi - t_lo][D][D], b_own [t_hi - t_lo][D] (the
 *                           layout of variational.py:153-162 restricted to the rank's grid points); rows I_p (forward) and
 *                           columns I_p (backward) of every A_t reach the recursions through two more exchanges.  No rank
 *                           ever holds a complete (Np, D, D) array: per rank seven arrays of Np/world matrices (x, the two
 *                           block copies of A, S, dEsde_dS / Psi, its row blocks, the gradient).
 * F comes back on every rank (host); the gradient stays TIME-sharded: grad_a_own [t_hi - t_lo][D][D], grad_b_own
 * [t_hi - t_lo][D] (device).  Synchronises the shard's streams before returning.  The return code is COLLECTIVE -- the same
 * on every rank: VGPA_ERR_NOT_PD when a marginal covariance S_t of ANY rank's grid points is not positive definite (the
 * reference raises LinAlgError, variational.py:380), VGPA_ERR_DEVICE when any rank could not allocate its buffers,
 * VGPA_ERR_ARG (before any collective) for observation indices that are out of range or not strictly increasing. */
typedef struct {
  double theta;                   /* Lorenz-96 forcing */
  const double* inv_sigma_diag;   /* [D] device: diagonal of Sigma^-1 */
  const double* m0;               /* [D] device */
  const double* s0;               /* [D][D] device */
  const double* sigma;            /* [D][D] device */
  int32_t n_obs;
  const int64_t* obs_t;           /* [n_obs] HOST: grid indices of the observations, strictly increasing */
  const double* obs_y;            /* [n_obs][D] device */
  const double* obs_rinv_diag;    /* [D] device: diagonal of R^-1 */
  double obs_const;               /* n_obs (D log(2 pi) + log det R)  (gaussian_like.py:87-92) */
  double e0;                      /* KL(q0||p0), constant in x */
} vgpa_shard_problem;
int vgpa_shard_sweep(vgpa_shard* s, const vgpa_shard_problem* problem, const double* x_dev, double* f_host,
                     double* grad_a_own, double* grad_b_own);
int vgpa_shard_sweep_sharded(vgpa_shard* s, const vgpa_shard_problem* problem, const double* a_own, const double* b_own,
                             double* f_host, double* grad_a_own, double* grad_b_own);
/* the two per-stage collectives alone (same buffers, sizes, streams and schedule as inside a stage), averaged over `reps`
 * rounds: what bench.py reports as per-stage collective milliseconds.  Collective call. */
int vgpa_shard_time_collectives(vgpa_shard* s, int reps, double* all_to_all_ms, double* gather_ms);
/* One stage of the forward RK4 recursion as the driver issues it (K-chunk products waiting for the previous gather's sub-blocks,
 * all-to-all, stage kernel, gather), `reps` times back to back on the shard's workspace; with_collectives == 0 leaves the
 * collectives out, so the difference of the two is the communication a stage does not hide.  Timing only (the workspace is
 * overwritten; call between sweeps).  Collective call when with_collectives != 0. */
int vgpa_shard_time_stage(vgpa_shard* s, int reps, int with_collectives, double* ms_per_stage);
/* Milliseconds of the six phases of this rank's LAST fused sweep (HIP events on the shard's stream): [0] exchanges of a
 * memory-sharded x, [1] forward recursion, [2] observation + E_sde terms of the own grid points, [3] small gathers + time -> row
 * exchange of dEsde_dS, [4] backward recursion, [5] gradient of the own grid points + F.  VGPA_ERR_STATE before the first sweep. */
int vgpa_shard_phase_ms(vgpa_shard* s, double* ms6);
/* RCCL behind the vgpa_comm table: collectives over xGMI; the library is dlopen'ed on first use */
#define VGPA_RCCL_UNIQUE_ID_BYTES 128
int vgpa_rccl_unique_id(void* out_128_bytes);
int vgpa_rccl_comm_create(vgpa_comm* out, const void* id_128_bytes, int rank, int world, int device);
void vgpa_rccl_comm_destroy(vgpa_comm* comm);
/* ranks of the communicator as librccl counts them (ncclCommCount); VGPA_ERR_ARG for a table RCCL did not fill */
int vgpa_rccl_comm_count(const vgpa_comm* comm, int* count);
/* communicators behind the table: 2 -- the collectives of the compute stream and the point-to-point groups of the communication stream
 * (the pipelined gather) each have their own (ncclCommSplit of the first) -- or 1 when the library cannot split */
int vgpa_rccl_comm_streams(const vgpa_comm* comm, int* count);

/* Device memory without a context -- what the callers of the row-sharded driver keep their operands and results in (the host
 * mirror vgpa_amd/large_d.py needs no tensor library for it).  kind: 1 = host -> device, 2 = device -> host, 3 = device -> device;
 * the copy is complete on return (it also waits for the device: results of an enqueued sweep are safe to read). */
int vgpa_device_alloc(int device, uint64_t bytes, void** out);
int vgpa_device_free(int device, void* ptr);
int vgpa_device_memcpy(int device, void* dst, const void* src, uint64_t bytes, int kind);

/* timing of the stepping kernel on the context's stream (HIP events), for bench.py's roofline */
int vgpa_profile_begin(vgpa_ctx* ctx);
int vgpa_profile_end(vgpa_ctx* ctx, double* fwd_ms, double* energy_ms, double* bwd_ms,
                     double* grad_ms, int64_t* n_sweeps);

#ifdef __cplusplus
}
#endif
#endif /* VGPA_HIP_H */
