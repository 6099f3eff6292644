// The host side of the particle entry points (vgpa_api.hip: ParticleRequest, ParticleRun, particle_run) without a device: a stand-alone
// program that links the host code of vgpa_api.hip against a HIP runtime and launchers of its own.  Device memory is host memory (every
// allocation a calloc of its own, so AddressSanitizer sees a copy or memset that leaves it), the launchers of sample.hip record their name
// and arguments and do nothing, and every operation on the stream -- memset, copy in either direction, launch, synchronisation -- is
// printed in order, device pointers as "d<allocation>+<offset>".  One request per entry point and variant (histories, rows, given slots,
// given start, both modes of the forecast; the marginals last) on a batch of two Lorenz-63 problems with different observation counts.  Two commits run the
// same host logic exactly when the two outputs are equal.
//
//   hipcc -x hip --offload-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ivgpa_amd/csrc \
//         -c vgpa_amd/csrc/vgpa_api.hip -o api.o      (likewise this file and vgpa_amd/csrc/host_linalg.cpp)
//   clang++ -fsanitize=address,undefined api.o host_linalg.o particle_stream.o -Wl,--unresolved-symbols=ignore-all -o particle_stream
//   ./particle_stream > stream.txt      # on the CPU; the launchers of the other files stay unresolved and are never called
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "vgpa_hip.h"
#include "vgpa_internal.h"

namespace {
struct Block { char* base; size_t size; };
std::vector<Block> blocks;
bool recording = false;

std::string where(const void* p) {
  if (!p) return "null";
  const char* q = static_cast<const char*>(p);
  for (size_t i = 0; i < blocks.size(); i++)
    if (blocks[i].base && q >= blocks[i].base && q < blocks[i].base + blocks[i].size) return "d" + std::to_string(i) + "+" + std::to_string(q - blocks[i].base);
  return "host";
}
void rec(const char* fmt, ...) {
  if (!recording) return;
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
}
#define W(p) where(p).c_str()
}      // namespace

// ---------------------------------------------------------------- the HIP runtime of this program
extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  *p = std::calloc(n ? n : 1, 1);
  blocks.push_back({static_cast<char*>(*p), n});
  rec("malloc %zu -> d%zu", n, blocks.size() - 1);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  for (auto& b : blocks)
    if (b.base == p) { rec("free %s", W(p)); b.base = nullptr; }
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = std::calloc(n ? n : 1, 1); return hipSuccess; }
hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { rec("memcpy %s <- %s %zu", W(d), W(s), n); std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  rec("memcpy_async %s <- %s %zu", W(d), W(s), n);
  std::memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t) {
  rec("memcpy2d_async %s/%zu <- %s/%zu %zu x %zu", W(d), dp, W(s), sp, w, h);
  for (size_t i = 0; i < h; i++) std::memcpy(static_cast<char*>(d) + i * dp, static_cast<const char*>(s) + i * sp, w);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { rec("memset_async %s %d %zu", W(d), v, n); std::memset(d, v, n); return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) { *v = 65536; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { rec("device_synchronize"); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "(no device)"; }
hipError_t hipMemGetInfo(size_t* f, size_t* t) { *f = *t = (size_t)64 << 30; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { rec("stream_synchronize"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
}

// ---------------------------------------------------------------- the launchers of sample.hip, as recorders
namespace vgpa {
static void pf(const char* name, const PfArgs& a) {
  rec("launch %s D %d B %d n %d M %d k %d last %d ess %g Np %d n_obs %d x0 %s mu0 %s Lt %s x %s ws %s lw %s x_in %s x_out %s cum %s anc %s h_ess %s h_flag %s "
      "h_anc %s h_clouds %s h_lw %s st_in %s st_out %s ref %s obs_t %s n_obs_v %s", name, a.D, a.batch, a.n_paths, a.M, a.k, a.last, a.ess_fraction, a.Np, a.n_obs,
      W(a.x0), W(a.mu0), W(a.Lt), W(a.x), W(a.ws), W(a.lw), W(a.x_in), W(a.x_out), W(a.cum), W(a.anc), W(a.h_ess), W(a.h_flag), W(a.h_anc), W(a.h_clouds),
      W(a.h_lw), W(a.st_in), W(a.st_out), W(a.ref), W(a.obs_t), W(a.n_obs_v));
}
static void walk(const SampleArgs& a) {
  rec("       kind %d model %d D %d Np %d B %d n %d stride %d n_keep %d first %d k %d..%d rows %d M %d slot_rows %d pf_n %d x0 %s out %s logw %s start %s "
      "pf_x %s pf_lw %s pf_stats %s pf_wtab %s pf_part %s pf_slots %s pf_clouds %s pf_hanc %s A %s b %s R %s theta_v %s", a.kind, a.model, a.D, a.Np, a.batch,
      a.n_paths, a.stride, a.n_keep, a.seg_first, a.k_begin, a.k_end, a.pf_rows, a.pf_M, a.pf_slot_rows, a.pf_n, W(a.x0), W(a.out), W(a.logw), W(a.start), W(a.pf_x),
      W(a.pf_lw), W(a.pf_stats), W(a.pf_wtab), W(a.pf_part), W(a.pf_slots), W(a.pf_clouds), W(a.pf_hanc), W(a.A), W(a.b), W(a.R), W(a.theta_v));
}
hipError_t launch_sample_walk(Walk w, const SampleArgs& a, hipStream_t, const WalkOwn& own) {
  rec("launch sample_walk walk %d pf_ref %s ev_level %s ev_side %s", (int)w, W(own.pf_ref), W(own.ev_level), W(own.ev_side));
  walk(a);
  if (const MarginalArgs* mg = own.mg) rec("       levels %s L %d qtab %s mass %s", W(mg->levels), mg->L, W(mg->qtab), W(mg->mass));      // (Walk::ReplayMarginals alone)
  return hipSuccess;
}
int sample_segment_blocks(int, int n_paths) { return (n_paths + 63) / 64; }
int sample_max_paths(int) { return 1 << 20; }
bool sample_lineages_fit(int, int, int) { return true; }
bool pf_flat_grid_fits(size_t) { return true; }
hipError_t launch_pf_start(const PfArgs& a, hipStream_t) { pf("pf_start", a); return hipSuccess; }
hipError_t launch_pf_resample(const PfArgs& a, hipStream_t) { pf("pf_resample", a); return hipSuccess; }
hipError_t launch_pf_pin(const PfArgs& a, hipStream_t) { pf("pf_pin", a); return hipSuccess; }
hipError_t launch_pf_cresample(const PfArgs& a, const SampleArgs& s, hipStream_t) { pf("pf_cresample", a); walk(s); return hipSuccess; }
hipError_t launch_pf_ref_fill(const PfArgs& a, int rows, const int32_t* table, double* out, hipStream_t) {
  pf("pf_ref_fill", a);
  rec("       rows %d table %s out %s", rows, W(table), W(out));
  return hipSuccess;
}
hipError_t launch_pf_gather(const PfArgs& a, hipStream_t) { pf("pf_gather", a); return hipSuccess; }
hipError_t launch_pf_descend(const PfArgs& a, int rows, double* wtab, double* less, hipStream_t) {
  pf("pf_descend", a);
  rec("       rows %d wtab %s less %s", rows, W(wtab), W(less));
  return hipSuccess;
}
hipError_t launch_pf_quantise(const PfArgs& a, int rows, const double* wtab, uint64_t* qtab, uint64_t* qfinal, hipStream_t) {
  pf("pf_quantise", a);
  rec("       rows %d wtab %s qtab %s qfinal %s", rows, W(wtab), W(qtab), W(qfinal));
  return hipSuccess;
}
hipError_t launch_pf_descend_q(const PfArgs& a, int rows, uint64_t* qtab, hipStream_t) {
  pf("pf_descend_q", a);
  rec("       rows %d qtab %s", rows, W(qtab));
  return hipSuccess;
}
hipError_t launch_pf_pick(const PfArgs& a, int k, int n_draw, int rows, int32_t* table, hipStream_t) {
  pf("pf_pick", a);
  rec("       k %d n_draw %d rows %d table %s", k, n_draw, rows, W(table));
  return hipSuccess;
}
hipError_t launch_pf_trace(const PfArgs& a, int n_draw, int rows, int32_t* table, hipStream_t) {
  pf("pf_trace", a);
  rec("       n_draw %d rows %d table %s", n_draw, rows, W(table));
  return hipSuccess;
}
hipError_t launch_pf_backward(const PfArgs& a, const SampleArgs& s, int n_draw, int rows, int32_t* table, hipStream_t) {
  pf("pf_backward", a);
  walk(s);
  rec("       n_draw %d rows %d table %s", n_draw, rows, W(table));
  return hipSuccess;
}
hipError_t launch_pf_normalise(int B, int n, const double* lw, double* w, hipStream_t) { rec("launch pf_normalise %d %d %s %s", B, n, W(lw), W(w)); return hipSuccess; }
hipError_t launch_pf_cov_unpack(int D, size_t kept, const double* in, double* mean, double* second, hipStream_t) {
  rec("launch pf_cov_unpack %d %zu %s %s %s", D, kept, W(in), W(mean), W(second));
  return hipSuccess;
}
hipError_t launch_pf_events_cdf(int D, int B, int n, int Np, int stride, const double* lw, const double* rows, double* cdf, hipStream_t) {
  rec("launch pf_events_cdf %d %d %d %d %d %s %s %s", D, B, n, Np, stride, W(lw), W(rows), W(cdf));
  return hipSuccess;
}
hipError_t launch_pf_stats_mean(int D, int B, int n, const double* lw, const double* rows, double* mean, hipStream_t) {
  rec("launch pf_stats_mean %d %d %d %s %s %s", D, B, n, W(lw), W(rows), W(mean));
  return hipSuccess;
}
hipError_t launch_pf_moments_sum(int B, int blocks, size_t len, const double* part, double* out, hipStream_t) {
  rec("launch pf_moments_sum %d %d %zu %s %s", B, blocks, len, W(part), W(out));
  return hipSuccess;
}
hipError_t launch_pf_events_start(int D, int B, int n, int Np, const double* x, const double* lev, const int32_t* side, double* rows, hipStream_t) {
  rec("launch pf_events_start %d %d %d %d %s %s %s %s", D, B, n, Np, W(x), W(lev), W(side), W(rows));
  return hipSuccess;
}
}      // namespace vgpa

// ---------------------------------------------------------------- the requests
int main() {
  const int D = 3, Np = 11, B = 2, M = 2, n = 65, K = 5, len_x = Np * D * (D + 1);
  const double theta[3] = {10.0, 28.0, 8.0 / 3.0}, sigma[9] = {4, 0, 0, 0, 4, 0, 0, 0, 4}, m0[3] = {1, 2, 3}, s0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double noise[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2}, obs_y[6] = {1, 2, 3, 4, 5, 6};
  const int64_t obs_t[2] = {3, 7};
  vgpa_config cfg{};
  cfg.abi_version = VGPA_ABI_VERSION; cfg.model = VGPA_MODEL_L63; cfg.method = VGPA_ODE_EULER; cfg.dim_d = D; cfg.n_pts = Np; cfg.batch = B;
  cfg.dt = 0.01; cfg.n_theta = 3; cfg.n_obs = M; cfg.theta = theta; cfg.sigma = sigma; cfg.m0 = m0; cfg.s0 = s0; cfg.obs_t = obs_t; cfg.obs_y = obs_y;
  cfg.obs_noise = noise;
  vgpa_ctx* c = nullptr;
  int rc = vgpa_create(&c, &cfg);
  if (rc) { std::printf("vgpa_create: %d %s\n", rc, vgpa_last_error(nullptr)); return 1; }
  const int32_t counts[2] = {2, 1};
  if ((rc = vgpa_set_problem_obs_model(c, counts, nullptr, nullptr))) { std::printf("obs model: %d %s\n", rc, vgpa_last_error(c)); return 1; }
  std::vector<double> x((size_t)B * len_x, 0.5), x0((size_t)B * D, 1.0), mu((size_t)B * D, 0.0), tau((size_t)B * D * D, 0.0), ref((size_t)B * Np * D, 0.25);
  for (int p = 0; p < B; p++) for (int j = 0; j < D; j++) tau[(size_t)p * D * D + j * D + j] = 2.0;
  std::vector<double> lw((size_t)B * n), st((size_t)B * n * D), ess((size_t)B * M), clouds((size_t)B * M * n * D), rows((size_t)B * n * 3 * D), mean((size_t)B * 3 * D);
  std::vector<int32_t> flag((size_t)B * M), anc((size_t)B * M * n), table((size_t)B * (M + 1) * K), given = {64, 0, 13, 13, 7, 1, 2, 3, 4, 5};
  std::vector<double> cdf((size_t)B * Np * D), mom((size_t)B * Np * 2 * D), less((size_t)B * (M + 1)), cmean((size_t)B * Np * D), csec((size_t)B * Np * D * D);
  std::vector<double> paths((size_t)B * K * Np * D), traj((size_t)B * Np * D), members((size_t)B * K * 10 * D), end((size_t)B * n * D), lev((size_t)B * D, 0.1);
  std::vector<int32_t> side((size_t)B * D, 1), fslots((size_t)B * K);
  side[1] = -1;
  int failed = 0;
  auto run = [&](const char* name, int got) {
    std::printf("== %s -> %d%s%s\n", name, got, got ? " " : "", got ? vgpa_last_error(c) : "");
    failed += got != 0;
  };
  recording = true;
  for (int start = 0; start < 2; start++) {      // a drawn start with the prior's term; a given start
    const double* s = start ? x0.data() : nullptr;
    const double* pm = start ? nullptr : mu.data();
    const double* pt = start ? nullptr : tau.data();
    std::printf("==== %s start\n", start ? "given" : "drawn");
    run("filter", vgpa_particle_filter(c, x.data(), s, n, 7, 0.5, pm, pt, lw.data(), st.data(), ess.data(), flag.data(), nullptr, nullptr));
    run("filter, histories", vgpa_particle_filter(c, x.data(), s, n, 7, 0.5, pm, pt, lw.data(), st.data(), ess.data(), flag.data(), anc.data(), clouds.data()));
    run("statistics", vgpa_particle_statistics(c, x.data(), s, n, 7, 0.5, pm, pt, lw.data(), st.data(), rows.data(), mean.data(), ess.data(), flag.data()));
    run("statistics, mean alone", vgpa_particle_statistics(c, x.data(), s, n, 7, 0.5, pm, pt, lw.data(), st.data(), nullptr, mean.data(), nullptr, nullptr));
    run("events", vgpa_particle_events(c, x.data(), s, n, 3, 7, 0.5, pm, pt, lev.data(), side.data(), lw.data(), st.data(), rows.data(), mean.data(), cdf.data(), ess.data(), flag.data()));
    run("events, cdf alone", vgpa_particle_events(c, x.data(), s, n, 1, 7, 0.5, pm, pt, lev.data(), side.data(), lw.data(), st.data(), nullptr, nullptr, cdf.data(), ess.data(), flag.data()));
    run("moments", vgpa_particle_moments(c, x.data(), s, n, 3, 7, 0.5, pm, pt, lw.data(), st.data(), mom.data(), less.data(), ess.data(), flag.data()));
    run("covariance", vgpa_particle_covariance(c, x.data(), s, n, 3, 7, 0.5, pm, pt, lw.data(), st.data(), cmean.data(), csec.data(), less.data(), ess.data(), flag.data()));
    run("paths", vgpa_particle_paths(c, x.data(), s, n, K, nullptr, 3, 7, 0.5, pm, pt, lw.data(), st.data(), paths.data(), table.data(), ess.data(), flag.data()));
    run("paths, given slots", vgpa_particle_paths(c, x.data(), s, n, K, given.data(), 1, 7, 0.5, pm, pt, lw.data(), st.data(), paths.data(), nullptr, ess.data(), flag.data()));
    run("backward paths", vgpa_particle_backward_paths(c, x.data(), s, n, K, nullptr, 3, 7, 0.5, pm, pt, lw.data(), st.data(), paths.data(), table.data(), ess.data(), flag.data()));
    run("backward paths, given slots", vgpa_particle_backward_paths(c, x.data(), s, n, K, given.data(), 1, 7, 0.5, pm, pt, lw.data(), st.data(), paths.data(), table.data(), ess.data(), flag.data()));
    run("conditional", vgpa_particle_conditional(c, x.data(), s, ref.data(), n, 7, 0.5, pm, pt, lw.data(), st.data(), traj.data(), table.data(), ess.data(), flag.data(), nullptr, nullptr));
    run("conditional, histories", vgpa_particle_conditional(c, x.data(), s, ref.data(), n, 7, 0.5, pm, pt, lw.data(), st.data(), traj.data(), table.data(), ess.data(), flag.data(), anc.data(), clouds.data()));
    run("forecast behind the filter", vgpa_particle_forecast(c, x.data(), s, n, 7, 0.5, pm, pt, nullptr, nullptr, 0, 9, 3, K, nullptr, lw.data(), st.data(), ess.data(), flag.data(), mom.data(), members.data(), fslots.data(), end.data()));
    run("forecast behind the filter, given slots", vgpa_particle_forecast(c, x.data(), s, n, 7, 0.5, pm, pt, nullptr, nullptr, 0, 9, 1, K, given.data(), lw.data(), st.data(), ess.data(), flag.data(), mom.data(), members.data(), fslots.data(), end.data()));
    run("forecast, no members", vgpa_particle_forecast(c, x.data(), s, n, 7, 0.5, pm, pt, nullptr, nullptr, 0, 9, 3, 0, nullptr, lw.data(), st.data(), nullptr, nullptr, mom.data(), nullptr, nullptr, nullptr));
  }
  run("forecast from a cloud", vgpa_particle_forecast(c, nullptr, nullptr, n, 7, 0.5, nullptr, nullptr, end.data(), lw.data(), 19, 9, 3, K, nullptr, lw.data(), st.data(), nullptr, nullptr, mom.data(), members.data(), fslots.data(), end.data()));
  run("forecast from a cloud, equal weights, given slots", vgpa_particle_forecast(c, nullptr, nullptr, n, 7, 0.5, nullptr, nullptr, end.data(), nullptr, 19, 9, 1, K, given.data(), lw.data(), st.data(), nullptr, nullptr, mom.data(), members.data(), fslots.data(), nullptr));
  // what the entry points refuse, by text
  run("refused: stride 0", vgpa_particle_moments(c, x.data(), nullptr, n, 0, 7, 0.5, nullptr, nullptr, lw.data(), st.data(), mom.data(), nullptr, nullptr, nullptr) == VGPA_OK);
  std::printf("   %s\n", vgpa_last_error(c));
  run("refused: statistics without stats and mean", vgpa_particle_statistics(c, x.data(), nullptr, n, 7, 0.5, nullptr, nullptr, lw.data(), st.data(), nullptr, nullptr, nullptr, nullptr) == VGPA_OK);
  std::printf("   %s\n", vgpa_last_error(c));
  run("refused: a slot outside", vgpa_particle_paths(c, x.data(), nullptr, 4, K, given.data(), 1, 7, 0.5, nullptr, nullptr, lw.data(), st.data(), paths.data(), nullptr, nullptr, nullptr) == VGPA_OK);
  std::printf("   %s\n", vgpa_last_error(c));
  // the marginals, behind every earlier request: their allocations and operations stay what they were
  {
    const int L = 5;
    std::vector<double> ladder((size_t)B * D * L);
    for (size_t e = 0; e < ladder.size(); e++) ladder[e] = 0.5 * (double)(e % L) - 1.0;
    std::vector<uint64_t> mass((size_t)B * Np * D * (L + 1)), qfinal((size_t)B * n);
    run("marginals", vgpa_particle_marginals(c, x.data(), nullptr, n, 3, 7, 0.5, mu.data(), tau.data(), ladder.data(), L, lw.data(), st.data(), mass.data(), qfinal.data(), less.data(), ess.data(), flag.data()));
    run("marginals, given start, mass alone", vgpa_particle_marginals(c, x.data(), x0.data(), n, 1, 7, 0.5, nullptr, nullptr, ladder.data(), L, lw.data(), st.data(), mass.data(), nullptr, nullptr, nullptr, nullptr));
    ladder[(size_t)(1 * D + 2) * L + 3] = ladder[(size_t)(1 * D + 2) * L + 2];
    run("refused: a ladder that does not increase", vgpa_particle_marginals(c, x.data(), nullptr, n, 1, 7, 0.5, nullptr, nullptr, ladder.data(), L, lw.data(), st.data(), mass.data(), nullptr, nullptr, nullptr, nullptr) == VGPA_OK);
    std::printf("   %s\n", vgpa_last_error(c));
  }
  recording = false;
  vgpa_destroy(c);
  return failed ? 1 : 0;
}
