// Which kernel every launcher of vgpa_amd/csrc picks, with what grid, block and dynamic LDS, over the whole run-time domain of its request --
// without a device.  A translation unit compiled --offload-host-only still registers its kernels at start-up (__hipRegisterFunction: the
// host stub's address with the mangled device name) and launches through __hipPushCallConfiguration / __hipPopCallConfiguration /
// hipLaunchKernel(stub, ...): this program is those symbols, hipFuncSetAttribute, hipGetLastError and the few stream calls of
// large_d_energy.hip, as recorders.  Pointers in the requests are dummies; nothing dereferences them on the host.
//
// Output.  Per launcher family one line: the number of requests, a hash over every request's text, launches and return code, and the number
// and a hash of its opt-in (attr) lines -- the dynamic-LDS opt-ins are the one thing two commits may differ in while they dispatch alike.
// --outcomes adds every distinct outcome under the line -- "launch <kernel> grid x,y,z block n lds bytes | rc <code>", "(attr)" behind a
// launch that opted in, "attr <kernel> <bytes>" where the opt-in stands alone -- with the number of requests that had it: where to look when
// a hash moved.  --full prints every request with its events, one per line, instead.  Then one request per launch_lds family with
// hipFuncSetAttribute failing (the launcher returns that error and launches nothing), and last every kernel that was registered and never
// launched: those named in kNotCovered with the reason, and the rest, which must be none.
// tests/test_dispatch_census_cpu.py holds the output to tests/golden/dispatch_census.txt.
//
//   F="-x hip --offload-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ivgpa_amd/csrc"
//   for s in ode_generic ode_small ode_wave ode_mfma ode_mfma_m0 ode_mfma_m1 ode_mfma_m2 ode_mfma_m3 energy assemble lag_cov sample \
//            large_d large_d_stage large_d_energy; do hipcc $F -c vgpa_amd/csrc/$s.hip -o $s.o; done
//   hipcc $F -c tools/host_check/dispatch_census.cpp -o dispatch_census.o
//   clang++ -fsanitize=address,undefined *.o -Wl,--unresolved-symbols=ignore-all -o dispatch_census
//   ./dispatch_census > census.txt      # on the CPU; (the pytest builds the same without the sanitizers)
#include <cxxabi.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "vgpa_hip.h"
#include "vgpa_internal.h"
#include "large_d_stage.h"

namespace {
struct Kernel { std::string name; long launches = 0; };
std::map<const void*, Kernel>& kernels() { static std::map<const void*, Kernel> k; return k; }      // (filled before main: no static order)

// "void vgpa::(anonymous namespace)::k_lag_lane<1, 0>(vgpa::LagArgs)" -> "k_lag_lane<1,0>"
std::string short_name(const char* mangled) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string s = status == 0 && d ? d : mangled;
  std::free(d);
  int depth = 0;
  size_t cut = s.size();
  for (size_t i = 0; i < s.size(); i++) {      // the argument list: the first '(' outside template brackets that opens no cast
    if (s[i] == '<') depth++;
    if (s[i] == '>') depth--;
    if (s[i] == '(' && depth == 0 && s.compare(i, 11, "(anonymous ") != 0) { cut = i; break; }
  }
  s.resize(cut);
  for (const char* drop : {"void ", "vgpa::", "(anonymous namespace)::", " "})
    for (size_t p; (p = s.find(drop)) != std::string::npos;) s.erase(p, std::strlen(drop));
  return s;
}

std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

bool full = false, outcomes = false, fail_attr = false;
struct Event {      // "attr <kernel> <bytes>" or "launch <kernel> grid x,y,z block n lds <bytes>"
  bool attr; std::string kernel, shape; size_t bytes;
  std::string text() const { return attr ? fmt("attr %s %zu", kernel.c_str(), bytes) : fmt("launch %s %s lds %zu", kernel.c_str(), shape.c_str(), bytes); }
};
std::vector<Event> events;      // of the request that is running
constexpr uint64_t kFnv = 1469598103934665603ull;
struct Family { std::string name; long requests = 0, attrs = 0; uint64_t hash = kFnv, attr_hash = kFnv; std::map<std::string, long> outcomes; };
Family* fam = nullptr;
void fnv(uint64_t& h, const std::string& s) { for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; } }      // FNV-1a
void hash_in(const std::string& s) { fnv(fam->hash, s); }

// one request: its text, the launcher's call, the return code.  The outcome as the summary prints it: the events in order of first
// appearance, each once with its count; an opt-in for the very kernel and size launched next is "(attr)" behind that launch.
template <class Call>
void request(const std::string& text, Call call) {
  events.clear();
  const std::string rc = fmt("rc %d", (int)call());
  fam->requests++;
  hash_in(text);
  if (full) std::printf("%s: %s\n", fam->name.c_str(), text.c_str());
  std::vector<std::pair<std::string, long>> seen;
  for (size_t i = 0; i < events.size(); i++) {
    const Event& e = events[i];
    if (full) std::printf("  %s\n", e.text().c_str());
    if (!e.attr) hash_in(e.text());
    else { fam->attrs++; fnv(fam->attr_hash, text + e.text()); }
    const bool own = e.attr && i + 1 < events.size() && !events[i + 1].attr && events[i + 1].kernel == e.kernel && events[i + 1].bytes == e.bytes;
    if (own) continue;      // (told with the launch)
    const std::string t = e.text() + (i > 0 && events[i - 1].attr && events[i - 1].kernel == e.kernel && events[i - 1].bytes == e.bytes && !e.attr ? " (attr)" : "");
    bool found = false;
    for (auto& s : seen)
      if (s.first == t) { s.second++; found = true; }
    if (!found) seen.push_back({t, 1});
  }
  hash_in(rc);
  if (full) std::printf("  %s\n", rc.c_str());
  std::string outcome;
  for (auto& s : seen) outcome += (s.second > 1 ? fmt("%ldx ", s.second) : std::string()) + s.first + " | ";
  fam->outcomes[outcome + rc]++;
}
struct Scope {
  Family f;
  explicit Scope(const char* name) { f.name = name; fam = &f; }
  ~Scope() {
    fam = nullptr;
    if (full) return;
    std::printf("== %s: %ld requests, hash %016llx; %ld opt-ins, hash %016llx\n", f.name.c_str(), f.requests, (unsigned long long)f.hash, f.attrs,
                (unsigned long long)f.attr_hash);
    if (outcomes)
      for (auto& o : f.outcomes) std::printf("  %6ld x %s\n", o.second, o.first.c_str());
  }
};

double* const P = reinterpret_cast<double*>(0x100000);       // a 16-byte aligned address nobody reads
template <class T> T* ptr(bool set, size_t off = 0) { return set ? reinterpret_cast<T*>(0x100000 + off) : nullptr; }
hipStream_t const ST = nullptr;
}  // namespace

// ---------------------------------------------------------------- the HIP runtime of this program
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* stub, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  kernels()[stub].name = short_name(device_name);
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}

static struct { dim3 grid, block; size_t lds; hipStream_t st; } pushed;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { pushed = {grid, block, lds, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) {
  *grid = pushed.grid; *block = pushed.block; *lds = pushed.lds; *st = pushed.st;
  return hipSuccess;
}
static std::string name_of(const void* stub) {
  auto it = kernels().find(stub);
  return it == kernels().end() ? "(not registered)" : it->second.name;
}
hipError_t hipLaunchKernel(const void* stub, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  auto it = kernels().find(stub);
  if (it != kernels().end()) it->second.launches++;
  events.push_back({false, name_of(stub), fmt("grid %u,%u,%u block %u", grid.x, grid.y, grid.z, block.x * block.y * block.z), lds});
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* stub, hipFuncAttribute, int value) {
  events.push_back({true, name_of(stub), "", (size_t)value});
  return fail_attr ? hipErrorOutOfMemory : hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
}

// ---------------------------------------------------------------- the requests
using namespace vgpa;

// Registered in the files this program links and never launched by the launchers above, each with the reason ('*': a prefix).
static const struct { const char* kernel; const char* reason; } kNotCovered[] = {
    {"k_ms_untranspose", "launch_ms_untranspose: one kernel, no run-time choice"},
    {"k_edf_dense", "launch_edf: one kernel"},
    {"k_obs*", "launch_obs / launch_obs_dense: not among the launchers of the dispatch header"},
    {"k_reduce", "launch_reduce: one kernel"},
    {"k_trapz_multi", "launch_trapz_multi: one kernel"},
    {"k_mirror_upper", "launch_mirror_upper: one kernel"},
    {"k_unpack_lower", "launch_unpack_lower: one kernel"},
    {"k_psi_from_q", "launch_psi_from_q: one kernel"},
    {"k_lag_start", "launch_lag_start: one kernel"},
    {"k_pf_*", "launch_pf_*: the particle filter's own steps, none of them among the launchers of the dispatch header (k_pf_backward is covered)"},
    {"ld::k_gemm_v<*", "BM = 128 only: launch_gemm's score never prefers 128 rows when M is a multiple of 128 (64 rows give twice the workgroups, "
                       "a balance at least as good, and are worth more), and k_gemm_v takes whole tiles"},
    {"ld::k_gemm<false,false,128,true>", "as k_gemm_v: whole tiles at 128 rows are never chosen"},
    {"ld::k_gemm<false,true,128,true>", "as k_gemm_v"},
    {"ld::k_gemm<true,false,128,true>", "as k_gemm_v"},
    {"ld::k_gemm<true,true,128,true>", "as k_gemm_v"},
    {"ld::k_*", "the element-wise stages, transposes and sharded steps of the D > 64 drivers (ld_solve_*, vgpa_ld_*): no template argument chosen at run time"},
    {"lde::k_gemm_b<true,true,64>", "gemm_b(true, true, ...) has no caller"},
};

static OdeArgs ode(int D) {
  OdeArgs a{};
  a.D = D; a.Np = 9; a.batch = 5; a.dt = 0.01;
  a.A = a.b = a.m0 = a.S0 = a.Sigma = P; a.m = a.S = P;
  a.strideA = (size_t)9 * D * D + 9 * D; a.strideB = a.strideA;
  return a;
}

static void census_steppers() {
  { Scope s("launch_ode_generic");
    for (int method = -1; method <= 4; method++) for (int fwd = 0; fwd < 2; fwd++) for (int D = 0; D <= 65; D++) for (int pj = 0; pj < 2; pj++) {
      OdeArgs a = ode(D);
      a.js_const_stride = pj ? (size_t)D * D : 0;
      request(fmt("method %d fwd %d D %d js_const_stride %d", method, fwd, D, pj), [&] { return launch_ode_generic(method, fwd, a, ST); });
    } }
  { Scope s("launch_ode_small");
    for (int method = -1; method <= 4; method++) for (int fwd = 0; fwd < 2; fwd++) for (int D = 0; D <= 5; D++) for (int bits = 0; bits < 32; bits++) {
      OdeArgs a = ode(D);
      a.msT = ptr<double>(bits & 1); a.Sigma_stride = (bits & 2) ? D * D : 0; a.js_const_stride = (bits & 4) ? D * D : 0;
      a.obs_idx_stride = (bits & 8) ? 9 : 0; a.js_dense = ptr<double>(bits & 16);
      request(fmt("method %d fwd %d D %d msT %d Sigma_stride %d js_const_stride %d obs_idx_stride %d js_dense %d", method, fwd, D, bits & 1, !!(bits & 2),
                  !!(bits & 4), !!(bits & 8), !!(bits & 16)), [&] { return launch_ode_small(method, fwd, a, ST); });
    } }
  { Scope s("launch_ode_wave");
    for (int method = -1; method <= 4; method++) for (int fwd = 0; fwd < 2; fwd++) for (int D = 0; D <= 5; D++) for (int bits = 0; bits < 4; bits++) {
      OdeArgs a = ode(D);
      a.js_dense = ptr<double>(bits & 1); a.js_const_stride = (bits & 2) ? D * D : 0;
      request(fmt("method %d fwd %d D %d js_dense %d js_const_stride %d", method, fwd, D, bits & 1, !!(bits & 2)), [&] { return launch_ode_wave(method, fwd, a, ST); });
    } }
  { Scope s("launch_ode_mfma");
    for (int method = -1; method <= 4; method++) for (int fwd = 0; fwd < 2; fwd++) for (int D = 0; D <= 65; D++) for (int su = 0; su < 2; su++)
      for (int roles = -1; roles <= 3; roles++) for (int bits = 0; bits < 32; bits++) {
        OdeArgs a = ode(D);
        a.sym_units = su; a.q_on = bits & 1; a.grad_on = !!(bits & 2); a.js_dense = ptr<double>(bits & 4); a.js_const_stride = (bits & 8) ? D * D : 0;
        if (bits & 16) { a.s_packed = 1; a.g = P; a.Ef = a.Am = P; }      // what the gradient wave demands (A, b, S, m are always set)
        request(fmt("method %d fwd %d D %d sym_units %d roles %d q_on %d grad_on %d js_dense %d js_const_stride %d grad_operands %d", method, fwd, D, su, roles,
                    bits & 1, !!(bits & 2), !!(bits & 4), !!(bits & 8), !!(bits & 16)), [&] { return launch_ode_mfma(method, fwd, a, roles, ST); });
      } }
}

static void census_lanes() {
  { Scope s("launch_sweep_lane");
    for (int method = -1; method <= 4; method++) for (int model = -1; model <= 4; model++) for (int D = 0; D <= 5; D++) for (int bits = 0; bits < 4096; bits++) {
      if ((bits & 0xe00) && (bits & 0x1ff)) continue;      // the last three (refusals of the whole launcher) one at a time, everything else off
      LaneSweepArgs q{};
      q.o = ode(D); q.model = model; q.o.msT = P; q.f = q.esde = q.g = P; q.eobs = P;
      q.want_grad = bits & 1; q.o.obs_idx_stride = (bits & 2) ? 9 : 0; q.o.jmT = ptr<double>(bits & 4); q.o.js_const_stride = (bits & 8) ? D * D : 0;
      q.o.js_const = ptr<double>(bits & 16); q.theta_v = ptr<double>(bits & 32); q.sigma1_v = ptr<double>(bits & 64); q.isig_v = ptr<double>(bits & 128);
      if (bits & 256) q.o.obs_idx = ptr<int32_t>(true);
      if (bits & 0x200) q.o.js_dense = P;
      if (bits & 0x400) q.o.Np = 1;
      if (bits & 0x800) q.o.msT = nullptr;
      request(fmt("method %d model %d D %d bits %03x", method, model, D, bits), [&] { return launch_sweep_lane(method, q, ST); });
    } }
  { Scope s("launch_theta_lane");
    for (int model = -1; model <= 4; model++) for (int D = 0; D <= 5; D++) for (int pp = 0; pp < 2; pp++) for (int bad = 0; bad < 5; bad++) {
      ThetaLaneArgs q{};
      q.model = model; q.D = D; q.Np = bad == 1 ? 1 : 9; q.batch = 70; q.bpad = 128; q.A = q.b = P; q.msT = ptr<double>(bad != 2); q.out = ptr<double>(bad != 3);
      q.stride_x = bad == 4 ? (size_t)1 << 22 : 99; q.theta_v = ptr<double>(pp);
      request(fmt("model %d D %d theta_v %d refusal %d", model, D, pp, bad), [&] { return launch_theta_lane(q, ST); });
    } }
  { Scope s("launch_obs_lane");
    for (int D = 0; D <= 5; D++) for (int bits = 0; bits < 32; bits++) {
      ObsArgs a{};
      a.D = D; a.Np = 9; a.batch = 70; a.n_obs = 3; a.n_obs_v = ptr<int32_t>(bits & 1); a.obs_const_v = ptr<double>(bits & 2); a.Q_stride = (bits & 4) ? D * D : 0;
      a.K_stride = (bits & 8) ? D * D : 0; a.rinv_stride = (bits & 16) ? D : 0;
      request(fmt("D %d n_obs_v %d obs_const_v %d Q_stride %d K_stride %d rinv_stride %d", D, bits & 1, !!(bits & 2), !!(bits & 4), !!(bits & 8), !!(bits & 16)),
              [&] { return launch_obs_lane(a, P, 128, P, ST); });
    } }
}

static void census_energy_grad() {
  { Scope s("launch_energy");
    for (int model = -1; model <= 4; model++) for (int D = 0; D <= 65; D++) for (int bits = 0; bits < 8; bits++) {
      EnergyArgs a{};
      a.model = model; a.D = D; a.Np = (bits & 4) ? 1 << 20 : 9; a.batch = (bits & 4) ? 1 << 12 : 5;      // (bit 2: more waves than a grid takes)
      a.hyp = ptr<double>(bits & 1); a.tg = ptr<double>(bits & 2);
      request(fmt("model %d D %d hyp %d tg %d Np %d batch %d", model, D, bits & 1, !!(bits & 2), a.Np, a.batch), [&] { return launch_energy(a, ST); });
    } }
  { Scope s("launch_grad");
    for (int D = 0; D <= 65; D++) for (int bits = 0; bits < 16; bits++) {
      GradArgs a{};
      a.D = D; a.Np = 9; a.batch = 5; a.sigma_diag = bits & 1; a.scalar_product = !!(bits & 2); a.psi_is_q = !!(bits & 4); a.Edf = ptr<double>(bits & 8);
      request(fmt("D %d sigma_diag %d scalar_product %d psi_is_q %d Edf %d", D, bits & 1, !!(bits & 2), !!(bits & 4), !!(bits & 8)), [&] { return launch_grad(a, ST); });
    } }
}

static LagArgs lag(int D, int method) {
  LagArgs a{};
  a.D = D; a.Np = 9; a.batch = 5; a.n_anchor = 3; a.stride = 2; a.n_keep = 5; a.method = method; a.dt = 0.01;
  a.A = a.start = P; a.anchors = ptr<int32_t>(true); a.out = P;
  return a;
}
static void census_lag() {
  Scope s("launch_lag");
  for (int method = -1; method <= 4; method++) for (int D = 0; D <= 65; D++) { const LagArgs a = lag(D, method); request(fmt("method %d D %d", method, D), [&] { return launch_lag(a, ST); }); }
  for (int D : {3, 17}) for (int bad = 0; bad < 9; bad++) {      // every other refusal, one at a time
    LagArgs a = lag(D, VGPA_ODE_RK4);
    if (bad == 0) a.A = nullptr;
    if (bad == 1) a.start = nullptr;
    if (bad == 2) a.anchors = nullptr;
    if (bad == 3) a.out = nullptr;
    if (bad == 4) a.Np = 0;
    if (bad == 5) a.batch = 0;
    if (bad == 6) a.n_anchor = 0;
    if (bad == 7) a.stride = 0;
    if (bad == 8) a.n_keep = 4;
    request(fmt("D %d refusal %d", D, bad), [&] { return launch_lag(a, ST); });
  }
}

// A request every field of which the walk `w` wants is set, and none that belongs to another walk.
struct WalkRequest { SampleArgs a; WalkOwn own; MarginalArgs mg; };
static void walk_request(WalkRequest& r, Walk w, int D, int model, int kind, int r_diag, int n_paths) {
  SampleArgs& a = r.a;
  a = SampleArgs{}; r.own = WalkOwn{}; r.mg = MarginalArgs{};
  a.kind = kind; a.model = model; a.D = D; a.Np = 9; a.batch = 5; a.n_paths = n_paths; a.stride = 2; a.n_keep = 5; a.dt = 0.01;
  a.A = a.b = a.R = a.m0 = a.L0 = P; a.R_diag = r_diag; a.stride_x = 999;
  a.obs_t = ptr<int64_t>(true); a.obs_y = a.Q = P; a.n_obs = 2; a.Q_diag = 1;
  const bool seg = w == Walk::Segment || w == Walk::SegmentStats || w == Walk::Conditional || w == Walk::SegmentEvents || w == Walk::Replay ||
                   w == Walk::ReplayCov || w == Walk::ReplayMarginals;
  if (seg) { a.pf_x = a.pf_lw = P; a.k_begin = 2; a.k_end = 6; a.pf_rows = 3; }
  if (w == Walk::Plain) a.out = P;
  if (w == Walk::Weighted) { a.logw = a.start = P; }
  if (w == Walk::SegmentStats || w == Walk::SegmentEvents) a.pf_stats = P;
  if (w == Walk::Conditional) r.own.pf_ref = P;
  if (w == Walk::SegmentEvents) { r.own.ev_level = P; r.own.ev_side = ptr<int32_t>(true); }
  if (w == Walk::Replay || w == Walk::ReplayCov) { a.pf_wtab = P; a.pf_part = P; }
  if (w == Walk::ReplayMarginals) { r.mg.levels = P; r.mg.L = 7; r.mg.qtab = ptr<uint64_t>(true); r.mg.mass = ptr<unsigned long long>(true); r.own.mg = &r.mg; }
  if (w == Walk::Lineage || w == Walk::Backward) { a.out = P; a.pf_slots = ptr<int32_t>(true); a.pf_slot_rows = 3; }
  if (w == Walk::Backward) { a.pf_clouds = P; a.pf_hanc = ptr<int32_t>(true); a.pf_M = 2; a.pf_n = n_paths; }
  if (w == Walk::Forecast) { a.pf_x = P; a.pf_n = n_paths; a.k_begin = 8; a.k_end = 16; a.pf_part = P; a.pf_wtab = P; }      // (the cloud; n_keep = 5)
}
static void census_samplers() {
  const int Ds[] = {0, 1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64, 65};
  { Scope s("launch_sample_walk");
    WalkRequest r;
    for (int w = 0; w <= (int)Walk::ReplayMarginals; w++) for (int D : Ds) for (int model = -1; model <= 4; model++)
      for (int kind : {VGPA_PATHS_POSTERIOR, VGPA_PATHS_MODEL}) for (int r_diag = 0; r_diag < 2; r_diag++) for (int many = 0; many < 2; many++) {
        const int n_paths = many ? sample_max_paths(D < 1 ? 1 : D) + 1 : 300;
        walk_request(r, (Walk)w, D, model, kind, r_diag, n_paths);
        request(fmt("walk %d D %d model %d kind %d R_diag %d n_paths %d", w, D, model, kind, r_diag, n_paths), [&] { return launch_sample_walk((Walk)w, r.a, ST, r.own); });
        if (w == (int)Walk::Plain && !many) {      // the given start, which halves k_sample_l96's LDS
          r.a.x0 = P;
          request(fmt("walk %d D %d model %d kind %d R_diag %d x0", w, D, model, kind, r_diag), [&] { return launch_sample_walk((Walk)w, r.a, ST, r.own); });
        }
        if (w == (int)Walk::Forecast && !many) {      // the members instead of the cloud
          r.a.pf_part = nullptr; r.a.pf_wtab = nullptr; r.a.out = P; r.a.pf_slots = ptr<int32_t>(true); r.a.pf_slot_rows = 1;
          request(fmt("walk %d D %d model %d kind %d R_diag %d members", w, D, model, kind, r_diag), [&] { return launch_sample_walk((Walk)w, r.a, ST, r.own); });
        }
      }
    // a field of another walk: refused whatever the walk
    walk_request(r, Walk::Segment, 3, VGPA_MODEL_L63, VGPA_PATHS_POSTERIOR, 1, 300);
    r.own.pf_ref = P;
    request("walk 2 D 3 with pf_ref", [&] { return launch_sample_walk(Walk::Segment, r.a, ST, r.own); });
  }
  { Scope s("launch_pf_backward");
    for (int D : Ds) for (int model = -1; model <= 4; model++) for (int K : {0, 1, 8, 9, 1000, kBackwardBlock * kMaxGridY + 1}) for (int r_diag = 0; r_diag < 2; r_diag++) {
      PfArgs f{};
      f.D = D; f.batch = 5; f.n_paths = 300; f.M = 2; f.h_flag = ptr<int32_t>(true); f.h_anc = ptr<int32_t>(true); f.h_clouds = f.h_lw = P;
      WalkRequest r;
      walk_request(r, Walk::Segment, D, model, VGPA_PATHS_POSTERIOR, r_diag, 300);
      request(fmt("D %d model %d K %d R_diag %d", D, model, K, r_diag), [&] { return launch_pf_backward(f, r.a, K, 3, ptr<int32_t>(true), ST); });
    } }
}

static void census_large_d() {
  { Scope s("vgpa_ld_gemm (ld::launch_gemm)");
    // M x N: shapes the three tile heights win (the score of launch_gemm; 128 rows: ragged M alone), whole tiles and ragged; K: whole k-tiles in fours, not in fours, ragged
    const int MN[][2] = {{64, 64}, {96, 128}, {512, 512}, {1536, 1536}, {2048, 2048}, {3072, 3072}, {4096, 512}, {100, 72}, {1000, 1000}, {2050, 2048}, {130, 8192}};
    for (auto& mn : MN) for (int K : {64, 48, 1024, 1040, 100}) for (int transa = 0; transa < 2; transa++) for (int bits = 0; bits < 16; bits++) {
      const int M = mn[0], N = mn[1];
      const double* A0 = ptr<double>(true, (bits & 1) ? 8 : 0);
      const double* A1 = (bits & 2) ? ptr<double>(true, (bits & 4) ? 4096 + 8 : 4096) : nullptr;
      const int lda = (transa ? M : K) + ((bits & 8) ? 1 : 0);
      request(fmt("transa %d M %d N %d K %d A0+%d A1 %d+%d lda %d", transa, M, N, K, (bits & 1) ? 8 : 0, !!(bits & 2), (bits & 4) ? 8 : 0, lda),
              [&] { return vgpa_ld_gemm(nullptr, transa, M, N, K, A0, A1, lda, P, N, P, N); });
    }
    for (auto& mn : MN) for (int K : {64, 48, 1024, 1040}) for (int transa = 0; transa < 2; transa++) for (int seg = 0; seg < 3; seg++) for (int acc = 0; acc < 2; acc++)
      for (int mis = 0; mis < 2; mis++) {
        const int M = mn[0], N = mn[1], tiles = seg == 0 ? 0 : seg == 1 ? K / 16 : 1, seg_stride = seg == 0 ? 0 : 4 * K;
        request(fmt("chunk transa %d M %d N %d K %d seg_tiles %d seg_stride %d accumulate %d B+%d", transa, M, N, K, tiles, seg_stride, acc, mis ? 8 : 0),
                [&] { return vgpa_ld_gemm_chunk(nullptr, transa, M, N, K, P, transa ? M : K, ptr<double>(true, mis ? 8 : 0), N, P, N, tiles, seg_stride, acc); });
      } }
  { Scope s("ld::launch_stage_fused");
    for (int kind = 0; kind < 2; kind++) for (int fwd = 0; fwd < 2; fwd++) for (int mid = 0; mid < 2; mid++) for (int D : {65, 96, 100, 1024}) for (int nb : {1, 3}) {
      ld::StageArgs a{};
      a.D = D; a.Mp = D; a.cw = D; a.fwd = fwd; a.nb = nb; a.M0 = P; a.M1 = ptr<double>(mid); a.Xm = P;
      request(fmt("kind %d fwd %d M1 %d D %d nb %d", kind, fwd, mid, D, nb), [&] { return ld::launch_stage_fused(kind, a, ST); });
    } }
  { Scope s("lde_energy / lde_theta_integrand / lde_grad (gemm_b, k_diag64m)");
    hipStream_t side = reinterpret_cast<hipStream_t>(0x200000);
    for (int D : {65, 72, 130, 256, 1024}) for (int Np : {1, 5}) for (int nbmax : {1, 4}) {
      for (int bits = 0; bits < 8; bits++)
        request(fmt("energy D %d Np %d nbmax %d Edf %d hyp %d side %d", D, Np, nbmax, bits & 1, !!(bits & 2), !!(bits & 4)), [&] {
          return ld::lde_energy(D, Np, 8.0, P, P, P, P, P, P, P, ptr<double>(bits & 1), P, P, ptr<int32_t>(true), P, nbmax, ST, ptr<double>(bits & 2), (bits & 4) ? side : nullptr);
        });
      request(fmt("theta_integrand D %d Np %d nbmax %d", D, Np, nbmax), [&] { return ld::lde_theta_integrand(D, Np, 8.0, P, P, P, P, P, P, ptr<int32_t>(true), P, nbmax, ST); });
      for (int dense = 0; dense < 2; dense++)
        request(fmt("grad D %d Np %d nbmax %d isig_dense %d", D, Np, nbmax, dense), [&] { return ld::lde_grad(D, Np, 0.01, P, P, P, P, P, P, P, P, P, P, P, nbmax, ST, ptr<double>(dense)); });
    } }
}

// One request per family that opts in to large dynamic LDS, with the opt-in failing: the error comes back and nothing is launched.
static void census_injected() {
  const bool was_full = full;
  fail_attr = full = true;      // (these few are printed whole)
  std::printf("== hipFuncSetAttribute fails\n");
  {
    Scope s("injected");
    { OdeArgs a = ode(64); request("launch_ode_generic D 64", [&] { return launch_ode_generic(VGPA_ODE_RK4, true, a, ST); }); }
    { OdeArgs a = ode(44); request("launch_ode_mfma D 44 (k_ode_pe)", [&] { return launch_ode_mfma(VGPA_ODE_RK4, true, a, 0, ST); }); }
    { OdeArgs a = ode(64); a.sym_units = 1; request("launch_ode_mfma D 64 (k_ode_sym)", [&] { return launch_ode_mfma(VGPA_ODE_RK4, true, a, 0, ST); }); }
    { EnergyArgs a{}; a.model = VGPA_MODEL_L96; a.D = 64; a.Np = 9; a.batch = 5; a.hyp = P; request("launch_energy L96 D 64 hyp", [&] { return launch_energy(a, ST); }); }
    { GradArgs a{}; a.D = 64; a.Np = 9; a.batch = 5; request("launch_grad D 64 (k_grad)", [&] { return launch_grad(a, ST); });
      a.sigma_diag = 1; request("launch_grad D 64 (k_grad_mfma)", [&] { return launch_grad(a, ST); }); }      // (k_grad_mfma_q stays below the threshold)
    { const LagArgs a = lag(64, VGPA_ODE_RK4); request("launch_lag D 64", [&] { return launch_lag(a, ST); }); }
    { WalkRequest r; walk_request(r, Walk::Segment, 64, VGPA_MODEL_L96, VGPA_PATHS_POSTERIOR, 1, 300);
      request("launch_sample_walk Segment D 64", [&] { return launch_sample_walk(Walk::Segment, r.a, ST, r.own); });
      PfArgs f{}; f.D = 64; f.batch = 5; f.n_paths = 300; f.M = 2; f.h_flag = ptr<int32_t>(true); f.h_anc = ptr<int32_t>(true); f.h_clouds = f.h_lw = P;
      request("launch_pf_backward D 64", [&] { return launch_pf_backward(f, r.a, 8, 3, ptr<int32_t>(true), ST); }); }
    request("lde_energy D 72 (k_diag64m)", [&] { return ld::lde_energy(72, 1, 8.0, P, P, P, P, P, P, P, nullptr, P, P, ptr<int32_t>(true), P, 1, ST, nullptr, nullptr); });
  }
  full = was_full;
  fail_attr = false;
}

int main(int argc, char** argv) {
  full = argc > 1 && std::strcmp(argv[1], "--full") == 0;
  outcomes = argc > 1 && std::strcmp(argv[1], "--outcomes") == 0;
  std::printf("kernels registered: %zu\n", kernels().size());
  census_steppers();
  census_lanes();
  census_energy_grad();
  census_lag();
  census_samplers();
  census_large_d();
  census_injected();
  std::set<std::string> idle;
  std::map<std::string, std::vector<std::string>> excused;
  for (auto& k : kernels()) {
    if (k.second.launches) continue;
    const char* why = nullptr;
    for (auto& e : kNotCovered) {
      const size_t n = std::strlen(e.kernel);
      if (!why && (e.kernel[n - 1] == '*' ? k.second.name.compare(0, n - 1, e.kernel, n - 1) == 0 : k.second.name == e.kernel)) why = e.reason;
    }
    if (why) excused[why].push_back(k.second.name);
    else idle.insert(k.second.name);
  }
  for (auto& e : excused) {
    std::sort(e.second.begin(), e.second.end());
    std::printf("never launched, excused (%s):", e.first.c_str());
    for (auto& n : e.second) std::printf(" %s", n.c_str());
    std::printf("\n");
  }
  std::printf("registered, never launched, not excused: %zu\n", idle.size());
  for (auto& n : idle) std::printf("  %s\n", n.c_str());
  return idle.empty() ? 0 : 1;
}
