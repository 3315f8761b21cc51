// engine.cpp -- host runtime behind include/rainier_hip.h.
//
// rh_model   : RIR -> (emit.cpp) HIP source -> hiprtc -> code object (cached on disk by content hash, the
//              "compile once per Model" of core/Model.scala:32-34) -> hipModule; observation columns copied to HBM.
// rh_sampler : device-resident state of all chains + the launch loop that drives rh_chain_kernel.
// All device work goes to the engine's own stream; HIP events on that stream give the kernel timings bench.py reports.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/rainier_hip.h"
#include "../../include/rainier_hip_rir.h"
#include "device/rh_shared.h"
#include "rir.hpp"
#include "optimize.hpp"
#include "engine_internal.hpp"
#include "lanes_plan.hpp"

// device sources embedded at build time (see Makefile: device_src.inc)
const char *const kSharedSrc =
#include "gen/rh_shared.inc"
    ;
const char *const kPreludeSrc =
#include "gen/rh_prelude.inc"
    ;
static const char *kEngineSrc =
#include "gen/rh_engine.inc"
    ;
static const char *kLaneSrc =
#include "gen/rh_lane.inc"
    ;
namespace {
thread_local std::string g_err;
std::atomic<long> g_compiles{0};   // hiprtc compilations of this process (cache misses): rh_compile_count

uint64_t fnv1a(const std::string &s, uint64_t h = 1469598103934665603ULL) {
  for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ULL; }
  return h;
}

std::string lib_dir() {
  Dl_info info;
  if (dladdr((void *)&fnv1a, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    auto pos = p.find_last_of('/');
    return pos == std::string::npos ? "." : p.substr(0, pos);
  }
  return ".";
}
std::string cache_dir() {
  const char *env = std::getenv("RH_KERNEL_CACHE");
  std::string d = env && *env ? env : lib_dir() + "/kcache";
  mkdir(d.c_str(), 0700);
  return d;
}
bool read_file(const std::string &path, std::vector<char> &out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return !out.empty();
}
void write_file(const std::string &path, const std::vector<char> &data) {
  const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
  { std::ofstream f(tmp, std::ios::binary); f.write(data.data(), (std::streamsize)data.size()); }
  std::rename(tmp.c_str(), path.c_str());
}

// hiprtc: source -> gfx950 code object
std::vector<std::string> split_flags(const std::string &flags) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < flags.size()) {
    size_t j = flags.find_first_of(" ,", i);
    if (j == std::string::npos) j = flags.size();
    if (j > i) out.push_back(flags.substr(i, j - i));
    i = j + 1;
  }
  return out;
}
std::vector<char> compile_hip(const std::string &src, const std::string &arch, const std::string &extra, std::string &log) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "rainier_model.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    throw Fail{RH_E_COMPILE, "hiprtcCreateProgram failed"};
  const std::string archopt = "--offload-arch=" + arch;
  std::vector<const char *> opts = {archopt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"};
  const std::vector<std::string> more = split_flags(extra);
  for (const std::string &f : more) opts.push_back(f.c_str());
  const hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  size_t ls = 0;
  hiprtcGetProgramLogSize(prog, &ls);
  log.assign(ls, '\0');
  if (ls) hiprtcGetProgramLog(prog, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    hiprtcDestroyProgram(&prog);
    throw Fail{RH_E_COMPILE, "hiprtc compile failed:\n" + log};
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  std::vector<char> code(cs);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  return code;
}
}  // namespace
std::string &thread_err() { return g_err; }

struct KSet {  // the per-chain sampler kernels of one compiled variant (with / without NUTS support)
  hipModule_t module = nullptr;
  hipFunction_t k_chain = nullptr, k_tick = nullptr;   // nullptr: absent, or not fit to run (why_chain / why_tick say which)
  std::string why_chain, why_tick;
  int state_words = 0, dense_off = 0;  // dense_off: u64 word offset of the dense-mass rows in the state image
  int off_Pq = -1, off_Pg = -1, off_PU = -1;   // u64 word offsets in a chain's image the create-time self-check reads
  bool chain_checked = false, tick_checked = false;
  bool loaded = false;
};

struct rh_model {
  KSet variants[8];  // sampler-kernel variants by (NUTS ? 1 : 0) | (dense mass ? 2 : 0); [0] aliases the base module; built on first use
  bool want_nuts = false;
  rh::Program prog;
  rh::EmitOptions eopt;
  rh::EmitInfo info;
  int mass_vec = 9;  // index of M in the state image (read back from the module: rh_state_mass_vec)
  std::string source, err, arch;
  std::vector<char> code;
  int device = 0;
  bool loaded = false;
  hipModule_t module = nullptr;
  hipFunction_t k_chain = nullptr, k_density = nullptr, k_selftest = nullptr, k_grad = nullptr, k_tick = nullptr;
  hipFunction_t k_grad_fused = nullptr;  // rh_grad_kernel + the mid-trajectory leapfrog update as its prologue (static HMC); absent when the model does not qualify
  hipFunction_t k_absorb = nullptr;      // the fused launches' per-chain records -> state image, before the tick that ends a trajectory
  hipFunction_t k_compact = nullptr;     // active flags -> ascending list of the chains that wait for a gradient (rh_compact_kernel)
  // the lane walk (rh_grad_lane_kernel: chains in the lanes, rows in scalar registers): a code object of its own, empty / nullptr when
  // the model does not qualify (lane_eligible) or the kernel is not fit to run
  std::vector<char> lane_code;
  hipModule_t lane_module = nullptr;
  hipFunction_t k_grad_lane = nullptr;
  int grad_chains_req = 0;               // rh_compile_opts.grad_chains as the caller gave it (0 = automatic)
  bool lane_tried = false;               // build_lane_code has run (lane_code is final)
  int lane_r = 0;                        // rows per scalar request of the kernel in lane_code (8 or 4; 0: none)
  // the lane walk's row feed (rh_grad_lane_kernel of a second code object: the same walk, the rows from an interleaved copy of each target's columns,
  // lanes_plan.hpp): one more code object, empty / nullptr when no row target is eligible or the kernel is not fit to run
  std::vector<char> lane_rows_code;
  std::string lane_rows_why;             // why the model has lane_code but no lane_rows_code (empty: no target is eligible)
  hipModule_t lane_rows_module = nullptr;
  hipFunction_t k_grad_lane_rows = nullptr;
  bool lane_rows_tried = false;          // build_lane_rows_code has run (lane_rows_code is final)
  std::vector<void *> dev_rows;          // per row target (ROWT order) the interleaved copy on the device, or nullptr (made by ensure_lane_rows)
  std::vector<long long> dev_rows_n;     // ... and the rows it holds: a launch whose data.nrows asks for more takes the column feed
  std::vector<long long> rows_uploaded;  // per target the rows of its columns as uploaded (data.nrows may be a prefix for a while: selfcheck_density)
  int ncols_max = 0, glm_ncols = 0;
  hipFunction_t k_grad_glm = nullptr;
  bool glm_small = false;  // <= 8 predictors: the plain VALU kernel (the fp64 matrix pipe pays from ~9 predictors on, profiles/r1_c)
  bool lk_lds = false;     // the kernels keep rh_logit_link's table in LDS (6176 B of static LDS: RH_LK_LDS_BYTES in rh_prelude.hip.h)
  bool has_glm = false;  // the emitter found a dense linear predictor: rh_grad_glm_kernel (fp64 MFMA) exists
  int n_row_targets_hint = 0; // row targets of the lowered program (known before the module is loaded)
  bool shape_guessed = false;    // assemble_source has made its first guesses from the size of the generated code
  bool rows_unroll_auto = true;  // the chain-per-wavefront kernels' row unroll is the engine's choice (rh_compile_opts.rows_unroll == 0)
  bool unroll_auto = false;  // the row-loop unroll was the engine's choice (not the caller's): it may be reduced for a heavy row function
  int gather_waves = 3;  // wavefronts per SIMD rh_grad_gather_kernel is compiled for (amdgpu_waves_per_eu; 1 = the allocator's choice)
  int glm_w = 4;  // wavefronts (16 chains each) per workgroup of rh_grad_glm_kernel: 4 measured best on cfg 4 (profiles/r2_c_cfg4)
  int n_row_targets = 0, grad_k = 4, nacc_max = 1;
  // gather mode: per row target (ROWT order) the host copy of the group offsets (rows sorted by table index)
  hipFunction_t k_grad_gather = nullptr, k_density_fin = nullptr;
  hipFunction_t k_grad_gather_scan = nullptr;   // the same launch for the row targets whose groups have fewer than 64 rows (rh_grad_gather_scan_kernel)
  std::vector<std::vector<int>> goff_host;   // [rowt][ngroups + 1]
  std::vector<void *> goff_dev;              // device copies
  std::vector<int> gather_count;             // per rowt: table size (0 = no gather)
  int state_words = 0;
  rh_model_data data{};
  std::vector<void *> dev_cols;
  void *d_coltab = nullptr;                  // device table of the column pointers (rh_model_data.cols)
  void *d_kpool = nullptr;                   // the constant pool of the data-free targets (rh_model_data.kpool; EmitInfo::kpool is the host copy)
  std::vector<std::vector<int64_t>> col_len; // ... and the length of every block (0xFFFFFFFF in col_src = a block of zeros)
  std::vector<std::vector<double>> synth_cols; // columns lifted out of many same-shaped data-free targets (lift.cpp)
  std::vector<std::vector<uint32_t>> col_src; // engine column -> the caller's columns concatenated into it (one, unless the
                                             // target was rolled back from Model.observe's 8-way split: refactor.cpp)
  int64_t rows_total = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::recursive_mutex engine_mu;   // rh_sampler_create: engine choice + the create-time engine self-check, which updates the variant's
                                    // shared kernel set (recursive: the self-check creates a sampler of its own on this thread)
  // what the code object's kernels are fit for (kernel_health): an engine whose kernels are not is never chosen, and an explicit
  // request for it fails with RH_E_UNSUPPORTED and the reason
  bool chain_ok = false, density_ok = false, tick_ok = false;
  std::string chain_why, density_why, tick_why;
  int compile_attempts = 0;   // code objects built or fetched for this model (re-lowering included)
  bool selfcheck_done = false;
};

namespace { struct GatherBufs; }

// Tick engine: what one chain population needs to advance on its own.  A sampler has one lane, or two that part its chains on a
// chain-group boundary (lanes_plan.hpp) and run on two streams: chains never interact, and while one lane sits between two
// launches, in a tick or in a launch's prologue, the other lane's gradient launch has the fp64 pipe.  The per-chain arrays (state,
// seeds, draws, stats, qbuf, active, records) stay the sampler's single allocations; a lane holds views at its first chain, and its
// kernels number the chains from there (lists, partial sums and scatter sums are lane-local).
struct Lane {
  int first = 0, chains = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;         // (lane 0 runs on the model's stream)
  hipEvent_t e0 = nullptr, e1 = nullptr;   // the span of a call's first tick
  // Two event pools, used by alternate rounds: r0 / r1 the span of the round that used the pool, ev[2 i], ev[2 i + 1] around its
  // gradient launch i.  A pool is recorded again only after the round that used it has been resolved (resolve_round).
  hipEvent_t r0[2] = {nullptr, nullptr}, r1[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> ev[2];
  void *d_running = nullptr, *d_list = nullptr, *d_nlive = nullptr, *d_graderr = nullptr;
  void *d_livelog = nullptr;       // [round cap + 1] live counts logged by rh_compact_kernel, one per tick of a round (+, in the last slot, the call's first tick)
  void *d_partial = nullptr, *d_partial2 = nullptr;   // (the second one: fused launches)
  int pp = 0;                      // which of the two partial-sum / record buffers the next launch writes
  int cur_live = 0;                // chains in the list the next gradient launch serves
  GatherBufs *gb = nullptr;
  // views into the sampler's arrays at chain `first`
  void *state = nullptr, *seeds = nullptr, *draws = nullptr, *stats = nullptr, *qbuf = nullptr, *active = nullptr, *rec[2] = {nullptr, nullptr};
  // host side of a round in flight
  int running = 0, B = 0;
  long long remaining = 0;         // gradient launches this call still has to do (exact in a lock-step run; lanes_plan.hpp round_launches)
  long long pos = 0;               // gradient launches since the first tick of this call
  bool live = false;               // still advancing in this call
  bool pending = false, prev_rec = false;   // the previous launch's gradient has not been consumed by a tick / it left records
  // per event pool, for resolve_round: the host copy of the round's live log and which of its launches a tick followed
  std::vector<int> livelog[2];
  std::vector<char> was_ticked[2];
};
// A finished round whose timing figures have not been read out of its events yet (resolve_round)
struct RoundRec {
  bool open = false;
  int pool = 0;
  bool live[2] = {false, false};   // the lanes that took part
  int B[2] = {0, 0};               // ... and their launches
};

struct rh_sampler {
  hipFunction_t k_chain = nullptr, k_tick = nullptr;
  int state_words = 0, dense_off = 0, pack_l = 64;  // pack_l: lanes per chain of the chosen chain kernel
  int off_Pq = -1, off_Pg = -1, off_PU = -1;        // u64 word offsets of (q, gradient at q, -logp at q) of the current point in a chain's image
  rh_model *m = nullptr;
  rh_cfg_dev cfg{};
  int chains = 0;
  void *d_state = nullptr, *d_seeds = nullptr, *d_mass = nullptr, *d_draws = nullptr, *d_stats = nullptr, *d_running = nullptr;
  int it_done = 0;  // sampling iterations completed
  bool started = false, warmed = false;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double kernel_ms = 0, total_ms = 0;
  // live-chain accounting of the tick engine's gradient launches (rh_timing.chain_slots / steady_*)
  int64_t chain_slots = 0, steady_launches = 0, steady_evals = 0;
  double steady_ms = 0;
  int64_t launches = 0;
  // tick engine
  bool tick_engine = false;
  int nsplit = 0, xcd_aware = 1;
  bool compact = true;             // gradient launches and ticks serve the listed (live) chains only
  void *d_qbuf = nullptr, *d_active = nullptr;
  void *d_rec[2] = {nullptr, nullptr};  // fused launches: the two record buffers (alternating)
  bool fuse = false;  // static HMC on the plain gradient kernel: mid-trajectory updates run as the gradient launch's epilogue
  bool lane_walk = false;          // the gradient launches are rh_grad_lane_kernel's (lanes_plan.hpp walk_is_lane; fixed at creation)
  bool lane_rows = false;          // ... the row-fed rh_grad_lane_kernel's: the lane walk fed from the interleaved copies (feed_is_rows; fixed at creation)
  std::vector<Lane> lanes;         // one, or two halves of the chains on two streams (lanes_plan.hpp)
  int round_cap = 0;               // gradient launches per lane of a round at the most (lanes_plan.hpp round_cap; RH_ROUND_MAX)
  int next_pool = 0;               // the event pool the next round records
  RoundRec round;                  // the last round, until its figures have been added to kernel_ms ... launches above
  std::vector<rh_chain_stats_dev> last_stats;
  int64_t grads_at_reset = 0;
};
int guard(rh_model *m, const std::function<void()> &fn) {
  try { fn(); return RH_OK; }
  catch (const Fail &f) { g_err = f.msg; if (m) m->err = f.msg; return f.code; }
  catch (const std::exception &e) { g_err = e.what(); if (m) m->err = e.what(); return RH_E_INVALID; }
}
DrawsView sampler_draws(rh_sampler *s) {
  return {s->d_draws, s->m->device, s->m->stream, s->chains, s->it_done, (int)s->m->prog.n_params, s->cfg.iterations, &s->m->mu, &s->m->err, s->m};
}

namespace {

void assemble_source(rh_model *m) {
  std::string defines, targets, err;
  if (const char *e = rh::knob("RH_GRAD_PIPELINE")) m->eopt.grad_pipeline = std::atoi(e);
  if (const char *e = rh::knob("RH_FMA_ADDS")) m->eopt.fma_adds = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_XFUSE")) m->eopt.xfuse = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_SIMPLIFY")) m->eopt.simplify = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_PACK")) m->eopt.pack = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_FAST_LOG")) m->eopt.fast_log = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_FORCE_BIGN")) m->eopt.force_bign = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_LOGIT_LINK")) m->eopt.logit_link = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_CONST_POOL")) m->eopt.const_pool = std::atoi(e) != 0;
  if (const char *e = rh::knob("RH_CHUNK")) if (m->eopt.chunk == 0) m->eopt.chunk = std::max(0, std::atoi(e));   // tests: the memory-resident lowering for any model
  if (m->eopt.chunk > 0) {   // the memory-resident lowering comes with the lightest kernel shapes and without the special-cased rows
    m->eopt.rows_unroll = 1; m->eopt.grad_unroll = 1; m->eopt.grad_pipeline = 0; m->unroll_auto = false;
    m->eopt.grad_chains = 1;
  }
  if (const char *e = rh::knob("RH_GATHER_MIN")) m->eopt.gather_min = std::max(1, std::atoi(e));  // tests: gather mode for small tables
  {  // tick-engine defaults from the register budget: K*NACC fp64 accumulators + U*NCOLS row values per lane
    int ncols_max = 1;
    for (auto &T : m->prog.targets) ncols_max = std::max<int>(ncols_max, (int)T.n_cols);
    // rolling pipeline: a load has the other U-1 tiles' arithmetic to land behind, so U is 8 where the row values fit
    // (measured on cfg 2, profiles/r3_a_cfg2/sweep.txt: U 6..16 within 1 %, U = 4 is 4 % slower)
    if (m->eopt.grad_unroll <= 0) {
      m->eopt.grad_unroll = m->eopt.grad_pipeline == 2 ? std::max(1, std::min(8, 32 / ncols_max)) : std::max(1, std::min(4, 16 / ncols_max));
      m->unroll_auto = true;
    }
  }
  if (!rh::emit_hip(m->prog, m->eopt, defines, targets, err, &m->info)) throw Fail{RH_E_UNSUPPORTED, err};
  m->n_row_targets_hint = 0;
  for (const auto &T : m->prog.targets) if (T.n_cols) m->n_row_targets_hint++;
  if (!m->shape_guessed) {
    // First guesses that spare a heavy model the attempts it is known to lose (each one a compilation of tens of seconds): a
    // generated function of more than 1000 statements goes to the memory-resident lowering at once, and a generic model beyond 512
    // parameters (theta and the outputs in memory, chain vectors in HBM) starts big mode's vector loops at 4 slots in flight --
    // where the 601- and 701-parameter state-space models of the tests end up after five attempts otherwise.
    m->shape_guessed = true;
    size_t longest = 0;
    for (size_t at = targets.find("void row("); at != std::string::npos; at = targets.find("void row(", at + 1)) {
      const size_t end = targets.find("\n  }\n", at);
      size_t c = 0;
      for (size_t i = targets.find("\n    const double n", at); i != std::string::npos && i < end; i = targets.find("\n    const double n", i + 1)) c++;
      longest = std::max(longest, c);
    }
    bool again = false;
    if (longest > 1000 && m->eopt.chunk == 0 && !rh::knob("RH_NO_CHUNKS")) {
      m->eopt.chunk = 48; again = true;
      if (!rh::knob("RH_CHAIN_WAVES")) m->eopt.chain_waves = 1;   // (such a model's chain kernel has never fitted two wavefronts per SIMD)
    }
    if (m->info.bign && !m->info.gather_mode && m->prog.n_params > 512 && m->eopt.big_unroll > 4) { m->eopt.big_unroll = 4; again = true; }
    if (again) { assemble_source(m); return; }
  }
  if (m->rows_unroll_auto && m->eopt.rows_unroll > 1 && m->n_row_targets_hint > 0) {
    // the chain-per-wavefront kernels' row unroll: four copies of a light row function hide the loads; a heavier one brings its own
    // parallelism and would only be lowered again after the compiler has spilled (build_code) -- start where those models end up
    size_t row_ops = 1;
    for (size_t hr = targets.find("HAS_ROWS = true;"); hr != std::string::npos; hr = targets.find("HAS_ROWS = true;", hr + 1)) {
      const size_t at = targets.find("void row(", hr);
      if (at == std::string::npos) break;
      const size_t end = std::min(targets.find("void row_g(", at), targets.find("void finish(", at));   // (row() only: row_g() repeats a part of it)
      size_t c = 0;
      for (size_t i = targets.find("\n    const double n", at); i != std::string::npos && i < end; i = targets.find("\n    const double n", i + 1)) c++;
      row_ops = std::max(row_ops, c);
    }
    if (row_ops > 24) {
      m->eopt.rows_unroll = 1;
      defines.clear(); targets.clear();
      if (!rh::emit_hip(m->prog, m->eopt, defines, targets, err, &m->info)) throw Fail{RH_E_UNSUPPORTED, err};
    }
  }
  if ((m->unroll_auto && m->eopt.grad_unroll > 1) || (m->eopt.grad_chains == 0 && m->info.grad_k > 1 && !m->info.gather_mode)) {
    // ... and where the row function is light: the unrolled body is K x U copies of it (cfg 2: 8 x 8 x 11 statements); a heavy row
    // function brings its own instruction-level parallelism and would only spill (build_code checks what the compiler did).
    // The weight is read off the code just generated: the statements of the longest row() body.  Budget: K x U x statements <= 720;
    // tiles go first, then chains per wavefront (when the caller left them to the engine).
    size_t row_ops = 1;
    for (size_t hr = targets.find("HAS_ROWS = true;"); hr != std::string::npos; hr = targets.find("HAS_ROWS = true;", hr + 1)) {
      const size_t at = targets.find("void row(", hr);
      if (at == std::string::npos) break;
      const size_t end = std::min(targets.find("void row_g(", at), targets.find("void finish(", at));   // (row() only: row_g() repeats a part of it)
      size_t c = 0;
      for (size_t i = targets.find("\n    const double n", at); i != std::string::npos && i < end; i = targets.find("\n    const double n", i + 1)) c++;
      row_ops = std::max(row_ops, c);
    }
    auto pow2floor = [](size_t v) { size_t p = 1; while (p * 2 <= v) p *= 2; return (int)p; };
    int k = std::max(1, m->info.grad_k), u = m->eopt.grad_unroll;
    if (m->eopt.grad_chains == 0 && !m->info.gather_mode && (size_t)k * row_ops > 720) k = std::min(k, pow2floor(std::max<size_t>(1, 720 / row_ops)));
    if (m->unroll_auto) u = std::min(u, pow2floor(std::max<size_t>(1, 720 / ((size_t)k * row_ops))));
    if (k != m->info.grad_k || u != m->eopt.grad_unroll) {
      if (k != m->info.grad_k) m->eopt.grad_chains = k;
      m->eopt.grad_unroll = u;
      defines.clear(); targets.clear();
      if (!rh::emit_hip(m->prog, m->eopt, defines, targets, err, &m->info)) throw Fail{RH_E_UNSUPPORTED, err};
    }
  }
  m->nacc_max = m->info.nacc_max;
  m->grad_k = m->info.grad_k;
  m->has_glm = m->info.glm_target >= 0;
  m->glm_small = m->info.glm_small;
  // experiment knobs of the MFMA GLM kernel (workgroup waves, forced waves per SIMD, scalar-part unroll)
  if (const char *e = rh::knob("RH_GLM_W")) { m->glm_w = std::max(1, std::min(16, std::atoi(e))); }
  defines += "#define RH_GLM_W " + std::to_string(m->glm_w) + "\n";
  if (const char *e = rh::knob("RH_GRAD_WAVES")) defines += "#define RH_GRAD_WAVES " + std::to_string(std::atoi(e)) + "\n";
  if (const char *e = rh::knob("RH_CHAIN_WAVES")) m->eopt.chain_waves = std::max(1, std::atoi(e));
  defines += "#define RH_CHAIN_WAVES " + std::to_string(m->eopt.chain_waves) + "\n";
  if (const char *e = rh::knob("RH_GLM_WPS")) defines += "#define RH_GLM_WAVES_PER_SIMD " + std::to_string(std::atoi(e)) + "\n";
  if (const char *e = rh::knob("RH_FUSE_SYNC")) defines += "#define RH_FUSE_SYNC " + std::to_string(std::atoi(e)) + "\n";
  if (const char *e = rh::knob("RH_TICK_FAST")) defines += "#define RH_TICK_FAST " + std::to_string(std::atoi(e)) + "\n";
  // rh_grad_gather_kernel asks for three wavefronts per SIMD (168 registers: cfg 5's K = 4 walk with its two-tile pipeline fits without
  // a spill; left alone the allocator takes 169 -- two wavefronts); a model that does not fit gets the unconstrained build (build_code)
  if (const char *e = rh::knob("RH_GATHER_WAVES")) m->gather_waves = std::max(1, std::atoi(e));
  defines += "#define RH_GATHER_WAVES " + std::to_string(m->gather_waves) + "\n";
  if (const char *e = rh::knob("RH_GATHER_V2")) defines += "#define RH_GATHER_V2 " + std::to_string(std::atoi(e)) + "\n";
  if (const char *e = rh::knob("RH_GLM_EU")) defines += "#define RH_GLM_ELEM_UNROLL " + std::to_string(std::atoi(e)) + "\n";
  // row code that calls the closed-form logit link reads its table from LDS (rh_prelude.hip.h: RH_LK_LDS)
  { bool lds = targets.find("rh_logit_link(") != std::string::npos;
    if (const char *e = rh::knob("RH_LK_LDS")) lds = lds && std::atoi(e) != 0;
    m->lk_lds = lds;
    if (lds) defines += "#define RH_LK_LDS 1\n"; }
  m->source = "// generated by rainier-hip: RIR -> HIP (gfx950), one translation unit per model\n" + defines + kSharedSrc +
              "\n" + kPreludeSrc + "\n// ---- generated from RIR -------------------------------------------\n" + targets + "\n" +
              kEngineSrc;
}

// Which compiler hiprtc dispatches to is a property of the PROCESS, not of the hiprtc version number: a process that imported
// torch first runs torch's bundled libhiprtc / comgr (another LLVM under the same API version), which produces different code for
// the same source.  The cache key therefore carries the identity of the hiprtc library actually bound -- the file behind
// hiprtcCompileProgram (name of the resolved file + its size) -- and, when one is already loaded, of the comgr library next to it.
std::string compiler_identity() {
  static const std::string id = [] {
    auto ident = [](const char *path) {
      std::string out = "?";
      if (!path) return out;
      char real[4096];
      const char *rp = realpath(path, real) ? real : path;
      struct stat st;
      const char *slash = std::strrchr(rp, '/');
      out = slash ? slash + 1 : rp;
      if (stat(rp, &st) == 0) out += ":" + std::to_string((long long)st.st_size);
      return out;
    };
    std::string r;
    Dl_info info;
    if (dladdr((void *)&hiprtcCompileProgram, &info) && info.dli_fname) r = ident(info.dli_fname);
    for (const char *soname : {"libamd_comgr.so.3", "libamd_comgr.so.2", "libamd_comgr.so"}) {
      void *h = dlopen(soname, RTLD_NOLOAD | RTLD_LAZY);
      if (!h) continue;
      void *sym = dlsym(h, "amd_comgr_get_version");
      if (sym && dladdr(sym, &info) && info.dli_fname) r += "+" + ident(info.dli_fname);
      dlclose(h);
      break;
    }
    return r;
  }();
  return id;
}
std::string cache_path(const std::string &arch, const std::string &source, const std::string &extra) {
  int hv = 0;
  hiprtcVersion(&hv, &hv);
  const uint64_t h = fnv1a(arch + "|" + std::to_string(hv) + "|" + compiler_identity() + "|" + extra + "|" + source);
  char name[64];
  std::snprintf(name, sizeof name, "/%016llx", (unsigned long long)h);
  return cache_dir() + name;
}
// suffix: ".hsaco" for a model's code object; the model-independent ones (rh_trace.hip.h, rh_summary.hip.h) are kept apart under a name of their own,
// so that what sweeps the cache's *.hsaco files (the census of GENERATED control flow, tools/unproven_census.py) sees models only
}  // namespace
std::vector<char> build_source(const std::string &arch, const std::string &source, const std::string &extra, const char *suffix) {
  const std::string path = cache_path(arch, source, extra) + suffix;
  std::vector<char> code;
  if (!std::getenv("RH_NO_KERNEL_CACHE") && read_file(path, code)) return code;
  std::string log;
  code = compile_hip(source, arch, extra, log);
  g_compiles++;
  if (!std::getenv("RH_NO_KERNEL_CACHE")) write_file(path, code);
  return code;
}
namespace {
// An attempt the engine abandons (build_code lowers the model again with a lighter shape) is not kept as a code object: a small
// marker with the kernels that were unfit takes its place, so that the next process takes the same decision without compiling.
// (a marker records a verdict of kernel_health: it carries the version of those rules and whether they were switched off, and a marker
//  written under other rules is ignored -- the attempt is compiled and judged again)
const int kHealthRulesVersion = 3;   // 3: round 6 (rh_grad_gather_scan_kernel joins the gather-mode ladder); 2: round 5 (rh_grad_gather_kernel's wavefront request; the gather walk without a divergent region)
std::string marker_header() {
  return "rules=" + std::to_string(kHealthRulesVersion) + " allow_unhealthy=" + (rh::unsafe_knob("RH_ALLOW_UNHEALTHY") ? "1" : "0") + "\n";
}
void abandon_attempt(const std::string &arch, const std::string &source, const std::string &extra, const std::string &unfit) {
  if (std::getenv("RH_NO_KERNEL_CACHE")) return;
  const std::string base = cache_path(arch, source, extra);
  std::remove((base + ".hsaco").c_str());
  const std::string text = marker_header() + unfit;
  write_file(base + ".unfit", std::vector<char>(text.begin(), text.end()));
}
bool abandoned_attempt(const std::string &arch, const std::string &source, const std::string &extra, std::string &unfit) {
  if (std::getenv("RH_NO_KERNEL_CACHE")) return false;
  std::vector<char> b;
  if (!read_file(cache_path(arch, source, extra) + ".unfit", b)) return false;
  const std::string text(b.begin(), b.end()), head = marker_header();
  if (text.compare(0, head.size(), head) != 0) return false;
  unfit = text.substr(head.size());
  return true;
}
const char *kNutsDefine = "#define RH_WITH_NUTS 1\n";

// ---- which kernels of a code object the engine agrees to launch ---------------------------------------------------------------
// A kernel is launched only if (1) its metadata reports NO spilled vector registers and (2) the static check of isacheck.cpp finds
// no vector instruction ahead of a join block's exec restore.  Both guard against the same fault of this toolchain's register
// allocator (spill code and live-range copies placed before `s_or_b64 exec, exec, s[a:b]` run under the mask of the region that
// just ended; root-caused in round 4 on rh_chain_kernel of hier_negbin(6, 7): profiles/r4_spill_rootcause).  A kernel
// that fails is replaced by a lighter build of itself (row unroll, chains per wavefront, wavefronts per SIMD) or by another engine;
// when nothing is left the call fails with RH_E_UNSUPPORTED -- it is never run.  RH_ALLOW_UNHEALTHY=1 (diagnostics: reproducing the
// fault on a GPU) switches the rule off.
}  // namespace
int kernel_health(const std::vector<char> &code, const std::string &name, std::string *why) {
  rh::KernelMeta km;
  std::vector<std::string> names;
  if (!rh::list_kernels(code, names)) { if (why) *why = name + ": the code object cannot be read"; return KH_BAD; }
  if (std::find(names.begin(), names.end(), name) == names.end()) return KH_ABSENT;
  if (rh::unsafe_knob("RH_ALLOW_UNHEALTHY")) return KH_OK;
  if (!rh::kernel_meta(code, name, km)) { if (why) *why = name + ": no metadata entry (spill count unknown)"; return KH_BAD; }
  // The count includes the allocator's VGPR -> AGPR copies: without a single scratch instruction in the kernel nothing went to
  // memory.  That reading is granted to the SAMPLER kernels only (rh_chain_kernel / rh_tick_kernel: their NUTS variants carry 64
  // such copies and are bit-compared with the oracle on the device); the row-streaming and density kernels -- the shapes that
  // returned wrong sums in round 3 -- stay on the plain rule: any spill count sends them to a lighter shape.
  const bool sampler_kernel = name == "rh_chain_kernel" || name == "rh_tick_kernel";
  if (km.vgpr_spills != 0 && !(sampler_kernel && rh::kernel_touches_scratch(code, name) == 0)) {
    if (why) *why = name + ": " + std::to_string(km.vgpr_spills) + " spilled vector registers";
    return KH_BAD;
  }
  std::vector<std::string> findings;
  if (!rh::check_code_object(code, name, findings) || !findings.empty()) {
    if (why) *why = findings.empty() ? name + ": machine code could not be walked" : findings[0];
    return KH_BAD;
  }
  return KH_OK;
}
namespace {

// Lower, compile, look at what the compiler did, and lower again with a lighter shape while a kernel the model would launch is
// not fit to run (every attempt is cached under its own key, so this costs a parse after the first time; the attempts are counted
// in m->compile_attempts).  What is still unfit afterwards is recorded by load_module (m->chain_ok, m->tick_ok, ...).
void build_code(rh_model *m) {
  const char *e = rh::knob("RH_HIPRTC_EXTRA");
  const std::string extra = e ? e : "";
  const bool keep = rh::knob("RH_KEEP_UNROLL") != nullptr;
  for (;;) {
    m->compile_attempts++;
    std::string unfit;   // "\n"-separated names of the unfit kernels of an attempt that was abandoned before
    const bool marker = !keep && abandoned_attempt(m->arch, m->source, extra, unfit);
    const auto t_attempt = std::chrono::steady_clock::now();
    if (!marker) m->code = build_source(m->arch, m->source, extra);
    if (rh::knob("RH_BUILD_LOG")) {   // diagnostics: what every attempt cost and which shape it had
      std::string unfit_now;
      for (const char *k : {"rh_chain_kernel", "rh_density_kernel", "rh_grad_kernel", "rh_grad_fused_kernel", "rh_grad_gather_kernel", "rh_grad_gather_scan_kernel", "rh_tick_kernel", "rh_density_fin_kernel"})
        if (marker ? unfit.find(std::string("\n") + k + "\n") != std::string::npos : kernel_health(m->code, k) == KH_BAD) unfit_now += std::string(" ") + k;
      std::fprintf(stderr, "[rh build] attempt %d%s: %.1f s, %zu KB source, rows_unroll %d grad_unroll %d K %d waves %d pipeline %d chunk %d bigu %d gwaves %d; unfit:%s\n",
                   m->compile_attempts, marker ? " (marker)" : "", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_attempt).count(),
                   m->source.size() / 1024, m->eopt.rows_unroll, m->eopt.grad_unroll, m->info.grad_k, m->eopt.chain_waves, m->eopt.grad_pipeline,
                   m->eopt.chunk, m->eopt.big_unroll, m->gather_waves, unfit_now.empty() ? " none" : unfit_now.c_str());
    }
    if (keep) return;
    // (one verdict per kernel and attempt: kernel_health parses the ELF and walks the machine code of the kernel and of every device
    //  function each time it is asked, and the ladder below asks a dozen times)
    std::map<std::string, int> verdicts;
    auto health = [&](const char *k) {
      auto it = verdicts.find(k);
      if (it == verdicts.end()) it = verdicts.emplace(k, kernel_health(m->code, k)).first;
      return it->second;
    };
    auto bad = [&](const char *k) {
      if (marker) return unfit.find(std::string("\n") + k + "\n") != std::string::npos;
      return health(k) == KH_BAD;
    };
    auto again = [&] {   // this attempt is abandoned: leave the marker, lower again
      if (!marker) {
        std::string names = "\n";
        for (const char *k : {"rh_chain_kernel", "rh_density_kernel", "rh_grad_kernel", "rh_grad_fused_kernel", "rh_grad_gather_kernel", "rh_grad_gather_scan_kernel",
                              "rh_tick_kernel", "rh_density_fin_kernel"})
          if (health(k) == KH_BAD) names += std::string(k) + "\n";
        abandon_attempt(m->arch, m->source, extra, names);
      }
      assemble_source(m);
    };
    // The last resort: when what has been built leaves the model without a sampling engine or without a density path, it is
    // lowered again in the memory-resident form (emit.cpp chunk_body: the generated functions cut into chunks, values travelling
    // through a per-lane scratch array -- the analogue of the reference's method splitting, ir/Packer.scala:10-71), with smaller
    // chunks while that does not fit either.  Slower, same bits, any size.
    auto usable = [&] {
      if (m->info.gather_mode) return !bad("rh_grad_gather_kernel") && !bad("rh_grad_gather_scan_kernel") && !bad("rh_tick_kernel") && !bad("rh_density_fin_kernel");
      // (a dense linear predictor's gradients come from the MFMA kernel: load_module prefers it, so it can stand in for rh_grad_kernel)
      const bool glm = m->has_glm && m->n_row_targets_hint == 1 && !m->glm_small && !marker && health("rh_grad_glm_kernel") == KH_OK;
      const bool tick = m->n_row_targets_hint > 0 && (!bad("rh_grad_kernel") || glm) && !bad("rh_tick_kernel") && !bad("rh_density_fin_kernel");
      return tick || (!bad("rh_chain_kernel") && !bad("rh_density_kernel"));
    };
    auto heavier = [&] {
      if (rh::knob("RH_NO_CHUNKS")) return false;
      if (m->eopt.chunk == 0) { m->eopt.chunk = 48; return true; }   // (assemble_source sets what goes with it)
      if (m->eopt.chunk > 12) { m->eopt.chunk /= 2; return true; }
      return false;
    };
    // big mode (chain vectors in HBM): the vector loops keep RH_BIGU slots in flight per lane; fewer while a sampler kernel does not fit
    if (m->info.bign && m->eopt.chunk == 0 && m->eopt.big_unroll > 2 && (bad("rh_tick_kernel") || bad("rh_chain_kernel"))) {
      m->eopt.big_unroll /= 2; again(); continue;
    }
    if (m->info.gather_mode) {   // K chains per wavefront x ~14 wave-uniform doubles each: fewer chains is the only lever
      if (bad("rh_grad_gather_kernel") && m->gather_waves > 1 && !rh::knob("RH_GATHER_WAVES")) { m->gather_waves = 1; again(); continue; }
      if ((bad("rh_grad_gather_kernel") || bad("rh_grad_gather_scan_kernel")) && m->info.grad_k > 1) { m->eopt.grad_chains = m->info.grad_k / 2; again(); continue; }
      if (!usable() && heavier()) { again(); continue; }
      if (marker) m->code = build_source(m->arch, m->source, extra);   // (abandoned under other settings: it is the last shape now)
      return;
    }
    // the chain-per-wavefront kernels walk the rows with RH_ROWS_UNROLL copies of the row function per iteration (the unroll does
    // not change a lane's summation order, so the results are the same bits)
    if (m->n_row_targets_hint > 0 && m->eopt.rows_unroll > 1 && (bad("rh_density_kernel") || bad("rh_chain_kernel"))) {
      m->eopt.rows_unroll /= 2;
      again();
      continue;
    }
    // rh_chain_kernel asks for two wavefronts per SIMD (256 registers: +47 % on cfg 3); a model that does not fit gets one (512)
    if (bad("rh_chain_kernel") && m->eopt.chain_waves != 1 && !rh::knob("RH_CHAIN_WAVES")) { m->eopt.chain_waves = 1; again(); continue; }
    if (bad("rh_grad_kernel") || bad("rh_grad_fused_kernel")) {
      // first fewer tiles per chunk, then fewer chains per wavefront; a row function that does not fit even alone keeps the plain row loop
      bool lighter = true;
      if (m->eopt.grad_unroll > 1) m->eopt.grad_unroll /= 2;
      else if (m->info.grad_k > 1) m->eopt.grad_chains = m->info.grad_k / 2;
      else if (m->eopt.grad_pipeline != 0) m->eopt.grad_pipeline = 0;
      else lighter = false;
      if (lighter) { again(); continue; }
    }
    if (!usable() && heavier()) { again(); continue; }
    if (marker) m->code = build_source(m->arch, m->source, extra);   // (abandoned under other settings: it is the last shape now)
    return;
  }
}

// The lane walk's code object: the model's own translation unit once more with rh_lane.hip.h behind it (rh_grad_lane_kernel).  Kept
// apart from the models' *.hsaco (like the predictors'): only that kernel is taken from it.  Built for the models the walk fits
// -- plain row streaming, chain-group size left to the engine, R rows of every column in scalar registers, the workgroup's sums in
// LDS -- and kept only if the kernel passes the engine's own fitness checks without a spill or a byte of scratch.
int lane_ncols_max(const rh_model *m) {
  int ncols_max = 0;
  for (const auto &T : m->prog.targets) ncols_max = std::max<int>(ncols_max, (int)T.n_cols);
  return ncols_max;
}
bool lane_eligible(const rh_model *m) {
  const int ncols_max = lane_ncols_max(m);
  const bool glm = m->has_glm && m->n_row_targets_hint == 1 && !m->glm_small;
  return m->n_row_targets_hint > 0 && !m->info.gather_mode && !m->info.bign && m->eopt.chunk == 0 && !glm && !m->lk_lds &&
         m->grad_chains_req == 0 && !m->want_nuts && rh_plan::lane_walk_fits_r(ncols_max, m->nacc_max, 4);
}
// Rows per scalar request: 8 where the kernel fits, else 4 (a strict build's row code leaves fewer scalar registers); a shape that
// does not compile or does not fit leaves a marker in the cache, like an abandoned attempt of build_code, and is not compiled again.
void build_lane_code(rh_model *m) {
  m->lane_code.clear();
  m->lane_r = 0;
  m->lane_tried = true;
  if (!lane_eligible(m)) return;
  const char *e = rh::knob("RH_HIPRTC_EXTRA");
  const std::string extra = e ? e : "";
  const bool cache = !std::getenv("RH_NO_KERNEL_CACHE");
  for (int R : {8, 4}) {
    if (!rh_plan::lane_walk_fits_r(lane_ncols_max(m), m->nacc_max, R)) continue;
    const std::string src = (R == rh_plan::kLaneR ? std::string() : "#define RH_LANE_R " + std::to_string(R) + "\n") + m->source + "\n" + kLaneSrc;
    const std::string marker = cache_path(m->arch, src, extra) + ".lane.unfit";
    std::vector<char> mk;
    if (cache && read_file(marker, mk) && std::string(mk.begin(), mk.end()).compare(0, marker_header().size(), marker_header()) == 0) continue;
    bool fit = false;
    std::string why;
    rh::KernelMeta km;
    std::vector<char> code;
    try {
      code = build_source(m->arch, src, extra, ".lane.co");
      fit = kernel_health(code, "rh_grad_lane_kernel", &why) == KH_OK && rh::kernel_meta(code, "rh_grad_lane_kernel", km) && km.vgpr_spills == 0 &&
            km.sgpr_spills == 0 && km.scratch_bytes == 0 && rh::kernel_touches_scratch(code, "rh_grad_lane_kernel") == 0;
    } catch (const Fail &f) { why = f.msg; }   // (row code the walk cannot hold does not compile)
    if (rh::knob("RH_BUILD_LOG"))
      std::fprintf(stderr, "[rh build] lane walk R %d: vgprs %ld sgprs %ld spills %ld/%ld scratch %ld: %s %s\n", R, km.vgprs, km.sgprs, km.vgpr_spills,
                   km.sgpr_spills, km.scratch_bytes, fit ? "fit" : "unfit", why.c_str());
    if (fit) { m->lane_code = code; m->lane_r = R; return; }
    if (cache) {
      std::remove((cache_path(m->arch, src, extra) + ".lane.co").c_str());
      const std::string text = marker_header() + "\nrh_grad_lane_kernel\n";   // (the form of build_code's markers: the unfit kernels)
      write_file(marker, std::vector<char>(text.begin(), text.end()));
    }
  }
}
// The lane walk's kernel, built and loaded the first time a sampler or an evaluation could take it (nullptr: the model has none)
hipFunction_t fit_kernel(const std::vector<char> &code, hipModule_t module, const char *name, std::string *why = nullptr);
hipFunction_t ensure_lane(rh_model *m) {
  std::lock_guard<std::recursive_mutex> lk(m->engine_mu);
  if (m->k_grad_lane) return m->k_grad_lane;
  if (!m->k_grad || !m->k_tick || m->info.gather_mode) return nullptr;
  if (!m->lane_tried) build_lane_code(m);
  if (m->lane_code.empty() || m->lane_module) return nullptr;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipModuleLoadData(&m->lane_module, m->lane_code.data()));
  m->k_grad_lane = fit_kernel(m->lane_code, m->lane_module, "rh_grad_lane_kernel", nullptr);
  return m->k_grad_lane;
}

// The row feed's code object: the lane walk's translation unit with RH_LANE_FEED_ROWS in front (rh_grad_lane_kernel in its row-fed
// form), at the rows per block the column feed settled on -- the two cut the rows alike, so a chain's sums are the same
// bits.  Kept under the column feed's conditions, and only if it keeps the eight wavefronts per SIMD where the column feed has them.
bool lane_rows_any_target(const rh_model *m) {
  for (const auto &T : m->prog.targets) if (T.n_cols && rh_plan::lane_rows_eligible((int)T.n_cols, m->lane_r)) return true;
  return false;
}
void build_lane_rows_code(rh_model *m) {
  const char *K = "rh_grad_lane_kernel";   // (the row-fed entry point has the column-fed one's name, in a code object of its own)
  m->lane_rows_code.clear();
  m->lane_rows_why.clear();
  m->lane_rows_tried = true;
  if (m->lane_code.empty() || !lane_rows_any_target(m)) return;
  const char *e = rh::knob("RH_HIPRTC_EXTRA");
  const std::string extra = e ? e : "";
  const bool cache = !std::getenv("RH_NO_KERNEL_CACHE");
  const std::string src = "#define RH_LANE_FEED_ROWS 1\n" + (m->lane_r == rh_plan::kLaneR ? std::string() : "#define RH_LANE_R " + std::to_string(m->lane_r) + "\n") +
                          m->source + "\n" + kLaneSrc;
  // (the marker has the form of build_code's: the unfit kernels; the reason, for the build report, lies in a file of its own beside it)
  const std::string marker = cache_path(m->arch, src, extra) + ".lanerows.unfit", reason = cache_path(m->arch, src, extra) + ".lanerows.why";
  std::vector<char> mk;
  if (cache && read_file(marker, mk) && std::string(mk.begin(), mk.end()).compare(0, marker_header().size(), marker_header()) == 0) {
    m->lane_rows_why = read_file(reason, mk) ? std::string(mk.begin(), mk.end()) : "unfit";
    return;
  }
  bool fit = false;
  std::string why;
  rh::KernelMeta km, kc;
  std::vector<char> code;
  try {
    code = build_source(m->arch, src, extra, ".lanerows.co");
    fit = kernel_health(code, K, &why) == KH_OK && rh::kernel_meta(code, K, km);
    if (fit && (km.vgpr_spills != 0 || km.sgpr_spills != 0 || km.scratch_bytes != 0 || rh::kernel_touches_scratch(code, K) != 0)) { fit = false; why = "spills or scratch"; }
    if (fit && rh::kernel_meta(m->lane_code, "rh_grad_lane_kernel", kc) && kc.vgprs <= 64 && km.vgprs > 64) {
      fit = false; why = std::to_string(km.vgprs) + " vector registers where the column feed has " + std::to_string(kc.vgprs) + ": eight wavefronts per SIMD would be lost";
    }
  } catch (const Fail &f) { why = f.msg; }
  if (rh::knob("RH_BUILD_LOG"))
    std::fprintf(stderr, "[rh build] lane walk row feed R %d: vgprs %ld sgprs %ld spills %ld/%ld scratch %ld: %s %s\n", m->lane_r, km.vgprs, km.sgprs, km.vgpr_spills,
                 km.sgpr_spills, km.scratch_bytes, fit ? "fit" : "unfit", why.c_str());
  if (fit) { m->lane_rows_code = code; return; }
  m->lane_rows_why = why.empty() ? "unfit" : why;
  if (cache) {
    std::remove((cache_path(m->arch, src, extra) + ".lanerows.co").c_str());
    const std::string text = marker_header() + "\n" + K + "\n";
    write_file(reason, std::vector<char>(m->lane_rows_why.begin(), m->lane_rows_why.end()));
    write_file(marker, std::vector<char>(text.begin(), text.end()));
  }
}
// The row feed's kernel and the interleaved copies it reads, made the first time a sampler or an evaluation could take it -- once per
// model and device, rows x NC x 8 bytes per eligible target -- (nullptr: the model has none)
hipFunction_t ensure_lane_rows(rh_model *m) {
  std::lock_guard<std::recursive_mutex> lk(m->engine_mu);
  if (m->k_grad_lane_rows) return m->k_grad_lane_rows;
  if (!ensure_lane(m)) return nullptr;
  if (!m->lane_rows_tried) build_lane_rows_code(m);
  if (m->lane_rows_code.empty() || m->lane_rows_module) return nullptr;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipModuleLoadData(&m->lane_rows_module, m->lane_rows_code.data()));
  hipFunction_t k = fit_kernel(m->lane_rows_code, m->lane_rows_module, "rh_grad_lane_kernel", nullptr);
  if (!k) return nullptr;
  // The copies hold ALL the rows of the uploaded columns (rows_uploaded), whatever prefix data.nrows names at the moment -- the
  // create-time self-check evaluates prefixes and may be the first to come here.  One column at a time goes through the host.  The
  // copies are optional: where one cannot be made (no memory) the model has no row feed and its launches take the column feed.
  m->dev_rows.assign((size_t)m->n_row_targets, nullptr);
  m->dev_rows_n.assign((size_t)m->n_row_targets, 0);
  try {
    size_t c = 0, rowt = 0;
    for (size_t t = 0; t < m->prog.targets.size(); t++) {
      const int nc = (int)m->prog.targets[t].n_cols;
      if (!nc) continue;
      if (rh_plan::lane_rows_eligible(nc, m->lane_r)) {
        const long long rows = t < m->rows_uploaded.size() ? m->rows_uploaded[t] : 0;
        std::vector<double> col((size_t)rows), inter((size_t)rh_plan::lane_rows_doubles(rows, nc), 0.0);
        for (int j = 0; j < nc; j++) {
          if (rows) HIPCHK(hipMemcpy(col.data(), m->dev_cols[c + (size_t)j], sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost));
          rh_plan::lane_rows_place_column(col.data(), rows, nc, j, inter.data());
        }
        void *d = nullptr;   // (hipMalloc's addresses are aligned to far more than a 64-byte line)
        HIPCHK(hipMalloc(&d, std::max<size_t>(64, inter.size() * sizeof(double))));
        m->dev_rows[rowt] = d;
        m->dev_rows_n[rowt] = rows;
        if (!inter.empty()) HIPCHK(hipMemcpy(d, inter.data(), inter.size() * sizeof(double), hipMemcpyHostToDevice));
      }
      c += (size_t)nc; rowt++;
    }
  } catch (const Fail &) {
    (void)hipGetLastError();
    for (void *d : m->dev_rows) if (d) (void)hipFree(d);
    m->dev_rows.clear(); m->dev_rows_n.clear();
    return nullptr;   // (lane_rows_module stays loaded: not tried again)
  } catch (const std::bad_alloc &) {
    for (void *d : m->dev_rows) if (d) (void)hipFree(d);
    m->dev_rows.clear(); m->dev_rows_n.clear();
    return nullptr;
  }
  m->k_grad_lane_rows = k;
  return k;
}

// kernel `name` of `module` if it is fit to run (kernel_health); otherwise nullptr and the reason
hipFunction_t fit_kernel(const std::vector<char> &code, hipModule_t module, const char *name, std::string *why) {
  std::string w;
  const int h = kernel_health(code, name, &w);
  if (h != KH_OK) {
    if (why) *why = h == KH_BAD ? w : std::string(name) + " is not part of this build";
    return nullptr;
  }
  hipFunction_t f = nullptr;
  HIPCHK(hipModuleGetFunction(&f, module, name));
  return f;
}

void load_module(rh_model *m) {
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipModuleLoadData(&m->module, m->code.data()));
  HIPCHK(hipModuleGetFunction(&m->k_selftest, m->module, "rh_selftest_kernel"));
  m->n_row_targets = 0;
  for (auto &T : m->prog.targets) if (T.n_cols) m->n_row_targets++;
  std::string wg, wf, wt;
  if (m->info.gather_mode) {  // parameter table indexed by a data column: tick engine with the group-major gather kernel only
    m->k_grad_gather = fit_kernel(m->code, m->module, "rh_grad_gather_kernel", &wg);
    { std::string ws;   // (needed only when the data have a gather target with small groups; both must be fit for the tick engine to be)
      m->k_grad_gather_scan = fit_kernel(m->code, m->module, "rh_grad_gather_scan_kernel", &ws);
      if (m->k_grad_gather && !m->k_grad_gather_scan) { m->k_grad_gather = nullptr; wg = ws; } }
    m->k_density_fin = fit_kernel(m->code, m->module, "rh_density_fin_kernel", &wf);
    m->k_tick = fit_kernel(m->code, m->module, "rh_tick_kernel", &wt);
    m->tick_ok = m->k_grad_gather && m->k_density_fin && m->k_tick;
    m->tick_why = !m->k_grad_gather ? wg : (!m->k_density_fin ? wf : wt);
    m->chain_why = m->density_why = "gather-mode models run on the tick engine only";
  } else {
    m->k_chain = fit_kernel(m->code, m->module, "rh_chain_kernel", &m->chain_why);
    m->k_density = fit_kernel(m->code, m->module, "rh_density_kernel", &m->density_why);
    m->chain_ok = m->k_chain != nullptr; m->density_ok = m->k_density != nullptr;
    m->tick_why = "the tick engine needs a model that streams rows";
  }
  if (m->n_row_targets > 0 && !m->info.gather_mode) {  // the tick engine only exists for models that stream rows
    m->k_grad = fit_kernel(m->code, m->module, "rh_grad_kernel", &wg);
    m->k_tick = fit_kernel(m->code, m->module, "rh_tick_kernel", &wt);
    m->k_density_fin = fit_kernel(m->code, m->module, "rh_density_fin_kernel", &wf);
    // compiled only for models whose chain group fits one wavefront's lanes (RH_HAVE_FUSED in rh_engine.hip.h)
    m->k_grad_fused = fit_kernel(m->code, m->module, "rh_grad_fused_kernel");
    m->k_absorb = fit_kernel(m->code, m->module, "rh_absorb_kernel");
    if (!m->k_absorb) m->k_grad_fused = nullptr;
  }
  if (m->n_row_targets > 0) m->k_compact = fit_kernel(m->code, m->module, "rh_compact_kernel");   // (unfit: every launch serves every chain)
  m->ncols_max = 0;
  for (auto &T : m->prog.targets) m->ncols_max = std::max<int>(m->ncols_max, (int)T.n_cols);
  // Dense linear predictors of more than 8 terms run both contractions on the fp64 matrix cores (rh_grad_glm_kernel).  Up to 8 the
  // plain VALU kernel wins (measured, profiles/r1_c: fp64 MFMA and fp64 VALU do not overlap and have the same peak, so moving eta to
  // the matrix cores only adds AGPR traffic) and no GLM kernel is built.  (Two more row-streaming kernels were measured and removed
  // in round 6 because they lost to these two: a hybrid for <= 8 predictors -- eta on the matrix cores, the sums on the VALU -- and
  // a VALU kernel whose workgroups share LDS-staged row tiles, VALU/occupancy-bound on cfg 4 like the register kernel; git history.)
  if (m->has_glm && m->n_row_targets == 1 && !m->info.gather_mode && !m->glm_small)
    m->k_grad_glm = fit_kernel(m->code, m->module, "rh_grad_glm_kernel");   // (unfit: the plain VALU kernel)
  if (m->has_glm) m->glm_ncols = (int)m->prog.targets[(size_t)m->info.glm_target].n_cols;
  // (Round 3 also measured the contractions OFF the matrix pipe -- one chain per lane, row values scalar-loaded as SGPR operands,
  //  162 VALU instructions per 64 evaluations: 33.9 vs 17.5 ms, bound by scalar-load latency; git 28d5e00, profiles/r3_cfg4.)
  // one 64-row tile of all columns must fit the CU's LDS (310 columns); wider dense predictors stay on the plain VALU kernel
  {  // (column-major, stride 66)
    const size_t tile = (size_t)m->glm_ncols * 66u * sizeof(double);
    if (tile + (m->lk_lds ? 6176u : 0u) > 160u * 1024u) m->k_grad_glm = nullptr;
  }
  if (const char *e = rh::knob("RH_GLM_MFMA")) if (std::atoi(e) == 0) m->k_grad_glm = nullptr;
  if (m->n_row_targets > 0 && !m->info.gather_mode) {
    m->tick_ok = m->k_tick && m->k_density_fin && (m->k_grad || m->k_grad_glm);
    m->tick_why = !m->k_tick ? wt : (!m->k_density_fin ? wf : wg);
  }
  if (!m->density_ok && !m->tick_ok)
    throw Fail{RH_E_UNSUPPORTED, "no kernel of this model is fit to run on this toolchain (the model is too heavy for the register file): " +
                                  (m->info.gather_mode ? m->tick_why : m->density_why + (m->n_row_targets > 0 ? "; " + m->tick_why : std::string()))};
  hipDeviceptr_t p; size_t sz;
  HIPCHK(hipModuleGetGlobal(&p, &sz, m->module, "rh_state_words"));
  HIPCHK(hipMemcpy(&m->state_words, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipModuleGetGlobal(&p, &sz, m->module, "rh_state_mass_vec"));  // same position in every sampler-kernel variant
  HIPCHK(hipMemcpy(&m->mass_vec, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  m->loaded = true;
}

// sampler-kernel variants: the same translation unit with RH_WITH_NUTS / RH_WITH_DENSE defined (larger chain state);
// only their per-chain kernels are used, so plain HMC/EHMC with diagonal mass pay nothing for them
std::string variant_defines(int v) {
  std::string d;
  if (v & 1) d += kNutsDefine;
  if (v & 2) d += "#define RH_WITH_DENSE 1\n";
  if (v & 4) d += "#define RH_PACK_L 64\n";  // one chain per wavefront although the model packs (few or diverging chains)
  return d;
}
// the code object of sampler-kernel variant v (v > 0) of a model whose base module has been built.  A variant's chain state is
// larger than the base module's (NUTS: seven more vectors, the tree's scalars), so its per-chain kernels may not fit where the base
// module's do: it is then built with one wavefront per SIMD for rh_chain_kernel and / or fewer slots in flight in big mode's vector
// loops (only the variant's per-chain kernels are used, so the base module's choices are not affected).  The first build whose
// sampler kernels are all fit is taken; otherwise the one with the most.
std::vector<char> build_variant_code(rh_model *m, int v) {
  const char *extra = rh::knob("RH_HIPRTC_EXTRA");  // the same flags as the base module (build_code)
  auto with = [&](int waves, int bigu) {
    std::string src = m->source;
    auto swap = [&](const std::string &name, int from, int to) {
      const std::string a = "#define " + name + " " + std::to_string(from) + "\n";
      const size_t at = src.find(a);
      if (at != std::string::npos && from != to) src.replace(at, a.size(), "#define " + name + " " + std::to_string(to) + "\n");
    };
    swap("RH_CHAIN_WAVES", m->eopt.chain_waves, waves);
    swap("RH_BIGU", m->eopt.big_unroll, bigu);
    m->compile_attempts++;
    return build_source(m->arch, variant_defines(v) + src, extra ? extra : "");
  };
  auto nfit = [&](const std::vector<char> &code) {
    int n = 0;
    if (!m->info.gather_mode && kernel_health(code, "rh_chain_kernel") != KH_BAD) n++;
    if (m->n_row_targets_hint > 0 && kernel_health(code, "rh_tick_kernel") != KH_BAD) n++;
    return n;
  };
  const int want = (m->info.gather_mode ? 0 : 1) + (m->n_row_targets_hint > 0 ? 1 : 0);
  std::vector<std::pair<int, int>> shapes = {{m->eopt.chain_waves, m->eopt.big_unroll}};
  if (!rh::knob("RH_CHAIN_WAVES") && m->eopt.chain_waves != 1 && !m->info.gather_mode) shapes.push_back({1, m->eopt.big_unroll});
  if (m->info.bign) for (int u = m->eopt.big_unroll / 2; u >= 2; u /= 2) shapes.push_back({1, u});
  std::vector<char> best;
  int best_n = -1;
  for (auto &sh : shapes) {
    std::vector<char> code = with(m->info.gather_mode ? m->eopt.chain_waves : sh.first, sh.second);
    const int n = nfit(code);
    if (n > best_n) { best_n = n; best.swap(code); }
    if (best_n >= want) break;
  }
  return best;
}
void read_state_offsets(KSet &ks) {
  hipDeviceptr_t p; size_t sz;
  HIPCHK(hipModuleGetGlobal(&p, &sz, ks.module, "rh_state_words"));
  HIPCHK(hipMemcpy(&ks.state_words, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipModuleGetGlobal(&p, &sz, ks.module, "rh_state_off_Pq"));
  HIPCHK(hipMemcpy(&ks.off_Pq, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipModuleGetGlobal(&p, &sz, ks.module, "rh_state_off_Pg"));
  HIPCHK(hipMemcpy(&ks.off_Pg, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipModuleGetGlobal(&p, &sz, ks.module, "rh_state_off_PU"));
  HIPCHK(hipMemcpy(&ks.off_PU, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
}
KSet &load_variant(rh_model *m, int v) {
  KSet &ks = m->variants[v];
  if (ks.loaded) return ks;
  HIPCHK(hipSetDevice(m->device));
  if (v == 0) {
    ks.module = m->module; ks.k_chain = m->k_chain; ks.k_tick = m->tick_ok ? m->k_tick : nullptr; ks.why_chain = m->chain_why; ks.why_tick = m->tick_why;
    read_state_offsets(ks);
    ks.loaded = true;
    return ks;
  }
  const std::vector<char> code = build_variant_code(m, v);
  HIPCHK(hipModuleLoadData(&ks.module, code.data()));
  if (!m->info.gather_mode) ks.k_chain = fit_kernel(code, ks.module, "rh_chain_kernel", &ks.why_chain);
  else ks.why_chain = "gather-mode models run on the tick engine only";
  if (m->n_row_targets > 0) ks.k_tick = fit_kernel(code, ks.module, "rh_tick_kernel", &ks.why_tick);
  else ks.why_tick = "the tick engine needs a model that streams rows";
  if (ks.k_tick && !m->tick_ok) { ks.k_tick = nullptr; ks.why_tick = m->tick_why; }   // the gradient kernels are the base module's
  read_state_offsets(ks);
  hipDeviceptr_t p; size_t sz;
  if (v & 2) {
    HIPCHK(hipModuleGetGlobal(&p, &sz, ks.module, "rh_state_dense_off"));
    HIPCHK(hipMemcpy(&ks.dense_off, (void *)p, sizeof(int), hipMemcpyDeviceToHost));
  }
  ks.loaded = true;
  return ks;
}


// rh_compile_opts -> emitter options, validated once for rh_model_create and rh_lower_only; returns the device ordinal
int apply_compile_opts(rh_model *m, const rh_compile_opts *opts) {
  if (!opts) return -1;
  if (opts->struct_size != (int32_t)sizeof(rh_compile_opts)) throw Fail{RH_E_INVALID, "rh_compile_opts.struct_size mismatch"};
  if (opts->math_mode != RH_MATH_FAST && opts->math_mode != RH_MATH_STRICT) throw Fail{RH_E_INVALID, "unknown math_mode"};
  m->eopt.strict_math = opts->math_mode == RH_MATH_STRICT;
  m->eopt.fp_contract = opts->fp_contract != 0;
  if (opts->rows_unroll < 0 || opts->rows_unroll > 64) throw Fail{RH_E_INVALID, "rows_unroll out of range [0,64]"};
  if (opts->rows_unroll > 0) { m->eopt.rows_unroll = opts->rows_unroll; m->rows_unroll_auto = false; }
  if (opts->grad_chains < 0 || opts->grad_chains > 16 || opts->grad_unroll < 0 || opts->grad_unroll > 16)
    throw Fail{RH_E_INVALID, "grad_chains / grad_unroll out of range [0,16]"};
  m->eopt.grad_chains = opts->grad_chains; m->eopt.grad_unroll = opts->grad_unroll;
  m->grad_chains_req = opts->grad_chains;
  m->eopt.factor_outputs = opts->factor_outputs != 0;
  if (opts->with_nuts < 0 || opts->with_nuts > 7) throw Fail{RH_E_INVALID, "with_nuts: unknown variant bits"};
  m->want_nuts = opts->with_nuts != 0;
  return opts->device;
}

// parse; when there are more targets than the engine holds: many data-free targets of one shape become one streamed target
// (lift.cpp: its columns are synthesised and owned by the model) and the remaining runs of data-free targets are merged.  cols =
// the caller's column pointers followed by the synthesised ones; nrows_m = the row count of every target that is left.
void load_program(rh_model *m, const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows,
                  std::vector<const double *> &cols, std::vector<int64_t> &nrows_m, bool tables_without_data = false) {
  std::string err;
  if (!rh::parse_rir(rir, rir_len, m->prog, err)) throw Fail{RH_E_INVALID, err};
  if (m->prog.kind != 0) throw Fail{RH_E_INVALID, "a density program (header kind 0) is needed"};
  const uint32_t caller_cols = m->prog.n_cols_total;
  std::vector<uint32_t> old1, old2;
  bool lift = true;
  if (const char *e = rh::knob("RH_LIFT_CONSTANTS")) lift = std::atoi(e) != 0;
  if (lift) rh::lift_constants(m->prog, m->synth_cols, old1);
  else for (uint32_t t = 0; t < m->prog.targets.size(); t++) old1.push_back(t);
  // (rh_lower_only has no data: the preparation of parameter tables for gather mode synthesises columns NEXT TO the caller's, and
  //  what follows from it -- canonicalisation, re-derivation, rolling -- needs all of them, so it waits for rh_model_create)
  //  -- unless the caller only wants to see the lifted program: rh_lift_rir)
  const bool have_data = columns != nullptr || caller_cols == 0 || tables_without_data;
  if (have_data) {  // a gather-shaped parameter table whose prior is data-free: the prior terms become a row target over the group index (lift.cpp)
    bool lp = true;
    if (const char *e = rh::knob("RH_LIFT_PRIORS")) lp = std::atoi(e) != 0;
    int gmin = m->eopt.gather_min;
    if (const char *e = rh::knob("RH_GATHER_MIN")) gmin = std::max(1, std::atoi(e));
    bool hoist = lp;
    if (const char *e = rh::knob("RH_HOIST_TABLES")) hoist = std::atoi(e) != 0;
    if (hoist) rh::hoist_table_maps(m->prog, gmin);
    // (fast builds also lift a prior that ties the entries to shared parameters -- the centred parameterisation -- with both
    //  gradients derived again and verified: lift.cpp)
    if (lp && rh::lift_table_priors(m->prog, m->synth_cols, gmin, m->eopt.fp_contract)) old1.push_back(0xFFFFFFFFu);
    if (lp) for (int k = rh::lift_single_entry_targets(m->prog, m->synth_cols, gmin); k > 0; k--) old1.push_back(0xFFFFFFFFu);
  }
  rh::merge_data_free_targets(m->prog, old2);
  if (m->prog.targets.size() > RH_MAX_TARGETS)
    throw Fail{RH_E_UNSUPPORTED, "more than 64 targets are left after merging the data-free ones (RH_MAX_TARGETS)"};
  cols.clear();
  for (uint32_t c = 0; c < caller_cols; c++) cols.push_back(columns ? columns[c] : nullptr);   // (rh_lower_only has no data)
  for (const auto &sc : m->synth_cols) cols.push_back(sc.data());
  nrows_m.assign(m->prog.targets.size(), 0);
  for (size_t t = 0; t < m->prog.targets.size(); t++) {
    if (!m->prog.targets[t].n_cols) continue;
    const uint32_t orig = old1[old2[t]];
    if (orig == 0xFFFFFFFFu) nrows_m[t] = (int64_t)m->synth_cols[m->prog.targets[t].col0 - caller_cols].size();   // a lifted group
    else nrows_m[t] = nrows ? nrows[orig] : -1;
  }
}

// derived columns (copies, negations, products, affine images, constants) -> expressions over the base columns (columns.cpp);
// fills m->col_src (engine column -> the caller's columns it is made of) and the per-target row counts
void canonicalize_once(rh_model *m, const double *const *columns, const int64_t *nrows, std::vector<int64_t> &nrows_t, bool allow_unroll,
                       bool *unroll_blocked = nullptr);
// Fast builds first try WITHOUT unrolling Model.observe's initial chunk: after the gradient re-derivation the chunk is the same
// function as a slot of the big target and is appended to it as rows (refactor.cpp), so no observation is written into the
// generated source and the code-object cache keeps working across data sets.  If a small row target is still there afterwards
// (not isomorphic, loose data columns, ...), or in strict builds, the chunk is unrolled into a data-free target instead.
void canonicalize(rh_model *m, const double *const *columns, const int64_t *nrows, std::vector<int64_t> &nrows_t) {
  if (m->eopt.fp_contract && m->eopt.simplify && m->prog.n_cols_total > 0) {
    const rh::Program saved = m->prog;
    bool blocked = false;                     // gather mode keeps the chunk as a row target: a second attempt would change nothing
    canonicalize_once(m, columns, nrows, nrows_t, false, &blocked);
    if (blocked) return;
    int64_t big = 0; bool small_left = false;
    for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) big = std::max(big, nrows_t[t]);
    for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols && nrows_t[t] >= 1 && nrows_t[t] <= 8 && big >= 16) small_left = true;
    if (!small_left) return;
    m->prog = saved;
  }
  canonicalize_once(m, columns, nrows, nrows_t, true);
}
void canonicalize_once(rh_model *m, const double *const *columns, const int64_t *nrows, std::vector<int64_t> &nrows_t, bool allow_unroll,
                       bool *unroll_blocked) {
  std::string err;
  nrows_t.assign(m->prog.targets.size(), 0);
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) nrows_t[t] = nrows[t];
  std::vector<uint32_t> kept;
  for (uint32_t c = 0; c < m->prog.n_cols_total; c++) {
    if (!columns[c]) throw Fail{RH_E_INVALID, "a column pointer is NULL"};
    kept.push_back(c);
  }
  bool canon = m->prog.n_cols_total > 0, changed = false;
  if (const char *e = rh::knob("RH_CANON_COLUMNS")) canon = canon && std::atoi(e) != 0;
  // gather mode (a Lookup over a long run of trailing parameters indexed by a column: emit.cpp) keeps its targets as they are
  bool gather = false;
  {
    uint32_t first_table_param = m->prog.n_params;
    int gmin = m->eopt.gather_min;
    if (const char *e = rh::knob("RH_GATHER_MIN")) gmin = std::max(1, std::atoi(e));
    const rh::Program &P = m->prog;
    for (const rh::Node &nd : P.nodes) {
      if (nd.op != RH_RIR_LOOKUP || (int)nd.table.size() < gmin) continue;
      const rh::Node &ix = P.nodes[nd.a], &t0 = P.nodes[nd.table[0]];
      if (ix.op == RH_RIR_INPUT && ix.input >= P.n_params && t0.op == RH_RIR_INPUT && t0.input < P.n_params &&
          t0.input + nd.table.size() == P.n_params) { gather = true; first_table_param = std::min(first_table_param, t0.input); }
    }
    // ... unless gather mode cannot apply anyway: a data-free target already has a gradient with respect to a table parameter
    // (the table's prior, in any model that comes from the reference's front end) and the emitter will take the generic path
    for (const rh::Target &T : P.targets) {
      if (T.n_cols) continue;
      for (uint32_t q = first_table_param; q < P.n_params && gather; q++) {
        const rh::Node &g = P.nodes[T.outputs[1 + q]];
        if (!(g.op == RH_RIR_CONST && g.cval == 0.0)) gather = false;
      }
    }
  }
  if (unroll_blocked) *unroll_blocked = gather;
  if (canon) changed = rh::canonicalize_columns(m->prog, columns, nrows_t.data(), m->eopt.fp_contract, kept, err, allow_unroll && !gather);
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (!m->prog.targets[t].n_cols) nrows_t[t] = 0;   // an unrolled initial chunk
  bool re = changed && m->eopt.fp_contract && m->eopt.simplify;
  if (const char *e = rh::knob("RH_REFACTOR")) re = re && std::atoi(e) != 0;
  m->col_src.clear(); m->col_len.clear();
  {
    size_t g = 0;
    for (size_t t = 0; t < m->prog.targets.size(); t++)
      for (uint32_t j = 0; j < m->prog.targets[t].n_cols; j++, g++) { m->col_src.push_back({kept[g]}); m->col_len.push_back({nrows_t[t]}); }
  }
  std::vector<int> owner;  // column (before rolling) -> its target
  for (size_t t = 0; t < m->prog.targets.size(); t++) for (uint32_t j = 0; j < m->prog.targets[t].n_cols; j++) owner.push_back((int)t);
  std::vector<std::vector<uint32_t>> parts;
  if (re) {
    // fast builds: gradient re-derivation, re-association, and Model.observe's 8-way split rolled back into rows
    rh::Program Q = rh::simplify(m->prog, true);
    bool rederive = true;
    if (const char *e = rh::knob("RH_REDERIVE")) rederive = std::atoi(e) != 0;
    if (rederive) {  // the gradient in its natural form, from the value output (verified against the supplied one): rederive.cpp
      std::vector<const double *> cp;
      for (uint32_t c : kept) cp.push_back(columns[c]);
      Q = rh::simplify(rh::rederive_gradients(Q, cp, nrows_t.data()), true);
    }
    m->prog = rh::simplify(rh::refactor(Q, &parts), true);
  } else {
    // strict builds: the 8 slots rolled back without re-association (rollstrict.cpp), if the program is the reference's lowering
    bool rs = changed && !m->eopt.fp_contract && m->eopt.simplify;
    if (const char *e = rh::knob("RH_ROLL_STRICT")) rs = rs && std::atoi(e) != 0;
    if (!rs) return;
    rh::Program Q = rh::simplify(m->prog, false);
    if (!rh::roll_strict(Q, parts)) return;
    m->prog = rh::simplify(Q, false);
  }
  // the row counts and the caller-side blocks of every column follow
  std::vector<std::vector<uint32_t>> src;
  std::vector<std::vector<int64_t>> len;
  std::vector<int64_t> nr(m->prog.targets.size(), 0);
  for (size_t t = 0; t < m->prog.targets.size(); t++) {
    const auto &T = m->prog.targets[t];
    for (uint32_t j = 0; j < T.n_cols; j++) {
      std::vector<uint32_t> cs;
      std::vector<int64_t> ls;
      int64_t rows = 0;
      const auto &pj = parts[T.col0 + j];
      for (size_t b = 0; b < pj.size(); b++) {
        const uint32_t g = pj[b];
        if (g == 0xFFFFFFFFu) {   // zeros, as long as block b of the target's first column
          if (j == 0 || b >= len[T.col0].size()) throw Fail{RH_E_INVALID, "internal: zero block without a reference column"};
          cs.push_back(g); ls.push_back(len[T.col0][b]);
        } else { cs.push_back(kept[g]); ls.push_back(nrows_t[(size_t)owner[g]]); }
        rows += ls.back();
      }
      if (j == 0) nr[t] = rows;
      else if (rows != nr[t]) throw Fail{RH_E_INVALID, "internal: rolled columns of one target disagree on the row count"};
      src.push_back(cs); len.push_back(ls);
    }
  }
  m->col_src = src; m->col_len = len;
  nrows_t = nr;
}

// ---- create-time self-checks (see selfcheck_engine) ----------------------------------------------------------------------------
bool selfcheck_enabled() {
  const char *e = rh::unsafe_knob("RH_SELFCHECK");
  return !(e && std::atoi(e) == 0);
}
// |a - b| within summation-order noise of each other, judged against the size of the whole output vector (gradients cancel)
bool outputs_agree(const double *lp, const double *g, const double *lp_ref, const double *g_ref, int n, std::string &what) {
  double scale = 0.0;
  for (int i = -1; i < n; i++) {
    const double a = i < 0 ? *lp : g[i], b = i < 0 ? *lp_ref : g_ref[i];
    if (std::isfinite(a)) scale = std::max(scale, std::fabs(a));
    if (std::isfinite(b)) scale = std::max(scale, std::fabs(b));
  }
  for (int i = -1; i < n; i++) {
    const double a = i < 0 ? *lp : g[i], b = i < 0 ? *lp_ref : g_ref[i];
    if (!std::isfinite(a) && !std::isfinite(b)) continue;
    if (std::isfinite(a) && std::isfinite(b) && std::fabs(a - b) <= 1e-7 * (std::fabs(a) + std::fabs(b)) + 1e-9 * scale + 1e-300) continue;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: %.17g vs %.17g", i < 0 ? "logp" : ("gradient " + std::to_string(i)).c_str(), a, b);
    what = buf;
    return false;
  }
  return true;
}
// rh_density_kernel against the tick engine's gradient path (gradient kernel + rh_density_fin_kernel) at three points, when a
// model has both.  They are different kernels around the same row code; a disagreement beyond summation-order noise means one of
// them is wrong on this device, and nothing says which: creation fails.  Round 5: the comparison is repeated on PREFIXES of the data
// -- 63, 6 and 1 rows per row target: the ragged-tile shapes, where row code runs under a partial mask or behind a select (the shape
// of round 3's fault) -- and a data set too large for one wavefront per chain (cfg 4: 1e7 rows) is checked on a prefix of 2^20 + 37
// rows instead of being skipped.  A prefix is taken by handing the kernels a smaller row count; the columns are not touched.
void selfcheck_density(rh_model *m) {
  if (!selfcheck_enabled() || !m->density_ok || !m->tick_ok || m->info.gather_mode) return;
  const int nc = 3, n = (int)m->prog.n_params;
  std::vector<double> q((size_t)nc * n), la(nc), lb(nc), ga((size_t)nc * n), gb((size_t)nc * n);
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (double &v : q) { x = x * 6364136223846793005ULL + 1442695040888963407ULL; v = ((double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5) * 1.2; }
  const rh_model_data full = m->data;
  const int64_t rows_full = m->rows_total;
  struct Restore { rh_model *m; rh_model_data d; int64_t r; ~Restore() { m->data = d; m->rows_total = r; } } restore{m, full, rows_full};
  int64_t longest = 0;
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) longest = std::max<int64_t>(longest, full.nrows[t]);
  const int64_t big = ((int64_t)1 << 20) + 37;
  for (const int64_t clip : {(int64_t)0, (int64_t)63, (int64_t)6, (int64_t)1}) {
    const int64_t lim = clip == 0 ? (m->rows_total > ((int64_t)1 << 22) ? big : longest) : clip;
    if (clip != 0 && lim >= longest) continue;   // (the whole data set is that small already: checked by the first pass)
    m->data = full;
    m->rows_total = 0;
    for (size_t t = 0; t < m->prog.targets.size(); t++) {
      if (!m->prog.targets[t].n_cols) continue;
      m->data.nrows[t] = std::min<long long>(full.nrows[t], lim);
      m->rows_total += m->data.nrows[t];
    }
    int rc = rh_density_eval_ex(m, q.data(), nc, RH_ENGINE_CHAIN, 0, la.data(), ga.data());
    if (rc == RH_E_LOOKUP) return;   // the data hold an index outside a Lookup table: every later call reports it
    if (rc == RH_OK) rc = rh_density_eval_ex(m, q.data(), nc, RH_ENGINE_TICK, 0, lb.data(), gb.data());
    if (rc != RH_OK) throw Fail{rc, "create-time self-check: " + m->err};
    for (int c = 0; c < nc; c++) {
      std::string what;
      if (!outputs_agree(&la[c], &ga[(size_t)c * n], &lb[c], &gb[(size_t)c * n], n, what))
        throw Fail{RH_E_DEVICE, "create-time self-check (" + (clip ? "first " + std::to_string(lim) + " rows" : std::string("all rows")) +
                                 "): rh_density_kernel and the tick engine's gradient path disagree at a test point (" + what +
                                 "): one of the two is wrong on this device"};
    }
  }
}

}  // namespace

namespace {
// the constants the data-free targets read instead of spelling them (EmitInfo::kpool) -> device
void upload_kpool(rh_model *m) {
  if (m->d_kpool) { (void)hipFree(m->d_kpool); m->d_kpool = nullptr; }
  const std::vector<double> &k = m->info.kpool;
  HIPCHK(hipMalloc(&m->d_kpool, std::max<size_t>(1, k.size()) * sizeof(double)));
  if (!k.empty()) HIPCHK(hipMemcpy(m->d_kpool, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
  m->data.kpool = (const double *)m->d_kpool;
}
}  // namespace

// ---- seam 1 -----------------------------------------------------------------------------------------
extern "C" int rh_model_create(const void *rir, size_t rir_len, const double *const *columns_in, const int64_t *nrows,
                               const rh_compile_opts *opts, rh_model **out) {
  if (!out) { g_err = "rh_model_create: out is NULL"; return RH_E_INVALID; }
  *out = nullptr;
  rh_model *m = new rh_model();
  const int rc = guard(m, [&] {
    std::vector<int64_t> nrows_in;
    std::vector<const double *> colv;
    const int dev0 = apply_compile_opts(m, opts);   // first: the loader's rewrites depend on the math mode
    load_program(m, rir, rir_len, columns_in, nrows, colv, nrows_in);
    if (m->prog.n_cols_total > m->synth_cols.size() && !columns_in) throw Fail{RH_E_INVALID, "columns is NULL but the model has data columns"};
    const double *const *columns = colv.data();
    int dev = dev0;
    for (size_t t = 0; t < m->prog.targets.size(); t++)
      if (m->prog.targets[t].n_cols && nrows_in[t] < 0) throw Fail{RH_E_INVALID, "negative or missing row count"};
    std::vector<int64_t> nrows_t;
    canonicalize(m, columns, nrows_in.data(), nrows_t);
    assemble_source(m);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      throw Fail{RH_E_DEVICE, "no HIP device available: the engine has no CPU fallback (use rh_lower_only to cross-compile)"};
    }
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    if (dev >= ndev) throw Fail{RH_E_INVALID, "device ordinal out of range"};
    m->device = dev;
    m->arch = device_arch(dev);
    build_code(m);
    load_module(m);
    upload_kpool(m);
    if (m->want_nuts) (void)load_variant(m, 1);
    // observation columns -> HBM (the engine copies; the caller keeps ownership).  In gather mode the rows of a gather
    // target are first brought into index order (stable counting sort; only the summation order of the rows changes):
    // group g = rows whose table index is low + g.  Row targets without a gather are cut into pseudo-groups of 4096 rows.
    for (size_t t = 0; t < m->prog.targets.size(); t++) {
      const auto &T = m->prog.targets[t];
      m->data.nrows[t] = T.n_cols ? nrows_t[t] : 0;
      m->rows_uploaded.push_back(m->data.nrows[t]);
      if (!T.n_cols) continue;
      m->rows_total += nrows_t[t];
      const int64_t nr = nrows_t[t];
      std::vector<double> joined;
      auto column = [&](uint32_t ec) -> const double * {   // engine column ec on the host: the caller's array, or its parts joined
        const auto &cs = m->col_src[ec];
        if (cs.size() == 1) return columns[cs[0]];
        joined.clear();
        for (size_t b = 0; b < cs.size(); b++) {
          const int64_t L = m->col_len[ec][b];
          if (cs[b] == 0xFFFFFFFFu) joined.insert(joined.end(), (size_t)L, 0.0);
          else joined.insert(joined.end(), columns[cs[b]], columns[cs[b]] + L);
        }
        if ((int64_t)joined.size() != nr) throw Fail{RH_E_INVALID, "internal: joined column length"};
        return joined.data();
      };
      std::vector<int64_t> perm;  // empty = identity
      if (m->info.gather_mode) {
        const auto &ti = m->info.targets[t];
        if (nr >= (int64_t)1 << 31) throw Fail{RH_E_UNSUPPORTED, "gather mode: more than 2^31 rows in one target"};
        std::vector<int> off;
        if (ti.has_gather) {
          std::vector<double> idx_store;
          const double *idx = column(T.col0 + ti.g_col);
          if (idx == joined.data()) { idx_store = joined; idx = idx_store.data(); }
          off.assign((size_t)ti.g_count + 1, 0);
          bool sorted = true;
          int64_t prev = 0;
          std::vector<int> key((size_t)nr);
          for (int64_t r = 0; r < nr; r++) {
            const double v = idx[r];
            const int64_t k = (int64_t)v - ti.g_low;   // D2I truncation like the Lookup it replaces
            if (!(v == v) || k < 0 || k >= ti.g_count) throw Fail{RH_E_LOOKUP, "Lookup index out of range in the data (row " + std::to_string(r) + ")"};
            if (k < prev) sorted = false;
            prev = k;
            key[(size_t)r] = (int)k;
            off[(size_t)k + 1]++;
          }
          for (int g = 0; g < ti.g_count; g++) off[(size_t)g + 1] += off[(size_t)g];
          if (!sorted) {
            perm.resize((size_t)nr);
            std::vector<int> next(off.begin(), off.end() - 1);
            for (int64_t r = 0; r < nr; r++) perm[(size_t)next[(size_t)key[(size_t)r]]++] = r;
          }
        } else {
          for (int64_t r = 0; r < nr; r += 4096) off.push_back((int)r);
          off.push_back((int)nr);
          if (off.size() == 1) off.push_back(0);
        }
        void *dp = nullptr;
        HIPCHK(hipMalloc(&dp, off.size() * sizeof(int)));
        m->goff_dev.push_back(dp);
        HIPCHK(hipMemcpy(dp, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
        m->goff_host.push_back(std::move(off));
        m->gather_count.push_back(ti.has_gather ? ti.g_count : 0);
      }
      std::vector<double> tmp;
      for (uint32_t j = 0; j < T.n_cols; j++) {
        void *d = nullptr;
        const size_t bytes = (size_t)nr * sizeof(double);
        HIPCHK(hipMalloc(&d, bytes ? bytes : 8));
        m->dev_cols.push_back(d);
        const double *src = column(T.col0 + j);
        if (!perm.empty()) {
          tmp.resize((size_t)nr);
          for (int64_t r = 0; r < nr; r++) tmp[(size_t)r] = src[perm[(size_t)r]];
          src = tmp.data();
        }
        if (bytes) HIPCHK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      }
    }
    // the pointer table itself (dev_cols is in flattened column order: targets ascending, then column)
    HIPCHK(hipMalloc(&m->d_coltab, std::max<size_t>(1, m->dev_cols.size()) * sizeof(void *)));
    if (!m->dev_cols.empty()) HIPCHK(hipMemcpy(m->d_coltab, m->dev_cols.data(), m->dev_cols.size() * sizeof(void *), hipMemcpyHostToDevice));
    m->data.cols = (const double *const *)m->d_coltab;
  });
  int rc2 = rc;
  if (rc2 == RH_OK) rc2 = guard(m, [&] { selfcheck_density(m); });
  if (rc2 != RH_OK) { const std::string keep = m->err; rh_model_destroy(m); g_err = keep; return rc2; }
  *out = m;
  return RH_OK;
}

// The same model on another device: everything rh_model_create derived on the host is copied, the code object is loaded as it
// is, the columns travel device to device.
extern "C" int rh_model_clone(const rh_model *src, int32_t device, rh_model **out) {
  if (!out) { g_err = "rh_model_clone: out is NULL"; return RH_E_INVALID; }
  *out = nullptr;
  if (!src || !src->loaded) { g_err = "rh_model_clone: model not loaded"; return RH_E_INVALID; }
  rh_model *m = new rh_model();
  const int rc = guard(m, [&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Fail{RH_E_DEVICE, "no HIP device available"};
    int dev = device;
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    if (dev >= ndev) throw Fail{RH_E_INVALID, "device ordinal out of range"};
    m->prog = src->prog; m->eopt = src->eopt; m->info = src->info; m->want_nuts = src->want_nuts;
    m->source = src->source; m->nacc_max = src->nacc_max; m->grad_k = src->grad_k; m->has_glm = src->has_glm;
    m->glm_small = src->glm_small; m->glm_w = src->glm_w; m->lk_lds = src->lk_lds; m->gather_waves = src->gather_waves;
    m->goff_host = src->goff_host; m->gather_count = src->gather_count; m->col_len = src->col_len; m->col_src = src->col_src;
    m->rows_total = src->rows_total; m->data = src->data; m->data.cols = nullptr; m->rows_uploaded = src->rows_uploaded;
    // ... and the state of the lowering itself: build_code / build_variant_code decide from it which kernels the model needs and
    // how the shape may still be lightened (a clone whose n_row_targets_hint stayed 0 accepted a variant with an unfit tick kernel)
    m->n_row_targets_hint = src->n_row_targets_hint; m->rows_unroll_auto = src->rows_unroll_auto; m->unroll_auto = src->unroll_auto;
    m->shape_guessed = src->shape_guessed; m->synth_cols = src->synth_cols; m->ncols_max = src->ncols_max; m->glm_ncols = src->glm_ncols;
    m->device = dev;
    m->arch = device_arch(dev);
    m->grad_chains_req = src->grad_chains_req;
    if (m->arch == src->arch) { m->code = src->code; m->lane_code = src->lane_code; m->lane_r = src->lane_r; m->lane_tried = src->lane_tried;
      m->lane_rows_code = src->lane_rows_code; m->lane_rows_why = src->lane_rows_why; m->lane_rows_tried = src->lane_rows_tried; }   // (its interleaved copies: ensure_lane_rows, on its device)
    else build_code(m);   // (a mixed node: compiled or fetched from the cache for that architecture)
    load_module(m);
    if (m->want_nuts) (void)load_variant(m, 1);
    // observation columns and group offsets: device to device (src's copies are immutable after rh_model_create)
    size_t c = 0;
    for (size_t t = 0; t < m->prog.targets.size(); t++) {
      const auto &T = m->prog.targets[t];
      for (uint32_t j = 0; j < T.n_cols; j++, c++) {
        const size_t bytes = (size_t)m->data.nrows[t] * sizeof(double);
        void *d = nullptr;
        HIPCHK(hipMalloc(&d, bytes ? bytes : 8));
        m->dev_cols.push_back(d);
        if (bytes) HIPCHK(hipMemcpyPeer(d, dev, src->dev_cols[c], src->device, bytes));
      }
    }
    for (size_t rt = 0; rt < src->goff_dev.size(); rt++) {
      const size_t bytes = m->goff_host[rt].size() * sizeof(int);
      void *dp = nullptr;
      HIPCHK(hipMalloc(&dp, bytes));
      m->goff_dev.push_back(dp);
      HIPCHK(hipMemcpy(dp, m->goff_host[rt].data(), bytes, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&m->d_coltab, std::max<size_t>(1, m->dev_cols.size()) * sizeof(void *)));
    if (!m->dev_cols.empty()) HIPCHK(hipMemcpy(m->d_coltab, m->dev_cols.data(), m->dev_cols.size() * sizeof(void *), hipMemcpyHostToDevice));
    m->data.cols = (const double *const *)m->d_coltab;
    m->d_kpool = nullptr; upload_kpool(m);
  });
  if (rc != RH_OK) { rh_model_destroy(m); return rc; }
  *out = m;
  return RH_OK;
}

extern "C" void rh_model_destroy(rh_model *m) {
  if (!m) return;
  if (m->module || !m->dev_cols.empty()) {  // also after a failure half-way through load_module
    hipSetDevice(m->device);
    for (void *d : m->dev_cols) hipFree(d);
    if (m->d_coltab) hipFree(m->d_coltab);
    if (m->d_kpool) hipFree(m->d_kpool);
    for (void *d : m->goff_dev) hipFree(d);
    if (m->stream) hipStreamDestroy(m->stream);
    for (int v = 1; v < 8; v++)  // [0] aliases the base module
      if (m->variants[v].module && m->variants[v].module != m->module) hipModuleUnload(m->variants[v].module);
    for (void *d : m->dev_rows) if (d) hipFree(d);
    if (m->lane_rows_module) hipModuleUnload(m->lane_rows_module);
    if (m->lane_module) hipModuleUnload(m->lane_module);
    if (m->module) hipModuleUnload(m->module);
  }
  delete m;
}
extern "C" int rh_model_nvars(const rh_model *m) { return m ? (int)m->prog.n_params : -RH_E_INVALID; }
extern "C" const char *rh_model_hip_source(const rh_model *m) { return m ? m->source.c_str() : ""; }
extern "C" int rh_optimize(rh_model *m, const double *x0, int32_t starts, int32_t max_evals, double *x_out,
                           int32_t *evals_out, int32_t *status_out) {
  if (!m || !m->loaded) { g_err = "rh_optimize: model not loaded"; return RH_E_INVALID; }
  if (!x_out || starts <= 0) { m->err = g_err = "rh_optimize: bad arguments"; return RH_E_INVALID; }
  std::string err;
  int rc = rh::lbfgs_multistart((int)m->prog.n_params, starts, x0, max_evals,
                                [m](const double *q, int k, double *lp, double *gr) { return rh_density_eval(m, q, k, lp, gr); },
                                x_out, evals_out, status_out, err);
  (void)err; // rh_density_eval has already recorded the failure in m->err
  return rc;
}

extern "C" int rh_model_engines(const rh_model *m, int32_t *chain_engine, int32_t *tick_engine, int32_t *density, int32_t *compile_attempts,
                                char *why, size_t why_cap) {
  if (!m || !m->loaded) { g_err = "rh_model_engines: model not loaded"; return RH_E_INVALID; }
  // (the base sampler-kernel variant; a NUTS / dense-mass variant is inspected when a sampler first asks for it)
  if (chain_engine) *chain_engine = m->chain_ok ? 1 : 0;
  if (tick_engine) *tick_engine = m->tick_ok ? 1 : 0;
  if (density) *density = (m->density_ok || m->tick_ok) ? 1 : 0;
  if (compile_attempts) *compile_attempts = m->compile_attempts;
  if (why && why_cap) {
    std::string w;
    if (!m->chain_ok) w += "chain engine: " + m->chain_why + "\n";
    if (!m->tick_ok) w += "tick engine: " + m->tick_why + "\n";
    if (!m->density_ok) w += "rh_density_kernel: " + m->density_why + "\n";
    std::snprintf(why, why_cap, "%s", w.c_str());
  }
  return RH_OK;
}
extern "C" int64_t rh_compile_count(void) { return (int64_t)g_compiles.load(); }
extern "C" const char *rh_last_error(const rh_model *m) { return m ? m->err.c_str() : g_err.c_str(); }
extern "C" int rh_abi_version(void) { return RH_ABI_VERSION; }
extern "C" int rh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Lower + cross-compile only (no device needed): used by build()/CPU tests.  Returns the generated source
// through *src_out (malloc'ed, caller frees with rh_free) and the code-object size.
// rh_lower_only_data: the same with the observation columns in hand, i.e. exactly the lowering rh_model_create performs
// (column canonicalisation and what follows from it included); columns == NULL skips the data-dependent passes.
namespace {
// one line per kernel of a code object: registers, spills, scratch, and whether the engine would launch it
std::string code_report(const std::vector<char> &code, const std::string &tag) {
  std::vector<std::string> names;
  std::string r;
  if (!rh::list_kernels(code, names)) return tag + " unreadable\n";
  for (const std::string &k : names) {
    rh::KernelMeta km;
    rh::kernel_meta(code, k, km);
    std::string why;
    const int h = kernel_health(code, k, &why);
    int unproven = 0;
    { std::vector<std::string> f; (void)rh::check_code_object(code, k, f, &unproven); }
    r += tag + " kernel=" + k + " unproven=" + std::to_string(unproven) + " vgprs=" + std::to_string(km.vgprs) + " sgprs=" + std::to_string(km.sgprs) + " vgpr_spills=" + std::to_string(km.vgpr_spills) +
         " sgpr_spills=" + std::to_string(km.sgpr_spills) + " scratch=" + std::to_string(km.scratch_bytes) + " fit=" + (h == KH_OK ? "1" : "0") +
         (h == KH_OK ? std::string() : " why=" + why) + "\n";
  }
  return r;
}
}  // namespace
// Test hooks (no device needed): the report of one code object in memory, and the decoder's instruction offsets of one kernel
extern "C" int rh_code_object_report(const void *code, size_t len, char **report) {
  if (!code || !report) return RH_E_INVALID;
  const std::vector<char> c((const char *)code, (const char *)code + len);
  const std::string r = code_report(c, "object");
  *report = (char *)std::malloc(r.size() + 1); std::memcpy(*report, r.c_str(), r.size() + 1);
  return RH_OK;
}
extern "C" int rh_code_object_offsets(const void *code, size_t len, const char *kernel, uint32_t **offs, size_t *n) {
  if (!code || !kernel || !offs || !n) return RH_E_INVALID;
  const std::vector<char> c((const char *)code, (const char *)code + len);
  std::vector<uint32_t> o;
  if (!rh::kernel_instruction_offsets(c, kernel, o)) return RH_E_INVALID;
  *offs = (uint32_t *)std::malloc(sizeof(uint32_t) * std::max<size_t>(1, o.size()));
  std::memcpy(*offs, o.data(), sizeof(uint32_t) * o.size());
  *n = o.size();
  return RH_OK;
}
extern "C" int rh_lower_report_data(const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows,
                                    const rh_compile_opts *opts, const char *arch, char **src_out, size_t *code_size, char **report);
extern "C" int rh_lower_only_data(const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows,
                                  const rh_compile_opts *opts, const char *arch, char **src_out, size_t *code_size) {
  return rh_lower_report_data(rir, rir_len, columns, nrows, opts, arch, src_out, code_size, nullptr);
}
extern "C" int rh_lower_report_data(const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows,
                                    const rh_compile_opts *opts, const char *arch, char **src_out, size_t *code_size, char **report) {
  rh_model m;
  const int rc = guard(nullptr, [&] {
    std::vector<int64_t> nrows_in;
    std::vector<const double *> colv;
    (void)apply_compile_opts(&m, opts);
    load_program(&m, rir, rir_len, columns, nrows, colv, nrows_in);
    bool all_cols = true;   // the data-dependent passes need every column (the caller's and the lifted ones) on the host
    for (const double *c : colv) all_cols = all_cols && c != nullptr;
    if (all_cols && ((columns && nrows) || !m.synth_cols.empty())) { std::vector<int64_t> nrows_t; canonicalize(&m, colv.data(), nrows_in.data(), nrows_t); }
    assemble_source(&m);
    m.arch = arch && *arch ? arch : "gfx950";
    if (code_size) {          // (nullptr: source only -- the CPU suite's host emulation of the generated code)
      build_code(&m);         // may lower again with a smaller row-loop unroll: the source returned is the one that was compiled
      build_lane_code(&m);
      build_lane_rows_code(&m);
      *code_size = m.code.size();
    }
    if (src_out) {
      // (test hook: the constant pool's VALUES travel behind the source as a trailing comment, for the CPU tier's host emulation of the
      //  generated code -- they are not part of the translation unit rh_model_create compiles and hashes)
      std::string text = m.source;
      if (!m.info.kpool.empty()) {
        text += "\n// rh_kpool " + std::to_string(m.info.kpool.size()) + ":";
        char buf[40];
        for (double v : m.info.kpool) { std::snprintf(buf, sizeof buf, " %a", v); text += buf; }
        text += "\n";
      }
      *src_out = (char *)std::malloc(text.size() + 1); std::memcpy(*src_out, text.c_str(), text.size() + 1);
    }
    if (!code_size) return;
    std::vector<char> vcode;
    if (opts && opts->with_nuts) vcode = build_variant_code(&m, opts->with_nuts & 7);
    if (report) {   // what the engine would launch of it: the shape it settled on and every kernel's fitness (kernel_health)
      std::string r = "attempts=" + std::to_string(m.compile_attempts) + " rows_unroll=" + std::to_string(m.eopt.rows_unroll) +
                      " grad_unroll=" + std::to_string(m.eopt.grad_unroll) + " grad_k=" + std::to_string(m.info.grad_k) +
                      " chain_waves=" + std::to_string(m.eopt.chain_waves) + " grad_pipeline=" + std::to_string(m.eopt.grad_pipeline) +
                      " chunk=" + std::to_string(m.eopt.chunk) + " bigu=" + std::to_string(m.eopt.big_unroll) + " gather=" + std::to_string((int)m.info.gather_mode) + " row_targets=" + std::to_string(m.n_row_targets_hint) + "\n";
      r += code_report(m.code, "base");
      if (!vcode.empty()) r += code_report(vcode, "variant" + std::to_string(opts->with_nuts & 7));
      if (!m.lane_code.empty()) {   // (of the lane walk's code object only the kernel the engine takes from it, which is fit: with
        // the rows per scalar request it was built for and its static LDS)
        rh::KernelMeta km;
        rh::kernel_meta(m.lane_code, "rh_grad_lane_kernel", km);
        std::istringstream all(code_report(m.lane_code, "lane"));
        for (std::string ln; std::getline(all, ln);)
          if (ln.find("rh_grad_lane_kernel") != std::string::npos) r += ln + " lane_r=" + std::to_string(m.lane_r) + " lds=" + std::to_string(km.lds_bytes) + "\n";
      }
      if (!m.lane_rows_code.empty()) {   // (the row feed's code object likewise, under a tag of its own)
        rh::KernelMeta km;
        rh::kernel_meta(m.lane_rows_code, "rh_grad_lane_kernel", km);
        std::istringstream all(code_report(m.lane_rows_code, "lane_rows"));
        for (std::string ln; std::getline(all, ln);)
          if (ln.find("rh_grad_lane_kernel") != std::string::npos) r += ln + " lane_r=" + std::to_string(m.lane_r) + " lds=" + std::to_string(km.lds_bytes) + "\n";
      } else if (!m.lane_rows_why.empty()) {   // eligible, built and dropped: the reason
        std::string why = m.lane_rows_why;
        std::replace(why.begin(), why.end(), '\n', ' ');
        r += "lane_rows kernel=rh_grad_lane_kernel unproven=0 vgprs=0 sgprs=0 vgpr_spills=0 sgpr_spills=0 scratch=0 fit=0 lane_r=" + std::to_string(m.lane_r) + " lds=0 why=" + why + "\n";
      }
      *report = (char *)std::malloc(r.size() + 1); std::memcpy(*report, r.c_str(), r.size() + 1);
    }
  });
  return rc;
}
extern "C" int rh_lower_only(const void *rir, size_t rir_len, const rh_compile_opts *opts, const char *arch,
                             char **src_out, size_t *code_size) {
  return rh_lower_only_data(rir, rir_len, nullptr, nullptr, opts, arch, src_out, code_size);
}
extern "C" void rh_free(void *p) { std::free(p); }
// Test hook (no device needed): the program after the emitter's clean-up pass, as RIR again, so that the CPU suite can
// check on the oracle's interpreter that simplify() is value-preserving.  fast != 0 adds the fast-mode-only rules.
extern "C" int rh_simplify_rir(const void *rir, size_t rir_len, int fast, void **out, size_t *out_len) {
  return guard(nullptr, [&] {
    rh::Program P; std::string err;
    if (!rh::parse_rir(rir, rir_len, P, err)) throw Fail{RH_E_INVALID, err};
    const std::vector<unsigned char> b = rh::write_rir(rh::simplify(P, fast != 0));
    *out = std::malloc(b.size()); std::memcpy(*out, b.data(), b.size()); *out_len = b.size();
  });
}

// Test hook (no device needed): the program after column canonicalisation (and, with refactor != 0, after everything else
// rh_model_create does to it in that math mode: re-derivation / re-association / slot rolling, or the strict rolling) as RIR again, so that the CPU suite can check on the oracle's interpreter that
// the rewrite preserves values.  parts_out receives, per column the rewritten program reads, a count followed by that many
// (caller column index | 0xFFFFFFFF = zeros, block length) pairs: the data concatenated into it, in order (*n_parts_words
// holds the capacity on entry); nrows_out the row
// count of every target.  Returns RH_OK also when nothing was rewritten.
extern "C" int rh_canonicalize_rir(const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows, int fast,
                                   int refactor, void **out, size_t *out_len, uint32_t *parts_out, uint32_t *n_parts_words,
                                   int64_t *nrows_out) {   // *n_parts_words: in = capacity of parts_out, out = words written
  rh_model m;
  return guard(nullptr, [&] {
    std::vector<int64_t> nrows_in, nr;
    std::vector<const double *> colv;
    m.eopt.fp_contract = fast != 0;
    load_program(&m, rir, rir_len, columns, nrows, colv, nrows_in);
    if (!m.synth_cols.empty()) throw Fail{RH_E_UNSUPPORTED, "rh_canonicalize_rir: the program lifts constants into columns of its own (use rh_lift_rir)"};
    m.eopt.simplify = refactor != 0;   // canonicalize() re-associates / rolls only when the clean-up pass is on
    canonicalize(&m, colv.data(), nrows_in.data(), nr);
    const std::vector<unsigned char> b = rh::write_rir(m.prog);
    *out = std::malloc(b.size()); std::memcpy(*out, b.data(), b.size()); *out_len = b.size();
    uint32_t w = 0;
    size_t need = 0;
    for (const auto &cs : m.col_src) need += 1 + 2 * cs.size();
    if (need > *n_parts_words) throw Fail{RH_E_INVALID, "rh_canonicalize_rir: parts_out is too small"};
    for (size_t c = 0; c < m.col_src.size(); c++) {
      parts_out[w++] = (uint32_t)m.col_src[c].size();
      for (size_t b = 0; b < m.col_src[c].size(); b++) { parts_out[w++] = m.col_src[c][b]; parts_out[w++] = (uint32_t)m.col_len[c][b]; }
    }
    *n_parts_words = w;
    for (size_t t = 0; t < nr.size(); t++) nrows_out[t] = nr[t];
  });
}

// Test hook (no device needed): what load_program makes of a program with more than RH_MAX_TARGETS targets -- same-shaped
// data-free targets lifted into one streamed target (lift.cpp), the other runs merged -- as RIR, plus the synthesised columns
// (column-major, malloc'ed: ncols x nrows doubles; the caller frees with rh_free); they follow the caller's columns in the
// rewritten program's column order.  nrows_in (per target of the program handed in) -> nrows_out (per target of the rewritten
// one, at most RH_MAX_TARGETS entries); both may be NULL.
extern "C" int rh_lift_rir(const void *rir, size_t rir_len, void **out, size_t *out_len, double **cols_out, uint32_t *ncols, uint32_t *nrows,
                           const int64_t *nrows_in_caller, int64_t *nrows_out, int fast) {
  rh_model m;
  return guard(nullptr, [&] {
    std::vector<int64_t> nrows_in;
    std::vector<const double *> colv;
    m.eopt.fp_contract = fast != 0;   // fast builds lift more (centred table priors)
    load_program(&m, rir, rir_len, nullptr, nrows_in_caller, colv, nrows_in, true);
    if (nrows_out) for (size_t t = 0; t < nrows_in.size(); t++) nrows_out[t] = nrows_in[t];
    const std::vector<unsigned char> b = rh::write_rir(m.prog);
    *out = std::malloc(b.size()); std::memcpy(*out, b.data(), b.size()); *out_len = b.size();
    *ncols = (uint32_t)m.synth_cols.size();
    *nrows = 0;                                       // several lifted groups: the longest; shorter columns are zero-padded
    for (const auto &sc : m.synth_cols) *nrows = std::max<uint32_t>(*nrows, (uint32_t)sc.size());
    *cols_out = (double *)std::calloc(std::max<size_t>(1, (size_t)*ncols * *nrows), sizeof(double));
    for (size_t c = 0; c < m.synth_cols.size(); c++) std::memcpy(*cols_out + c * *nrows, m.synth_cols[c].data(), sizeof(double) * m.synth_cols[c].size());
  });
}

namespace {
// per-use device buffers of gather mode: split -> group boundaries and the scatter sums
struct GatherBufs {
  rh_gather_data gd{};
  std::vector<void *> owned;
  bool any_big = false, any_small = false;   // row targets for rh_grad_gather_kernel (no gather, or groups of >= 64 rows) / for rh_grad_gather_scan_kernel
  void build(rh_model *m, int chains, int nsplit) {
    for (size_t rt = 0; rt < m->goff_host.size(); rt++) {
      const std::vector<int> &off = m->goff_host[rt];
      const int ng = (int)off.size() - 1;
      const int64_t nr = off.back();
      std::vector<int> gs((size_t)nsplit + 1, ng);
      gs[0] = 0;
      int g = 0;
      for (int sidx = 1; sidx < nsplit; sidx++) {  // balanced by rows, cut at group boundaries only
        const int64_t want = nr * sidx / nsplit;
        while (g < ng && off[(size_t)g] < want) g++;
        gs[(size_t)sidx] = g;
      }
      void *dg = nullptr;
      HIPCHK(hipMalloc(&dg, gs.size() * sizeof(int)));
      owned.push_back(dg);
      HIPCHK(hipMemcpy(dg, gs.data(), gs.size() * sizeof(int), hipMemcpyHostToDevice));
      gd.goff[rt] = (const int *)m->goff_dev[rt];
      gd.gsplit[rt] = (const int *)dg;
      int gmin = 0x7fffffff;   // smallest non-empty group (the gather kernel's two-accumulator walk needs >= 64 rows per group)
      for (int gi = 0; gi < ng; gi++) { const int sz = off[(size_t)gi + 1] - off[(size_t)gi]; if (sz > 0) gmin = std::min(gmin, sz); }
      gd.gmin[rt] = gmin;
      if (const char *e = rh::knob("RH_GATHER_SCAN")) if (std::atoi(e)) gd.gmin[rt] = 0;   // tests: the general (segmented scan) walk
      if (m->gather_count[rt] == 0 || gd.gmin[rt] >= 64) any_big = true; else any_small = true;   // (the kernels' own test)
      if (m->gather_count[rt] > 0) {
        void *sb = nullptr;
        const size_t bytes = sizeof(double) * (size_t)chains * m->gather_count[rt];
        HIPCHK(hipMalloc(&sb, bytes));
        owned.push_back(sb);
        HIPCHK(hipMemset(sb, 0, bytes));
        gd.sbuf[rt] = (double *)sb;
      }
    }
    // hipMemset on device memory is a fill KERNEL on the null stream and returns before it has run; the engine's own stream is
    // non-blocking, so nothing orders its first launch behind these fills but this
    HIPCHK(hipDeviceSynchronize());
  }
  ~GatherBufs() { for (void *p : owned) (void)hipFree(p); }
};

// tick engine: row splits per chain group -- ~4 wavefronts per SIMD (256 CUs x 4 SIMDs), a multiple of 8 so that the XCD
// mapping applies, and >= 2048 rows per split
int default_nsplit(const rh_model *m, int chains) {
  const int ngroups = (chains + m->grad_k - 1) / m->grad_k;
  int64_t max_rows = 1;
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) max_rows = std::max<int64_t>(max_rows, m->data.nrows[t]);
  // the generic kernel with the rolling row loop hides its loads inside the wavefront: 2 wavefronts per SIMD in ONE round
  // (2048) beat 4096 in 1.33 rounds of three (profiles/r3_a_cfg2/sweep.txt)
  int nsplit = (int)std::max<int64_t>(1, ((m->eopt.grad_pipeline == 2 ? 2048 : 4096) + ngroups - 1) / ngroups);
  // the gather kernel (three wavefronts per SIMD, its own two-tile pipeline): many short workgroups measured best on cfg 5 --
  // 8 / 16 / 24 splits of 256 chain groups: 3.41 / 3.11 / 2.92 ms per launch (profiles/r5_cfg5)
  // (call B, another box: 16 / 24 / 32 / 48 splits 3.00 / 2.78 / 2.71 / 2.67 ms -- four rounds of 3072 wavefronts)
  // (call C: 32 / 48 / 64 / 96 splits 2.68 / 2.67 / 2.61 / 2.60 ms; 64 is also the most partial sums the tick's combine reads in one pass)
  if (m->info.gather_mode) nsplit = (int)std::max<int64_t>(1, (16384 + ngroups - 1) / ngroups);
  if (const char *e = rh::knob("RH_GATHER_WG")) if (m->info.gather_mode) nsplit = (int)std::max<int64_t>(1, (std::atoi(e) + ngroups - 1) / ngroups);
  if (m->k_grad_glm) { const int ctiles = (chains + 15) / 16; nsplit = (int)std::max<int64_t>(1, (2048 + ctiles - 1) / ctiles); }
  nsplit = ((nsplit + 7) / 8) * 8;
  const int64_t cap = std::max<int64_t>(8, (max_rows / 2048) / 8 * 8);
  return (int)std::min<int64_t>(nsplit, cap);
}

// the lane walk: RH_GRAD_WALK=tile|lane (RH_DIAG) forces the walk; total_chains = the chains of the whole sampler, all shards
int64_t lane_max_rows(const rh_model *m) {
  int64_t max_rows = 1;
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) max_rows = std::max<int64_t>(max_rows, m->data.nrows[t]);
  return max_rows;
}
thread_local int g_total_chains = 0;   // set by rh_sample_multi's shard threads around rh_sample
thread_local int g_shard_walk = -1;    // ... with the walk rh_sample_multi chose for all of its shards (0 tile, 1 lane; -1: no shards)
bool walk_is_lane(rh_model *m, bool static_hmc, int total_chains) {
  if (g_shard_walk >= 0) return g_shard_walk == 1 && ensure_lane(m) != nullptr;
  int forced = 0;
  if (const char *e = rh::knob("RH_GRAD_WALK")) forced = std::strcmp(e, "tile") == 0 ? 1 : (std::strcmp(e, "lane") == 0 ? 2 : 0);
  if (!rh_plan::walk_is_lane(true, static_hmc, m->grad_chains_req, total_chains, lane_max_rows(m), forced)) return false;   // (no reason to build the kernel)
  return ensure_lane(m) != nullptr;
}
int lane_nsplit(const rh_model *m, int total_chains) {
  return rh_plan::lane_nsplit(total_chains, lane_max_rows(m));
}
// the feed of a lane walk's launches: RH_LANE_FEED=cols|rows (RH_DIAG) forces it; `rows` is the column feed where the model has no
// row-fed kernel.  The two feeds give a chain the same bits, so every shard decides for itself.  Decided where a sampler is created
// and where a density evaluation begins, not launch by launch: a copy holds the rows that were uploaded, and should data.nrows
// name more at that moment, the launches take the column feed.
bool feed_is_rows(rh_model *m) {
  int forced = 0;
  if (const char *e = rh::knob("RH_LANE_FEED")) forced = std::strcmp(e, "cols") == 0 ? 1 : (std::strcmp(e, "rows") == 0 ? 2 : 0);
  if (!rh_plan::feed_is_rows(true, forced)) return false;   // (no reason to build the kernel and the copies)
  if (!rh_plan::feed_is_rows(ensure_lane_rows(m) != nullptr, forced)) return false;
  std::vector<long long> want;
  for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) want.push_back(m->data.nrows[t]);
  return m->k_grad_lane_rows && rh_plan::lane_rows_cover((int)want.size(), want.data(), (int)m->dev_rows_n.size(), m->dev_rows_n.data(), m->dev_rows.data());
}

// one batched gradient launch of the tick engine: whichever row-streaming kernel the model was lowered to
// (rh_grad_gather_kernel [+ rh_grad_gather_scan_kernel] | rh_grad_glm_kernel | rh_grad_kernel), per-split partial sums -> d_partial.
// The grid covers every chain; with a list (d_list / d_nlive; nullptr = all `chains`) slot s of the launch is chain list[s] and the
// workgroups of the slots past the live count -- the last of the grid -- return at once.
// d_vflag: the chains' request flags (rh_tick_kernel: 2 = gradient only, the log-density of that evaluation is never read) or nullptr.
void launch_grad(rh_model *m, GatherBufs *gb, void *d_q, void *d_list, void *d_nlive, void *d_vflag, void *d_partial, void *d_graderr, void *d_running,
                 int chains, int nsplit, int xcd, hipStream_t stream = nullptr, bool lane_walk = false, bool lane_rows = false) {
  if (!stream) stream = m->stream;
  if (lane_walk) {   // rh_grad_lane_kernel: 64 C chains per group, W wavefronts per workgroup, rh_grad_kernel's arguments
    const int lgroups = (chains + rh_plan::kLaneGroup - 1) / rh_plan::kLaneGroup;
    if (lane_rows) {   // (the caller has asked feed_is_rows, which looks at the copies) the row-fed rh_grad_lane_kernel: the same, with the interleaved copies' addresses (struct rh_lane_rows) behind the model's data
      void *ra[] = {&m->data, m->dev_rows.data(), &d_q, &d_list, &d_nlive, &d_vflag, &d_partial, &d_graderr, &d_running, &chains, &nsplit, &xcd};
      launch(m->k_grad_lane_rows, (unsigned)(lgroups * nsplit), 64 * rh_plan::kLaneW, stream, ra);
      return;
    }
    void *la[] = {&m->data, &d_q, &d_list, &d_nlive, &d_vflag, &d_partial, &d_graderr, &d_running, &chains, &nsplit, &xcd};
    launch(m->k_grad_lane, (unsigned)(lgroups * nsplit), 64 * rh_plan::kLaneW, stream, la);
    return;
  }
  const int ngroups = (chains + m->grad_k - 1) / m->grad_k;
  if (m->info.gather_mode) {
    void *ga[] = {&m->data, &gb->gd, &d_q, &d_list, &d_nlive, &d_vflag, &d_partial, &d_graderr, &d_running, &chains, &nsplit};
    if (gb->any_big) launch(m->k_grad_gather, (unsigned)(ngroups * nsplit), 64, stream, ga);
    if (gb->any_small) launch(m->k_grad_gather_scan, (unsigned)(ngroups * nsplit), 64, stream, ga);   // (its own row targets: other partial-sum slots)
    return;
  }
  void *args[] = {&m->data, &d_q, &d_list, &d_nlive, &d_vflag, &d_partial, &d_graderr, &d_running, &chains, &nsplit, &xcd};
  if (m->k_grad_glm) {
    const int ctiles = (chains + 15) / 16;
    const unsigned blocks = (unsigned)(((ctiles + m->glm_w - 1) / m->glm_w) * nsplit);
    const unsigned tile = (unsigned)m->glm_ncols * 66u * (unsigned)sizeof(double);  // the kernel's NBUF rule: two tiles while they fit
    const unsigned lds = (2u * tile + (m->lk_lds ? 6176u : 0u) <= 160u * 1024u ? 2u : 1u) * tile;
    HIPCHK(hipModuleLaunchKernel(m->k_grad_glm, blocks, 1, 1, 64u * m->glm_w, 1, 1, lds, stream, args, nullptr));
  } else
    launch(m->k_grad, (unsigned)(ngroups * nsplit), 64, stream, args);
}
}  // namespace

// ---- seam 2 -----------------------------------------------------------------------------------------
extern "C" int rh_density_eval(rh_model *m, const double *q, int32_t chains, double *logp, double *grad) {
  return rh_density_eval_ex(m, q, chains, RH_ENGINE_AUTO, 0, logp, grad);
}

extern "C" int rh_density_eval_ex(rh_model *m, const double *q, int32_t chains, int32_t engine, int32_t grad_splits,
                                  double *logp, double *grad) {
  if (!m || !m->loaded) { g_err = "rh_density_eval: model not loaded"; return RH_E_INVALID; }
  if (!q || !logp || !grad || chains <= 0) { m->err = g_err = "rh_density_eval: bad arguments"; return RH_E_INVALID; }
  if (engine < RH_ENGINE_AUTO || engine > RH_ENGINE_TICK || grad_splits < 0 || grad_splits > 65536) { m->err = g_err = "rh_density_eval_ex: unknown engine / bad grad_splits"; return RH_E_INVALID; }
  if (engine == RH_ENGINE_TICK && m->n_row_targets == 0) { m->err = g_err = "the tick engine needs a model that streams rows"; return RH_E_INVALID; }
  if (engine == RH_ENGINE_CHAIN && m->info.gather_mode) { m->err = g_err = "gather-mode models run on the tick engine only"; return RH_E_UNSUPPORTED; }
  // AUTO: rh_density_kernel (one chain per wavefront) unless it is not fit to run (kernel_health) -- then the tick engine's path
  const bool use_tick = m->info.gather_mode || engine == RH_ENGINE_TICK || (engine == RH_ENGINE_AUTO && !m->density_ok && m->tick_ok);
  if (use_tick && !m->tick_ok) { m->err = g_err = "the tick engine's kernels of this model are not fit to run: " + m->tick_why; return RH_E_UNSUPPORTED; }
  if (!use_tick && !m->density_ok) { m->err = g_err = "rh_density_kernel of this model is not fit to run: " + m->density_why; return RH_E_UNSUPPORTED; }
  std::lock_guard<std::mutex> lk(m->mu);
  int lookup_err = 0;
  const int rc = guard(m, [&] {
    HIPCHK(hipSetDevice(m->device));
    const int n = (int)m->prog.n_params;
    DevBuf bq(sizeof(double) * n * chains), bl(sizeof(double) * chains), bg(sizeof(double) * n * chains), be(sizeof(int));
    // generic models beyond 512 parameters accumulate their n + 1 outputs in memory (RH_BIGTH): one scratch row per chain
    const bool bigth = m->info.bign && !m->info.gather_mode && (n > 512 || m->eopt.chunk > 0);
    DevBuf btot(bigth ? sizeof(double) * (size_t)(n + 1) * chains : 8);
    void *dq = bq.p, *dl = bl.p, *dg = bg.p, *de = be.p, *dtot = btot.p;
    HIPCHK(hipMemcpyAsync(dq, q, sizeof(double) * n * chains, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(de, 0, sizeof(int), m->stream));
    int ch = chains;
    if (use_tick) {
      // the tick engine's gradient path exactly as the sampler drives it: the row-streaming gradient kernel fills the
      // per-split partial sums (and, in gather mode, the scatter sums) for all chains, the finish kernel combines them in
      // the same fixed order as rh_tick_kernel (rh_combine_chain) -- so parity tests reach the kernels the bench times
      const bool lane_walk = walk_is_lane(m, false, chains);   // (only where RH_GRAD_WALK=lane asks for it)
      const bool lane_rows = lane_walk && feed_is_rows(m);
      int nsplit = grad_splits > 0 ? grad_splits : (m->info.gather_mode ? 64 : lane_walk ? lane_nsplit(m, chains) : default_nsplit(m, chains));
      GatherBufs gb;
      if (m->info.gather_mode) gb.build(m, chains, nsplit);
      const size_t pbytes = sizeof(double) * (size_t)m->n_row_targets * nsplit * chains * m->nacc_max;
      DevBuf bpart(pbytes), brun(sizeof(int)), blist(sizeof(int) * chains);
      { std::vector<int> ident((size_t)chains);   // every chain is served: the identity list
        for (int c = 0; c < chains; c++) ident[(size_t)c] = c;
        HIPCHK(hipMemcpyAsync(blist.p, ident.data(), sizeof(int) * chains, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream)); }
      HIPCHK(hipMemsetAsync(bpart.p, 0, pbytes, m->stream));
      int xcd = 1;
      if (const char *e = rh::knob("RH_XCD_AWARE")) xcd = std::atoi(e);
      // RH_DIAG only -- RH_EVAL_LIVE="3,7,8": the launch serves exactly these chains through a compacted list, as the sampler's launches
      // do (rh_compact_kernel); the rows of the chains it leaves out come back as zeros (tools/r6_live_diag.py)
      void *dnl = nullptr;
      std::unique_ptr<DevBuf> bnl;
      if (const char *e = rh::knob("RH_EVAL_LIVE")) {
        std::vector<int> live;
        for (const char *p = e; *p;) { char *q2; long v = std::strtol(p, &q2, 10); if (q2 == p) break; if (v >= 0 && v < chains) live.push_back((int)v); p = *q2 ? q2 + 1 : q2; }
        std::sort(live.begin(), live.end());
        live.erase(std::unique(live.begin(), live.end()), live.end());
        if (!live.empty()) {
          const int nl = (int)live.size();
          HIPCHK(hipMemcpyAsync(blist.p, live.data(), sizeof(int) * nl, hipMemcpyHostToDevice, m->stream));
          bnl.reset(new DevBuf(sizeof(int)));
          HIPCHK(hipMemcpyAsync(bnl->p, &nl, sizeof(int), hipMemcpyHostToDevice, m->stream));
          HIPCHK(hipStreamSynchronize(m->stream));
          dnl = bnl->p;
        }
      }
      launch_grad(m, &gb, dq, blist.p, dnl, nullptr, bpart.p, de, brun.p, chains, nsplit, xcd, nullptr, lane_walk, lane_rows);
      void *dpart = bpart.p;
      if (m->info.gather_mode) {
        void *fa[] = {&m->data, &gb.gd, &dq, &dpart, &dl, &dg, &de, &ch, &nsplit, &dtot};
        launch(m->k_density_fin, (unsigned)chains, 64, m->stream, fa);
      } else {
        void *fa[] = {&m->data, &dq, &dpart, &dl, &dg, &de, &ch, &nsplit, &dtot};
        launch(m->k_density_fin, (unsigned)chains, 64, m->stream, fa);
      }
      HIPCHK(hipMemcpyAsync(logp, dl, sizeof(double) * chains, hipMemcpyDeviceToHost, m->stream));
      HIPCHK(hipMemcpyAsync(grad, dg, sizeof(double) * n * chains, hipMemcpyDeviceToHost, m->stream));
      HIPCHK(hipMemcpyAsync(&lookup_err, de, sizeof(int), hipMemcpyDeviceToHost, m->stream));
      HIPCHK(hipStreamSynchronize(m->stream));
      return;
    }
    void *args[] = {&m->data, &dq, &dl, &dg, &de, &ch, &dtot};
    launch(m->k_density, (unsigned)((chains + 64 / m->info.pack_l - 1) / (64 / m->info.pack_l)), 64, m->stream, args);  // packed: 64 / pack_l chains per wavefront
    HIPCHK(hipMemcpyAsync(logp, dl, sizeof(double) * chains, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(grad, dg, sizeof(double) * n * chains, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(&lookup_err, de, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
  });
  if (rc == RH_OK && lookup_err) { m->err = g_err = "Lookup index out of range during evaluation"; return RH_E_LOOKUP; }
  return rc;
}

extern "C" int rh_selftest(rh_model *m, int32_t mode, int64_t seed, const double *in, double *out, int32_t n) {
  if (!m || !m->loaded || !out || n <= 0) { g_err = "rh_selftest: bad arguments"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(m->mu);
  return guard(m, [&] {
    HIPCHK(hipSetDevice(m->device));
    const size_t in_n = (mode == 5 || mode == 14) ? 2 * (size_t)n : (size_t)n;
    DevBuf bin(sizeof(double) * in_n), bout(sizeof(double) * n);
    void *din = bin.p, *dout = bout.p;
    if (mode >= 2) HIPCHK(hipMemcpyAsync(din, in, sizeof(double) * in_n, hipMemcpyHostToDevice, m->stream));
    int md = mode, nn = n; long long sd = seed;
    void *args[] = {&md, &sd, &din, &dout, &nn};
    launch(m->k_selftest, mode <= 1 ? 1u : 64u, 64, m->stream, args);
    HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
  });
}

// ---- seam 3 -----------------------------------------------------------------------------------------
extern "C" void rh_config_default(rh_config *c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->struct_size = (int32_t)sizeof(rh_config);
  c->iterations = 1000; c->warmup = 1000;                     // Sampler.scala:18-19
  c->sampler = RH_SAMPLER_EHMC; c->hmc_steps = 1;
  c->ehmc_max_steps = 1024; c->ehmc_min_steps = 1; c->ehmc_buf_size = 100; c->ehmc_p_count = 0.1;  // :26, EHMC.scala:3-6
  c->step_tuner = RH_STEP_DUALAVG; c->dualavg_delta = 0.8;    // :22-23
  c->static_step = 0.1;
  c->mass_tuner = RH_MASS_DIAG_WINDOWED;                      // :24-25
  c->mass_init_window = 50; c->mass_expansion = 1.5; c->mass_skip_first = 50; c->mass_skip_last = 50;
}

// ---- create-time self-check ------------------------------------------------------------------------------------------------------
// The sampler kernels carry their own inlined copy of the model's density (rh_chain_kernel: the whole row walk; rh_tick_kernel:
// the data-free targets and the combination of the gradient kernel's partial sums).  Before an engine is used for the first time
// with a sampler-kernel variant, three chains are initialised with it (LeapFrog.initialize: one gradient at a N(0, 1) point) and the
// (logp, gradient) they hold is compared with the density path of seam 2 at the same points -- different kernels of the same
// translation unit, with different register pressure and different control flow around the same row code.  A disagreement beyond
// summation-order noise is this toolchain's register-allocator fault (or a bug of ours) showing on this very model and data: the
// engine is taken out of use (AUTO then chooses the other one, an explicit request fails with the reason).  RH_SELFCHECK=0 skips it.
namespace {
thread_local int g_force_variant = -1;   // set while a self-check sampler is created: the variant is given, and no nested check
bool selfcheck_engine(rh_model *m, KSet &ks, int v, bool tick) {
  if (g_force_variant >= 0 || !selfcheck_enabled()) return true;
  bool &done = tick ? ks.tick_checked : ks.chain_checked;
  if (done) return true;
  // the reference: rh_density_kernel where it exists and the data are small enough for one wavefront per chain, else the tick
  // engine's gradient path (for the tick engine that still checks rh_tick_kernel against rh_density_fin_kernel)
  const bool ref_density = m->density_ok && m->rows_total <= ((int64_t)1 << 22);
  if (!ref_density && !m->tick_ok) { done = true; return true; }
  const int nc = 3, n = (int)m->prog.n_params;
  rh_config cfg;
  rh_config_default(&cfg);
  cfg.iterations = 1; cfg.warmup = 0; cfg.sampler = RH_SAMPLER_HMC; cfg.hmc_steps = 1;
  cfg.step_tuner = RH_STEP_STATIC; cfg.static_step = 1e-3; cfg.mass_tuner = RH_MASS_IDENTITY;
  cfg.engine = tick ? RH_ENGINE_TICK : RH_ENGINE_CHAIN;
  const int64_t seeds[3] = {0x5e1fc4ec, 0x5e1fc4ed, 0x5e1fc4ee};
  std::string why;
  rh_sampler *s2 = nullptr;
  g_force_variant = v;
  int rc = rh_sampler_create(m, &cfg, seeds, nc, &s2);
  g_force_variant = -1;
  if (rc == RH_OK) rc = rh_sampler_warmup(s2);   // LeapFrog.initialize, then paused at the head of iteration 0
  std::vector<uint64_t> img;
  if (rc == RH_OK) {
    img.resize((size_t)nc * ks.state_words);
    if (hipMemcpy(img.data(), s2->d_state, img.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) rc = RH_E_DEVICE;
  }
  if (s2) rh_sampler_destroy(s2);
  if (rc != RH_OK) why = "self-check run failed: " + m->err;
  else {
    std::vector<double> q((size_t)nc * n), g((size_t)nc * n), lp(nc), gr((size_t)nc * n), lr(nc);
    for (int c = 0; c < nc; c++) {
      const uint64_t *st = img.data() + (size_t)c * ks.state_words;
      std::memcpy(&q[(size_t)c * n], st + ks.off_Pq, sizeof(double) * n);
      std::memcpy(&g[(size_t)c * n], st + ks.off_Pg, sizeof(double) * n);
      double pu; std::memcpy(&pu, st + ks.off_PU, sizeof pu);
      lp[c] = -pu;
    }
    rc = rh_density_eval_ex(m, q.data(), nc, ref_density ? RH_ENGINE_CHAIN : RH_ENGINE_TICK, 0, lr.data(), gr.data());
    if (rc == RH_E_LOOKUP) { done = true; return true; }   // (a Lookup index out of range in the data: the sampler reports it itself)
    if (rc != RH_OK) why = "self-check reference failed: " + m->err;
    for (int c = 0; c < nc && why.empty(); c++) {
      std::string what;
      if (!outputs_agree(&lp[c], &g[(size_t)c * n], &lr[c], &gr[(size_t)c * n], n, what))
        why = std::string("create-time self-check: ") + (tick ? "rh_tick_kernel" : "rh_chain_kernel") + " disagrees with " +
              (ref_density ? "rh_density_kernel" : "rh_density_fin_kernel") + " at an initial point (" + what + ")";
    }
  }
  done = true;
  if (why.empty()) return true;
  if (tick) { ks.k_tick = nullptr; ks.why_tick = why; } else { ks.k_chain = nullptr; ks.why_chain = why; }
  std::fprintf(stderr, "rainier-hip: the %s engine is taken out of use for this model: %s\n", tick ? "tick" : "chain", why.c_str());   // never silently
  return false;
}
}  // namespace

extern "C" int rh_sampler_create(rh_model *m, const rh_config *cfg, const int64_t *seeds, int32_t chains, rh_sampler **out) {
  if (!out) { g_err = "rh_sampler_create: out is NULL"; return RH_E_INVALID; }
  *out = nullptr;
  if (!m || !m->loaded) { g_err = "rh_sampler_create: model not loaded"; return RH_E_INVALID; }
  rh_sampler *s = new rh_sampler();
  const int rc = guard(m, [&] {
    if (!cfg || cfg->struct_size != (int32_t)sizeof(rh_config)) throw Fail{RH_E_INVALID, "rh_config.struct_size mismatch"};
    if (!seeds || chains <= 0) throw Fail{RH_E_INVALID, "seeds/chains invalid"};
    if (cfg->iterations < 0 || cfg->warmup < 0) throw Fail{RH_E_INVALID, "negative iteration count"};
    if (cfg->sampler != RH_SAMPLER_HMC && cfg->sampler != RH_SAMPLER_EHMC && cfg->sampler != RH_SAMPLER_NUTS) throw Fail{RH_E_INVALID, "unknown sampler"};
    if (cfg->sampler == RH_SAMPLER_NUTS && (cfg->nuts_max_depth < 1 || cfg->nuts_max_depth > RH_NUTS_MAXD)) throw Fail{RH_E_INVALID, "nuts_max_depth must be in [1, 12]"};
    if (cfg->sampler == RH_SAMPLER_EHMC && (cfg->ehmc_buf_size < 1 || cfg->ehmc_buf_size > 64 * RH_RING_SLOTS))
      throw Fail{RH_E_INVALID, "ehmc_buf_size must be in [1, 256]"};
    if (cfg->mass_tuner == RH_MASS_STATIC_DIAG) {
      if (!cfg->static_mass) throw Fail{RH_E_INVALID, "static_mass is NULL"};
      for (uint32_t i = 0; i < m->prog.n_params; i++)  // require(!elements.contains(0.0))  MassMatrix.scala:8
        if (cfg->static_mass[i] == 0.0) throw Fail{RH_E_INVALID, "requirement failed: mass matrix element is 0.0"};
    }
    s->m = m; s->chains = chains;
    HIPCHK(hipSetDevice(m->device));
    {
      int v = (cfg->sampler == RH_SAMPLER_NUTS ? 1 : 0) | (cfg->mass_tuner == RH_MASS_DENSE_WINDOWED ? 2 : 0);
      // packed chains share a wavefront: free for lock-step static HMC, but EHMC / NUTS trajectories of different lengths
      // serialise, which only pays once there are more chains than wavefront slots
      s->pack_l = m->info.pack_l;
      if (m->info.pack_l != 64 && cfg->sampler != RH_SAMPLER_HMC && chains < 4096) { v |= 4; s->pack_l = 64; }
      if (g_force_variant >= 0) { v = g_force_variant; s->pack_l = (v & 4) ? 64 : m->info.pack_l; }   // a self-check run of exactly that variant
      if ((v & 2) && (m->prog.n_params > 64 || m->info.bign)) throw Fail{RH_E_UNSUPPORTED, "DenseMassMatrixTuner supports at most 64 parameters"};
      if (cfg->engine < RH_ENGINE_AUTO || cfg->engine > RH_ENGINE_TICK) throw Fail{RH_E_INVALID, "unknown engine"};
      if (cfg->engine == RH_ENGINE_TICK && m->n_row_targets == 0) throw Fail{RH_E_INVALID, "the tick engine needs a model that streams rows"};
      if (cfg->engine == RH_ENGINE_CHAIN && m->info.gather_mode) throw Fail{RH_E_UNSUPPORTED, "gather-mode models run on the tick engine only"};
      KSet *ksp = nullptr;
      { std::lock_guard<std::mutex> lk(m->mu);  // variants are built lazily: two samplers may be created concurrently
        ksp = &load_variant(m, v);
        // a packed variant (several chains per wavefront) whose chain kernel is not fit to run: the one-chain-per-wavefront variant
        // of the same sampler kernels takes its place (same chains, bit for bit; eight-schools' packed NUTS kernel is the case)
        if (!ksp->k_chain && !m->info.gather_mode && !(v & 4) && m->info.pack_l != 64 && g_force_variant < 0) {
          KSet &alt = load_variant(m, v | 4);
          if (alt.k_chain) { v |= 4; s->pack_l = 64; ksp = &alt; }
        } }
      KSet &ks = *ksp;
      // Engine choice.  AUTO: the tick engine for gather mode and from 65 536 rows on, the chain engine below -- and whichever of
      // the two has kernels that are fit to run (kernel_health) and agree with the density kernel on this device (self-check)
      // when the preferred one does not.  An explicit request is never rerouted: it fails with the reason.
      std::lock_guard<std::recursive_mutex> elk(m->engine_mu);   // (two samplers may be created concurrently on one model)
      for (int round = 0; ; round++) {
        const bool want_tick = m->info.gather_mode || cfg->engine == RH_ENGINE_TICK ||
                               (cfg->engine == RH_ENGINE_AUTO && m->n_row_targets > 0 && (m->rows_total >= 65536 || !ks.k_chain));
        bool tick = want_tick;
        if (tick && !ks.k_tick) {
          if (cfg->engine == RH_ENGINE_AUTO && ks.k_chain) tick = false;
          else throw Fail{RH_E_UNSUPPORTED, "the tick engine's kernels of this model are not fit to run: " + ks.why_tick};
        }
        if (!tick && !ks.k_chain) throw Fail{RH_E_UNSUPPORTED, "the chain engine's kernel of this model is not fit to run: " + ks.why_chain +
                                                                 (m->n_row_targets > 0 && cfg->engine == RH_ENGINE_AUTO ? "; tick engine: " + ks.why_tick : std::string())};
        s->tick_engine = tick;
        if (round >= 2 || selfcheck_engine(m, ks, v, tick)) break;   // (a failed check has cleared the kernel and left the reason: choose again)
      }
      s->k_chain = ks.k_chain; s->k_tick = ks.k_tick; s->state_words = ks.state_words; s->dense_off = ks.dense_off;
      s->off_Pq = ks.off_Pq; s->off_Pg = ks.off_Pg; s->off_PU = ks.off_PU;
    }
    rh_cfg_dev &d = s->cfg;
    d.iterations = cfg->iterations; d.warmup = cfg->warmup; d.sampler = cfg->sampler; d.hmc_steps = cfg->hmc_steps;
    d.ehmc_max_steps = cfg->ehmc_max_steps; d.ehmc_min_steps = cfg->ehmc_min_steps; d.ehmc_buf_size = cfg->ehmc_buf_size;
    d.step_tuner = cfg->step_tuner; d.ehmc_p_count = cfg->ehmc_p_count; d.dualavg_delta = cfg->dualavg_delta;
    d.static_step = cfg->static_step; d.mass_tuner = cfg->mass_tuner; d.mass_init_window = cfg->mass_init_window;
    d.mass_skip_first = cfg->mass_skip_first; d.mass_skip_last = cfg->mass_skip_last; d.mass_expansion = cfg->mass_expansion;
    d.nuts_max_depth = cfg->nuts_max_depth;
    HIPCHK(hipSetDevice(m->device));
    const int n = (int)m->prog.n_params;
    const size_t state_bytes = (size_t)chains * s->state_words * sizeof(uint64_t);
    HIPCHK(hipMalloc(&s->d_state, state_bytes));
    HIPCHK(hipMalloc(&s->d_seeds, sizeof(int64_t) * 2 * chains));  // per chain: seed, bits of the pending nextNextGaussian
    HIPCHK(hipMalloc(&s->d_mass, sizeof(double) * n));
    const size_t draws_bytes = (size_t)chains * (size_t)(cfg->iterations ? cfg->iterations : 1) * n * sizeof(double);
    HIPCHK(hipMalloc(&s->d_draws, draws_bytes));
    HIPCHK(hipMalloc(&s->d_stats, sizeof(rh_chain_stats_dev) * chains));
    HIPCHK(hipMalloc(&s->d_running, sizeof(int)));
    {
      std::vector<int64_t> rec((size_t)2 * chains);
      for (int c = 0; c < chains; c++) {
        const double nn = cfg->rng_next_gaussian ? cfg->rng_next_gaussian[c] : std::nan("");
        rec[2 * c] = seeds[c];
        std::memcpy(&rec[2 * c + 1], &nn, sizeof nn);
      }
      HIPCHK(hipMemcpy(s->d_seeds, rec.data(), sizeof(int64_t) * rec.size(), hipMemcpyHostToDevice));
    }
    std::vector<double> mass(n, 1.0);
    if (cfg->mass_tuner == RH_MASS_STATIC_DIAG) mass.assign(cfg->static_mass, cfg->static_mass + n);
    HIPCHK(hipMemcpy(s->d_mass, mass.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->d_draws, 0, draws_bytes));
    HIPCHK(hipEventCreate(&s->e0));
    HIPCHK(hipEventCreate(&s->e1));
    s->last_stats.resize(chains);
    if (s->tick_engine) {
      // The walk of the gradient launches, for the sampler's whole life (warm-up, every request of a trajectory): the lane walk where
      // lanes_plan.hpp's rule says so, from the model, the configuration and the chains of the WHOLE sampler.  It has no fused form
      // (each workgroup would combine 64 C chains x nsplit partial sums in its prologue, nsplit^2 x chains sums per launch: more
      // bytes than the rows), so its trajectories run launch, tick, launch.
      s->lane_walk = walk_is_lane(m, cfg->sampler == RH_SAMPLER_HMC, g_total_chains > 0 ? g_total_chains : chains);
      s->lane_rows = s->lane_walk && feed_is_rows(m);
      int nsplit = cfg->grad_splits;
      if (nsplit <= 0) nsplit = s->lane_walk ? lane_nsplit(m, g_total_chains > 0 ? g_total_chains : chains) : default_nsplit(m, chains);
      // The dynamic samplers' trajectories end at different launches (EHMC: DefaultConfig's, sampler/Sampler.scala:17-27; NUTS:
      // BASELINE's): their launches serve the LISTED chains only (rh_compact_kernel), and the rows are cut into 8 x as many, shorter
      // splits as a lock-step launch needs, so that a launch with few live chains still spreads over the machine (as long as a
      // split keeps >= 1024 rows).  Static HMC runs in lock step -- every launch serves every chain -- and keeps the count it had.
      // A function of the sampler and the model only: a chain's sums do not depend on how many chains there are, are live, or
      // share the device (rh_sample_multi fixes grad_splits from the total chain count).
      int subf = cfg->sampler == RH_SAMPLER_HMC ? 1 : 8;
      if (const char *e = rh::knob("RH_SUBF")) { subf = 1; while (subf * 2 <= std::atoi(e) && subf < 64) subf *= 2; }
      if (const char *e = rh::knob("RH_COMPACT")) s->compact = std::atoi(e) != 0;
      { int64_t max_rows = 1;
        for (size_t t = 0; t < m->prog.targets.size(); t++) if (m->prog.targets[t].n_cols) max_rows = std::max<int64_t>(max_rows, m->data.nrows[t]);
        while (subf > 1 && max_rows / ((int64_t)nsplit * subf) < 1024) subf >>= 1; }
      if (!m->k_compact) s->compact = false;
      nsplit *= subf;
      if (nsplit > 65536) throw Fail{RH_E_INVALID, "grad_splits too large"};
      s->nsplit = nsplit;
      if (const char *e = rh::knob("RH_XCD_AWARE")) s->xcd_aware = std::atoi(e);
      HIPCHK(hipMalloc(&s->d_qbuf, sizeof(double) * n * chains));
      HIPCHK(hipMalloc(&s->d_active, sizeof(int) * chains));
      HIPCHK(hipMemset(s->d_qbuf, 0, sizeof(double) * n * chains));
      HIPCHK(hipMemset(s->d_active, 0, sizeof(int) * chains));
      const size_t rec_u64 = (size_t)(3 * n + 8);   // RH_REC_U64 (rh_engine.hip.h)
      {  // The fused launch (rh_grad_fused_kernel: static HMC's mid-trajectory update as the gradient launch's prologue) needs the
         // base sampler-kernel variant (its state layout is compiled into the gradient module), the plain VALU gradient kernel and
         // a lock-step sampler.  Chains are bit-identical with and without it (tests/test_gpu_fused.py); RH_FUSE=0 turns it off.
        bool fuse = m->k_grad_fused && m->k_absorb && s->k_tick == m->k_tick && cfg->sampler == RH_SAMPLER_HMC && !m->k_grad_glm && !s->lane_walk;
        if (const char *e = rh::knob("RH_FUSE")) fuse = fuse && std::atoi(e) != 0;
        if (fuse) {
          const size_t rec_bytes = sizeof(uint64_t) * rec_u64 * chains;
          for (int k = 0; k < 2; k++) { HIPCHK(hipMalloc(&s->d_rec[k], rec_bytes)); HIPCHK(hipMemset(s->d_rec[k], 0, rec_bytes)); }
          s->fuse = true;
        }
      }
      // The lanes (lanes_plan.hpp): nsplit above came from the total chain count, so a chain's sums are the same in one lane and
      // in two.  Without a switch lanes_cut's rule decides: two lanes where each alone still offers a wavefront to every SIMD
      // (measured on cfg 2, profiles/lanes_cfg2: +4 % under static HMC, +1.5..5 % under DefaultConfig).  RH_LANES=1|2 forces the
      // count (2: wherever there are two chain groups to part).
      int forced = 0;
      if (const char *e = rh::knob("RH_LANES")) forced = std::atoi(e) == 1 ? 1 : (std::atoi(e) == 2 ? 2 : 0);
      const rh_plan::LaneCut cut = rh_plan::lanes_cut(chains, s->lane_walk ? rh_plan::kLaneGroup : m->k_grad_glm ? 16 : m->grad_k, nsplit,
                                                      s->lane_walk ? rh_plan::kLaneW : m->k_grad_glm ? m->glm_w : 1, device_cus(m->device), forced);
      s->lanes.resize((size_t)cut.lanes);
      // The longest round (lanes_plan.hpp round_launches) sizes each lane's live log and event pools; RH_ROUND_MAX=n lowers it, so
      // that tests cross round boundaries at tiny sizes.
      s->round_cap = rh_plan::kRoundCapDefault;
      if (const char *e = rh::knob("RH_ROUND_MAX")) s->round_cap = rh_plan::round_cap(std::atoi(e));
      const size_t cap = (size_t)s->round_cap;
      const size_t iters_alloc = (size_t)cfg->iterations;   // (a chain's draws are addressed as chain * cfg.iterations * n)
      for (int li = 0; li < cut.lanes; li++) {
        Lane &L = s->lanes[(size_t)li];
        const int f = cut.first[li], lc = cut.count[li];
        L.first = f; L.chains = lc;
        if (li == 0) L.stream = m->stream;
        else { HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking)); L.own_stream = true; }
        HIPCHK(hipEventCreate(&L.e0));
        HIPCHK(hipEventCreate(&L.e1));
        for (int p = 0; p < 2; p++) { HIPCHK(hipEventCreate(&L.r0[p])); HIPCHK(hipEventCreate(&L.r1[p])); }
        L.state = (uint64_t *)s->d_state + (size_t)f * s->state_words;
        L.seeds = (int64_t *)s->d_seeds + (size_t)2 * f;
        L.draws = (double *)s->d_draws + (size_t)f * iters_alloc * n;
        L.stats = (rh_chain_stats_dev *)s->d_stats + f;
        L.qbuf = (double *)s->d_qbuf + (size_t)f * n;
        L.active = (int *)s->d_active + f;
        for (int k = 0; k < 2; k++) L.rec[k] = s->d_rec[k] ? (uint64_t *)s->d_rec[k] + (size_t)f * rec_u64 : nullptr;
        const size_t partial_bytes = sizeof(double) * (size_t)m->n_row_targets * nsplit * lc * m->nacc_max;
        HIPCHK(hipMalloc(&L.d_running, sizeof(int)));
        HIPCHK(hipMalloc(&L.d_list, sizeof(int) * lc));
        HIPCHK(hipMalloc(&L.d_nlive, sizeof(int)));
        HIPCHK(hipMalloc(&L.d_livelog, sizeof(int) * (cap + 1)));
        HIPCHK(hipMemset(L.d_livelog, 0, sizeof(int) * (cap + 1)));
        { std::vector<int> ident((size_t)lc);   // (the list of a sampler that does not compact: every chain, every launch)
          for (int c = 0; c < lc; c++) ident[(size_t)c] = c;
          HIPCHK(hipMemcpy(L.d_list, ident.data(), sizeof(int) * lc, hipMemcpyHostToDevice)); }
        HIPCHK(hipMemset(L.d_nlive, 0, sizeof(int)));
        HIPCHK(hipMalloc(&L.d_partial, partial_bytes));
        HIPCHK(hipMalloc(&L.d_graderr, sizeof(int)));
        HIPCHK(hipMemset(L.d_graderr, 0, sizeof(int)));
        if (s->fuse) HIPCHK(hipMalloc(&L.d_partial2, partial_bytes));
        if (m->info.gather_mode) {
          HIPCHK(hipMemset(L.d_partial, 0, partial_bytes));
          L.gb = new GatherBufs(); L.gb->build(m, lc, nsplit);
        }
        for (int p = 0; p < 2; p++) { L.livelog[p].assign(cap, 0); L.was_ticked[p].assign(cap, 0); }
      }
    }
    // The buffers above were cleared with hipMemset: fill KERNELS on the null stream that return before they have run, while the
    // sampler's launches go to the model's non-blocking stream -- a late fill of `active` / `qbuf` would wipe what the first tick has
    // published (seen under `rocprofv3 --pmc`, where dispatches are serialised: the round-4 self-check caught the first gradient
    // of a 3-chain sampler summing 29 of its 488 row splits).  Everything is in place before the handle leaves this function.
    HIPCHK(hipDeviceSynchronize());
  });
  if (rc != RH_OK) { rh_sampler_destroy(s); return rc; }
  *out = s;
  return RH_OK;
}

namespace {
// Tick engine: the timing figures of the last finished round, read out of its events.  advance_to_ticks leaves a round as a record
// (s->round: which lanes ran, how many launches, which event pool) and calls this only once the NEXT round is in the streams -- the
// device works while the host asks for a few thousand elapsed times and sorts them -- or, when nothing follows, not at all: then
// rh_sampler_timing, the sampler's next advance or its destruction does.  Only ever called after the stream synchronisation that
// ended the round, so every event asked about has completed; and always before the round's pool is recorded again.
//   total_ms: the union of the live lanes' [r0, r1] spans of the round.
//   Every launch's span; with two lanes in flight on one time base (hipEventElapsedTime from one reference event works across the
//   streams of a device), and a launch is charged its busy share: the time it ran alone + half of the time it ran beside the other
//   lane's.  kernel_ms then is the time during which a gradient launch was running, and never exceeds total_ms.
void resolve_round(rh_sampler *s) {
  RoundRec &R = s->round;
  if (!R.open) return;
  R.open = false;   // (whatever a query below answers, the round is not asked about twice)
  HIPCHK(hipSetDevice(s->m->device));
  const int p = R.pool, nl = (int)s->lanes.size();
  int nlive = 0;
  for (int li = 0; li < nl; li++) nlive += R.live[li] ? 1 : 0;
  hipEvent_t ref = nullptr;
  {
    double t0[2], t1[2], share[2];
    int k = 0;
    for (int li = 0; li < nl; li++) {
      if (!R.live[li]) continue;
      Lane &L = s->lanes[(size_t)li];
      float a = 0, b = 0;
      if (!ref) ref = L.r0[p]; else HIPCHK(hipEventElapsedTime(&a, ref, L.r0[p]));
      HIPCHK(hipEventElapsedTime(&b, L.r0[p], L.r1[p]));
      t0[k] = a; t1[k] = (double)a + b; k++;
    }
    s->total_ms += k == 1 ? t1[0] - t0[0] : rh_plan::busy_shares(k, t0, t1, share);
  }
  std::vector<double> t0, t1, share;
  for (int li = 0; li < nl; li++) {
    if (!R.live[li]) continue;
    Lane &L = s->lanes[(size_t)li];
    for (int i = 0; i < R.B[li]; i++) {
      float a = 0, g = 0;
      if (nlive > 1) HIPCHK(hipEventElapsedTime(&a, ref, L.ev[p][(size_t)2 * i]));
      HIPCHK(hipEventElapsedTime(&g, L.ev[p][(size_t)2 * i], L.ev[p][(size_t)2 * i + 1]));
      t0.push_back(a); t1.push_back((double)a + g);
    }
  }
  share.resize(t0.size());
  if (nlive > 1) rh_plan::busy_shares((int)t0.size(), t0.data(), t1.data(), share.data());
  else for (size_t i = 0; i < t0.size(); i++) share[i] = t1[i] - t0[i];
  size_t at = 0;
  for (int li = 0; li < nl; li++) {
    if (!R.live[li]) continue;
    Lane &L = s->lanes[(size_t)li];
    for (int i = 0; i < R.B[li]; i++, at++) {
      const double g = share[at];
      s->kernel_ms += g;
      // launch i served the chains listed by the last compaction before it (rounds are resolved in order: cur_live is carried from
      // the call's first tick through every round)
      const int served = L.cur_live;
      s->chain_slots += served;
      if ((int64_t)served * 10 >= (int64_t)L.chains * 9) { s->steady_ms += g; s->steady_launches += 1; s->steady_evals += served; }
      if (s->compact && L.was_ticked[p][(size_t)i]) L.cur_live = L.livelog[p][(size_t)i];
    }
    s->launches += R.B[li];
  }
}
}  // namespace

extern "C" void rh_sampler_destroy(rh_sampler *s) {
  if (!s) return;
  if (s->m) hipSetDevice(s->m->device);
  if (s->m) (void)guard(nullptr, [&] { resolve_round(s); });   // (nobody reads the figures any more: the record is closed so that no pool is left recorded and unread)
  for (void *p : {s->d_state, s->d_seeds, s->d_mass, s->d_draws, s->d_stats, s->d_running, s->d_qbuf, s->d_active, s->d_rec[0], s->d_rec[1]})
    if (p) hipFree(p);
  for (Lane &L : s->lanes) {
    for (void *p : {L.d_running, L.d_list, L.d_nlive, L.d_livelog, L.d_partial, L.d_partial2, L.d_graderr})
      if (p) hipFree(p);
    for (int p = 0; p < 2; p++) {
      for (hipEvent_t e : L.ev[p]) hipEventDestroy(e);
      if (L.r0[p]) hipEventDestroy(L.r0[p]);
      if (L.r1[p]) hipEventDestroy(L.r1[p]);
    }
    if (L.e0) hipEventDestroy(L.e0);
    if (L.e1) hipEventDestroy(L.e1);
    delete L.gb;
    if (L.own_stream && L.stream) hipStreamDestroy(L.stream);
  }
  if (s->e0) hipEventDestroy(s->e0);
  if (s->e1) hipEventDestroy(s->e1);
  delete s;
}

namespace {
// tick engine: [tick, all chains] [compact] then repeat { [grad] [tick] [compact] } until no chain asks for a gradient any more.
// rh_compact_kernel lists the chains whose tick asked for a gradient; the gradient launch and the tick behind it serve exactly those.
// The launches go out in ROUNDS (lanes_plan.hpp round_launches: a lock-step run's whole remainder, 32 otherwise), each ended by a
// synchronisation and the read-back of `running`.  With two lanes a round is enqueued step-major -- launch i of lane 0, launch i of
// lane 1, launch i + 1 of lane 0, ... -- so that both streams have work from the round's first microseconds to its last and neither
// lane runs a stretch alone while the host is still busy with the other's launches; a lane whose chains have all arrived drops out of
// the rounds that follow.  What a round means for the timing figures is read out of its events later (resolve_round).
void advance_to_ticks(rh_sampler *s, int it_stop) {
  rh_model *m = s->m;
  HIPCHK(hipSetDevice(m->device));
  resolve_round(s);   // (a round the last call left unread)
  int nsplit = s->nsplit, stop = it_stop, xcd = s->xcd_aware;
  void *no_list = nullptr;
  bool value_free = true;   // gradient-only requests (RH_VALUE_FREE=0: every launch computes the log-density too)
  if (const char *e = rh::knob("RH_VALUE_FREE")) if (std::atoi(e) == 0) value_free = false;
  auto tick = [&](Lane &L, int fresh, bool reset_counter, void *partial, bool listed, int log_slot) {
    int chains = L.chains;
    if (reset_counter) HIPCHK(hipMemsetAsync(L.d_running, 0, sizeof(int), L.stream));
    void *lst = listed && s->compact ? L.d_list : no_list, *nl = listed && s->compact ? L.d_nlive : no_list;
    if (m->info.gather_mode) {
      void *args[] = {&m->data, &L.gb->gd, &s->cfg, &L.state, &L.seeds, &s->d_mass, &L.draws, &L.stats, &L.d_running, &L.qbuf,
                      &L.active, &partial, &L.d_graderr, &lst, &nl, &chains, &nsplit, &stop, &fresh};
      launch(s->k_tick, (unsigned)chains, 64, L.stream, args);
    } else {
      void *args[] = {&m->data, &s->cfg, &L.state, &L.seeds, &s->d_mass, &L.draws, &L.stats, &L.d_running, &L.qbuf,
                      &L.active, &partial, &L.d_graderr, &lst, &nl, &chains, &nsplit, &stop, &fresh};
      launch(s->k_tick, (unsigned)chains, 64, L.stream, args);
    }
    if (s->compact) {
      void *lg = (int *)L.d_livelog + log_slot;
      void *ca[] = {&L.active, &L.d_list, &L.d_nlive, &lg, &chains};
      launch(m->k_compact, 1u, 1024, L.stream, ca);
    }
  };
  auto grad = [&](Lane &L, void *partial) {
    launch_grad(m, L.gb, L.qbuf, L.d_list, s->compact ? L.d_nlive : nullptr /* (without compaction d_list stays the identity) */,
                value_free ? L.active : nullptr, partial, L.d_graderr, L.d_running, L.chains, nsplit, xcd, L.stream, s->lane_walk, s->lane_rows);
  };
  // gradient at the point the PREVIOUS launch's gradient moves every chain to (rh_fused_prologue); no tick between the two
  auto grad_fused = [&](Lane &L, void *partial_in, void *partial_out, void *rec_in, void *rec_out) {
    int chains = L.chains;
    void *live_n = s->compact ? L.d_nlive : nullptr;
    void *args[] = {&m->data, &L.qbuf, &L.d_list, &live_n, &partial_in, &partial_out, &L.d_graderr, &L.d_running, &L.state, &rec_in, &rec_out,
                    &chains, &nsplit, &xcd};
    launch(m->k_grad_fused, (unsigned)(((chains + m->grad_k - 1) / m->grad_k) * nsplit), 64, L.stream, args);
  };
  auto absorb = [&](Lane &L, void *rec) {
    int chains = L.chains;
    void *args[] = {&L.state, &rec, &L.qbuf, &L.active, &chains};
    launch(m->k_absorb, (unsigned)chains, 64, L.stream, args);
  };
  // Static HMC in the sampling phase runs in lock step: every chain was paused at the head of the same iteration, so gradient
  // request j of a trajectory is request j of every chain, and all but the L-th are followed by the plain update the fused
  // launch that follows performs itself in its prologue.  (A chain that is out of step anyway is simply served by the next tick.)
  const int Ltraj = std::max(1, s->cfg.hmc_steps);
  const bool fuse_now = s->fuse && s->warmed && s->cfg.sampler == RH_SAMPLER_HMC && Ltraj > 1;
  // launches between host checks: the count is exact for static HMC in the sampling phase (lanes_plan.hpp round_launches)
  const bool lock_step = s->cfg.sampler == RH_SAMPLER_HMC && s->warmed;
  const long long todo = lock_step ? (long long)std::max(0, it_stop - (s->cfg.warmup + s->it_done)) * Ltraj : 0;
  // the union of the lanes' [e0, e1] spans of the call's first tick -> total_ms (two or three queries: not worth deferring)
  auto add_total = [&]() {
    hipEvent_t ref = nullptr;
    double t0[2], t1[2], share[2];
    int k = 0;
    for (Lane &L : s->lanes) {
      if (!L.live) continue;
      float a = 0, b = 0;
      if (!ref) ref = L.e0; else HIPCHK(hipEventElapsedTime(&a, ref, L.e0));
      HIPCHK(hipEventElapsedTime(&b, L.e0, L.e1));
      t0[k] = a; t1[k] = (double)a + b; k++;
    }
    s->total_ms += k == 1 ? t1[0] - t0[0] : rh_plan::busy_shares(k, t0, t1, share);
  };
  for (Lane &L : s->lanes) {
    L.live = true; L.pos = 0; L.remaining = todo;
    HIPCHK(hipEventRecord(L.e0, L.stream));
    tick(L, s->started ? 0 : 1, true, L.d_partial, false, s->round_cap);   // (its live count: the slot behind a round's)
    HIPCHK(hipEventRecord(L.e1, L.stream));
  }
  s->started = true;
  // One launch of a round on one lane: [event] gradient [event], and -- unless the fused launch that follows does the update itself --
  // the tick that consumes it, with its compaction
  auto step = [&](Lane &L, int pool, int i) {
    void *pbuf[2] = {L.d_partial, L.d_partial2};
    std::vector<hipEvent_t> &ev = L.ev[pool];
    while (ev.size() < (size_t)2 * (i + 1)) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }   // (while the device works on the launches before)
    // the last launch of a round is always followed by a tick: it is the tick that counts the chains still running
    const bool ticked = !(fuse_now && (int)(L.pos % Ltraj) + 1 < Ltraj && i != L.B - 1);
    const int cur = fuse_now ? L.pp : 0;
    HIPCHK(hipEventRecord(ev[(size_t)2 * i], L.stream));
    if (L.pending) grad_fused(L, pbuf[cur ^ 1], pbuf[cur], L.prev_rec ? L.rec[cur ^ 1] : nullptr, L.rec[cur]);
    else grad(L, pbuf[cur]);
    HIPCHK(hipEventRecord(ev[(size_t)2 * i + 1], L.stream));
    L.prev_rec = L.pending;
    if (ticked) {
      if (L.prev_rec) absorb(L, L.rec[cur]);
      tick(L, 0, false, pbuf[cur], true, i);
    }
    L.pending = !ticked;
    L.was_ticked[pool][(size_t)i] = ticked ? 1 : 0;
    if (fuse_now) L.pp ^= 1;
    L.pos++;
  };
  for (bool first = true;; first = false) {
    // (a copy to pageable host memory returns when it is done: the read-backs come after ALL lanes' launches have been enqueued)
    for (Lane &L : s->lanes) {
      if (!L.live) continue;
      L.running = 0;
      HIPCHK(hipMemcpyAsync(&L.running, L.d_running, sizeof(int), hipMemcpyDeviceToHost, L.stream));
      if (first && s->compact) HIPCHK(hipMemcpyAsync(&L.cur_live, (int *)L.d_livelog + s->round_cap, sizeof(int), hipMemcpyDeviceToHost, L.stream));
      if (!first && s->compact) HIPCHK(hipMemcpyAsync(L.livelog[s->round.pool].data(), L.d_livelog, sizeof(int) * (size_t)L.B, hipMemcpyDeviceToHost, L.stream));
    }
    for (Lane &L : s->lanes) if (L.live) HIPCHK(hipStreamSynchronize(L.stream));
    if (first) add_total();
    else s->round.open = true;   // the round is over and its events have completed: from here on it may be resolved
    int nlive_lanes = 0;
    for (Lane &L : s->lanes) {
      if (!L.live) continue;
      if (!s->compact) L.cur_live = L.chains;
      if (L.running == 0) L.live = false; else nlive_lanes++;
    }
    if (nlive_lanes == 0) break;
    // The next round, step-major, into the event pool the last round did not use
    const int pool = s->next_pool;
    RoundRec next;
    next.pool = pool;
    int maxB = 0;
    for (size_t li = 0; li < s->lanes.size(); li++) {
      Lane &L = s->lanes[li];
      if (!L.live) continue;
      L.B = rh_plan::round_launches(lock_step, lock_step ? L.remaining : rh_plan::kRoundHint, Ltraj, s->round_cap);
      L.pending = L.prev_rec = false;
      next.live[li] = true; next.B[li] = L.B;
      maxB = std::max(maxB, L.B);
      HIPCHK(hipEventRecord(L.r0[pool], L.stream));
    }
    for (int i = 0; i < maxB; i++)
      for (Lane &L : s->lanes) {
        if (!L.live || i >= L.B) continue;
        step(L, pool, i);
        if (i == L.B - 1) HIPCHK(hipEventRecord(L.r1[pool], L.stream));
      }
    // the device has this round to work on: time to read the last one's figures out of the other pool
    resolve_round(s);
    s->round = next;
    s->next_pool = pool ^ 1;
    for (Lane &L : s->lanes) if (L.live) L.remaining = std::max(0LL, L.remaining - L.B);
  }
}

// drive every chain to global iteration index it_stop (warmup iterations count first)
void advance_to(rh_sampler *s, int it_stop) {
  if (s->tick_engine) { advance_to_ticks(s, it_stop); return; }
  rh_model *m = s->m;
  HIPCHK(hipSetDevice(m->device));
  // bound one launch to roughly seconds of device time: a tick streams rows_total rows per chain
  long long ticks = 4000000000LL / (m->rows_total + 2000);
  int max_ticks = (int)std::min<long long>(std::max<long long>(ticks, 8), 1 << 22);
  for (;;) {
    int fresh = s->started ? 0 : 1, chains = s->chains, stop = it_stop;
    HIPCHK(hipMemsetAsync(s->d_running, 0, sizeof(int), m->stream));
    void *args[] = {&m->data, &s->cfg, &s->d_state, &s->d_seeds, &s->d_mass, &s->d_draws, &s->d_stats, &s->d_running,
                    &chains, &stop, &max_ticks, &fresh};
    HIPCHK(hipEventRecord(s->e0, m->stream));
    launch(s->k_chain, (unsigned)((chains + 64 / s->pack_l - 1) / (64 / s->pack_l)), 64, m->stream, args);
    HIPCHK(hipEventRecord(s->e1, m->stream));
    int running = 0;
    HIPCHK(hipMemcpyAsync(&running, s->d_running, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s->e0, s->e1));
    s->kernel_ms += ms;
    s->total_ms += ms;
    s->launches += 1;
    s->started = true;
    if (running == 0) break;
  }
}
void fetch_stats(rh_sampler *s) {
  HIPCHK(hipSetDevice(s->m->device));
  HIPCHK(hipMemcpy(s->last_stats.data(), s->d_stats, sizeof(rh_chain_stats_dev) * s->chains, hipMemcpyDeviceToHost));
}
}  // namespace

namespace {
// Run-time spot check of the tick engine (VERDICT r5 next #6b): the create-time self-checks compare the kernels at three points once;
// this one runs behind every rh_sampler_run.  The current point of three chains -- (q, gradient, log-density) as the sampler carries
// them in its state, i.e. as the batched gradient launches of the run produced them (live-chain lists, gradient-only requests, fused
// prologues and all) -- is evaluated again from scratch: on rh_density_kernel (another kernel around the same row code, one wavefront
// per chain) when the model has one and the data are small enough for it, otherwise through a fresh, uncompacted launch of the
// gradient path.  A disagreement beyond summation-order noise is RH_E_DEVICE naming the kernels.  Cost: three small copies and one
// density evaluation per call.
int spot_check(rh_sampler *s) {
  rh_model *m = s->m;
  if (!s->tick_engine || s->off_Pq < 0 || s->it_done <= 0 || !selfcheck_enabled()) return RH_OK;
  if (const char *e = rh::knob("RH_SPOTCHECK")) if (std::atoi(e) == 0) return RH_OK;
  const bool ref_density = m->density_ok && !m->info.gather_mode && m->rows_total <= ((int64_t)1 << 24);
  const int n = (int)m->prog.n_params, nc = std::min(3, s->chains);
  const int pick[3] = {0, s->chains / 2, s->chains - 1};
  std::vector<double> q((size_t)nc * n), g((size_t)nc * n), lp(nc), gr((size_t)nc * n), lr(nc);
  std::vector<uint64_t> img((size_t)s->state_words);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    if (hipSetDevice(m->device) != hipSuccess) return RH_OK;
    for (int c = 0; c < nc; c++) {
      if (hipMemcpy(img.data(), (const uint64_t *)s->d_state + (size_t)pick[c] * s->state_words, img.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return RH_OK;
      std::memcpy(&q[(size_t)c * n], img.data() + s->off_Pq, sizeof(double) * n);
      std::memcpy(&g[(size_t)c * n], img.data() + s->off_Pg, sizeof(double) * n);
      double pu; std::memcpy(&pu, img.data() + s->off_PU, sizeof pu);
      lp[c] = -pu;
    }
  }
  const int rc = rh_density_eval_ex(m, q.data(), nc, ref_density ? RH_ENGINE_CHAIN : RH_ENGINE_TICK, 0, lr.data(), gr.data());
  if (rc != RH_OK) return RH_OK;   // (RH_E_LOOKUP: the sampler reports it itself; anything else: no reference, no verdict)
  for (int c = 0; c < nc; c++) {
    std::string what;
    if (!outputs_agree(&lp[c], &g[(size_t)c * n], &lr[c], &gr[(size_t)c * n], n, what)) {
      rh_timing t; std::memset(&t, 0, sizeof t);
      (void)rh_sampler_timing(s, &t, 0);
      m->err = g_err = std::string("run-time spot check: the point chain ") + std::to_string(pick[c]) + " carries (" + t.dominant_kernel + " + rh_tick_kernel) disagrees with " +
                       (ref_density ? "rh_density_kernel" : "a fresh evaluation through the gradient path") + " at the same q (" + what + "): one of the two is wrong on this device";
      return RH_E_DEVICE;
    }
  }
  return RH_OK;
}
}  // namespace

extern "C" int rh_sampler_warmup(rh_sampler *s) {
  if (!s) { g_err = "rh_sampler_warmup: NULL"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(s->m->mu);
  return guard(s->m, [&] {
    if (s->warmed) return;
    advance_to(s, s->cfg.warmup);
    s->warmed = true;
  });
}
extern "C" int rh_sampler_run(rh_sampler *s, int32_t n) {
  if (!s || n < 0) { g_err = "rh_sampler_run: bad arguments"; return RH_E_INVALID; }
  int rc;
  {
    std::lock_guard<std::mutex> lk(s->m->mu);
    rc = guard(s->m, [&] {
      if (!s->warmed) { advance_to(s, s->cfg.warmup); s->warmed = true; }
      if (s->it_done + n > s->cfg.iterations) throw Fail{RH_E_INVALID, "rh_sampler_run: more iterations than configured"};
      advance_to(s, s->cfg.warmup + s->it_done + n);
      s->it_done += n;
    });
  }
  return rc == RH_OK && n > 0 ? spot_check(s) : rc;
}
extern "C" int rh_sampler_draws(rh_sampler *s, int32_t first, int32_t count, double *out) {
  if (!s || !out || first < 0 || count < 0 || first + count > s->it_done) { g_err = "rh_sampler_draws: bad range"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(s->m->mu);
  return guard(s->m, [&] {
    HIPCHK(hipSetDevice(s->m->device));
    const size_t n = s->m->prog.n_params, row = n * sizeof(double);
    // draws [chains][iterations][n] -> out [chains][count][n]
    HIPCHK(hipMemcpy2D(out, (size_t)count * row, (const char *)s->d_draws + (size_t)first * row, (size_t)s->cfg.iterations * row,
                       (size_t)count * row, (size_t)s->chains, hipMemcpyDeviceToHost));
  });
}
extern "C" int rh_sampler_draws_device(rh_sampler *s, void **p) {
  if (!s || !p) { g_err = "rh_sampler_draws_device: NULL"; return RH_E_INVALID; }
  *p = s->d_draws;
  return RH_OK;
}
extern "C" int rh_sampler_stats(rh_sampler *s, rh_chain_stats *stats, double *mass_diag) {
  if (!s) { g_err = "rh_sampler_stats: NULL"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(s->m->mu);
  int any_lookup = 0, any_zero_mass = 0;
  const int rc = guard(s->m, [&] {
    fetch_stats(s);
    for (int c = 0; c < s->chains; c++) {
      const rh_chain_stats_dev &d = s->last_stats[c];
      if (d.error & 1) any_lookup = 1;
      if (d.error & 2) any_zero_mass = 1;
      if (!stats) continue;
      rh_chain_stats &o = stats[c];
      o.leapfrog_steps = d.leapfrog_steps; o.warmup_leapfrog_steps = d.warmup_leapfrog_steps;
      o.gradient_evaluations = d.gradient_evaluations; o.accepted = d.accepted;
      o.mean_accept_prob = d.sampling_iterations ? d.sum_accept_prob / (double)d.sampling_iterations : 0.0;
      o.step_size = d.step_size; o.error = (d.error & 1) ? RH_E_LOOKUP : ((d.error & 2) ? RH_E_INVALID : RH_OK); o.reserved = 0;
      o.bfmi = s->cfg.sampler == RH_SAMPLER_NUTS ? std::nan("") : d.e_trans2 / d.e_raw;
    }
    if (mass_diag) {
      // M's position among the state image's vectors comes from the device code itself (rh_state_mass_vec)
      const int n = (int)s->m->prog.n_params, slots = (n + 63) / 64, W = s->state_words;
      const size_t width = (size_t)slots * 64 * sizeof(uint64_t);
      std::vector<uint64_t> img((size_t)slots * 64 * s->chains);
      const char *base = (const char *)s->d_state + (size_t)s->m->mass_vec * slots * 64 * sizeof(uint64_t);
      HIPCHK(hipMemcpy2D(img.data(), width, base, (size_t)W * sizeof(uint64_t), width, (size_t)s->chains, hipMemcpyDeviceToHost));
      for (int c = 0; c < s->chains; c++)
        for (int i = 0; i < n; i++) std::memcpy(&mass_diag[(size_t)c * n + i], &img[(size_t)c * slots * 64 + i], sizeof(double));
    }
  });
  if (rc == RH_OK && any_lookup) { s->m->err = g_err = "Lookup index out of range during sampling"; return RH_E_LOOKUP; }
  if (rc == RH_OK && any_zero_mass) {
    s->m->err = g_err = "requirement failed: an adapted mass matrix has a zero element (MassMatrix.scala:8,16) -- a chain did not move during a window";
    return RH_E_INVALID;
  }
  return rc;
}
extern "C" int rh_sampler_mass_dense(rh_sampler *s, double *out) {
  if (!s || !out) { g_err = "rh_sampler_mass_dense: NULL"; return RH_E_INVALID; }
  if (s->cfg.mass_tuner != RH_MASS_DENSE_WINDOWED) { g_err = "rh_sampler_mass_dense: the sampler has no dense mass matrix"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(s->m->mu);
  return guard(s->m, [&] {
    HIPCHK(hipSetDevice(s->m->device));
    // row i of DenseMassMatrix.elements lives in lane i: word (dense_off + j) * 64 + i holds M[i][j]
    const int n = (int)s->m->prog.n_params;
    std::vector<uint64_t> img((size_t)n * 64 * s->chains);
    const char *base = (const char *)s->d_state + (size_t)s->dense_off * 64 * sizeof(uint64_t);
    HIPCHK(hipMemcpy2D(img.data(), (size_t)n * 64 * 8, base, (size_t)s->state_words * sizeof(uint64_t), (size_t)n * 64 * 8, (size_t)s->chains, hipMemcpyDeviceToHost));
    for (int c = 0; c < s->chains; c++)
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) std::memcpy(&out[((size_t)c * n + i) * n + j], &img[((size_t)c * n + j) * 64 + i], sizeof(double));
  });
}
// comm.cpp: device, stream and size (in doubles) of a sampler's draws buffer; the calling thread's error string
extern "C" int rh_sampler_geometry_(rh_sampler *s, int *device, void **stream, int64_t *doubles) {
  if (!s || !s->m) return RH_E_INVALID;
  if (device) *device = s->m->device;
  if (stream) *stream = (void *)s->m->stream;
  if (doubles) *doubles = (int64_t)s->chains * (int64_t)s->cfg.iterations * (int64_t)s->m->prog.n_params;
  return RH_OK;
}
extern "C" void rh_set_thread_error_(const char *msg) { g_err = msg ? msg : ""; }

// which feed the sampler's gradient launches take: 0 = they are not the lane walk's, 1 = the model's columns, 2 = the interleaved copy
extern "C" int rh_sampler_lane_feed(const rh_sampler *s) {
  if (!s) { g_err = "rh_sampler_lane_feed: NULL"; return -RH_E_INVALID; }
  return !s->lane_walk ? 0 : (s->lane_rows ? 2 : 1);
}
extern "C" int rh_sampler_progress(const rh_sampler *s, int32_t *warmed, int32_t *iterations_done) {
  if (!s) { g_err = "rh_sampler_progress: NULL"; return RH_E_INVALID; }
  if (warmed) *warmed = s->warmed ? 1 : 0;
  if (iterations_done) *iterations_done = s->it_done;
  return RH_OK;
}
extern "C" int rh_sampler_timing(rh_sampler *s, rh_timing *out, int reset) {
  if (!s || !out) { g_err = "rh_sampler_timing: NULL"; return RH_E_INVALID; }
  std::lock_guard<std::mutex> lk(s->m->mu);
  return guard(s->m, [&] {
    fetch_stats(s);
    resolve_round(s);   // (the last round of the last advance: nothing followed it that could have hidden the read-out)
    int64_t grads = 0;
    for (auto &d : s->last_stats) grads += d.gradient_evaluations;
    std::memset(out, 0, sizeof(*out));
    out->kernel_ms = s->kernel_ms; out->total_ms = s->total_ms; out->launches = s->launches;
    out->density_evals = grads - s->grads_at_reset;
    out->row_chain_evals = out->density_evals * s->m->rows_total;
    std::snprintf(out->dominant_kernel, sizeof out->dominant_kernel, s->tick_engine ? (s->m->info.gather_mode ? "rh_grad_gather_kernel" : s->m->k_grad_glm ? "rh_grad_glm_kernel" : s->lane_walk ? "rh_grad_lane_kernel" : (s->fuse && s->warmed && s->cfg.hmc_steps > 1) ? "rh_grad_fused_kernel" : "rh_grad_kernel") : "rh_chain_kernel");
    out->chain_slots = s->tick_engine ? s->chain_slots : out->density_evals;
    out->steady_kernel_ms = s->steady_ms; out->steady_launches = s->steady_launches; out->steady_density_evals = s->steady_evals;
    if (reset) { s->kernel_ms = 0; s->total_ms = 0; s->launches = 0; s->grads_at_reset = grads; s->chain_slots = 0; s->steady_ms = 0; s->steady_launches = 0; s->steady_evals = 0; }
  });
}

extern "C" int rh_sample(rh_model *m, const rh_config *cfg, const int64_t *seeds, int32_t chains, double *draws,
                         double *mass_diag, rh_chain_stats *stats) {
  rh_sampler *s = nullptr;
  int rc = rh_sampler_create(m, cfg, seeds, chains, &s);
  if (rc != RH_OK) return rc;
  rc = rh_sampler_warmup(s);
  if (rc == RH_OK) rc = rh_sampler_run(s, cfg->iterations);
  if (rc == RH_OK && draws && cfg->iterations > 0) rc = rh_sampler_draws(s, 0, cfg->iterations, draws);
  if (rc == RH_OK) rc = rh_sampler_stats(s, stats, mass_diag);
  rh_sampler_destroy(s);
  return rc;
}

// Model.sample's loop over chains (core/Model.scala:16-22) fanned out over several devices: one host thread per shard,
// shard g owns the global chains [g*C/G, (g+1)*C/G) (remainder to the first shards), seeds / draws / stats / mass are
// simply the caller's arrays at the shard's chain offset, so the result does not depend on how the chains were cut.
// No device-to-device traffic: chains never interact (sampler/Driver.scala:13-17); the caller's host buffer is the gather.
extern "C" int rh_sample_multi(rh_model *const *models, int32_t n_models, const rh_config *cfg, const int64_t *seeds,
                               int32_t chains, double *draws, double *mass_diag, rh_chain_stats *stats) {
  if (!models || n_models <= 0 || !cfg || !seeds || chains <= 0) { g_err = "rh_sample_multi: bad arguments"; return RH_E_INVALID; }
  if (cfg->struct_size != (int32_t)sizeof(rh_config)) { g_err = "rh_config.struct_size mismatch"; return RH_E_INVALID; }   // before *cfg is copied per shard
  const int nv = models[0] ? rh_model_nvars(models[0]) : -1;
  for (int g = 0; g < n_models; g++) {
    if (!models[g] || !models[g]->loaded) { g_err = "rh_sample_multi: model " + std::to_string(g) + " not loaded"; return RH_E_INVALID; }
    if (rh_model_nvars(models[g]) != nv) { g_err = "rh_sample_multi: the models differ (nvars)"; return RH_E_INVALID; }
  }
  const int G = std::min<int>(n_models, chains);
  // the tick engine's row-split count is derived from the chain count; fix it from the TOTAL here so that every shard sums its
  // rows in the same order as the unsharded call would (bit-identical draws for every shard count)
  int splits_all = cfg->grad_splits;
  // ... and so is the walk: the lane walk only where every shard's model has the kernel (a mixed node may not), decided here once
  bool lane_all = models[0]->n_row_targets > 0;
  for (int g = 0; g < G && lane_all; g++) lane_all = walk_is_lane(models[g], cfg->sampler == RH_SAMPLER_HMC, chains);
  if (splits_all <= 0 && models[0]->n_row_targets > 0) splits_all = lane_all ? lane_nsplit(models[0], chains) : default_nsplit(models[0], chains);
  std::vector<int> first((size_t)G + 1, 0);
  for (int g = 0; g < G; g++) first[(size_t)g + 1] = first[(size_t)g] + chains / G + (g < chains % G ? 1 : 0);
  std::vector<int> rcs((size_t)G, RH_OK);
  std::vector<std::string> errs((size_t)G);
  std::vector<std::thread> th;
  for (int g = 0; g < G; g++)
    th.emplace_back([&, g] {
      const int c0 = first[(size_t)g], nc = first[(size_t)g + 1] - c0;
      rh_config c = *cfg;
      c.grad_splits = splits_all;
      if (cfg->rng_next_gaussian) c.rng_next_gaussian = cfg->rng_next_gaussian + c0;
      const size_t per_chain = (size_t)cfg->iterations * (size_t)nv;
      g_total_chains = chains; g_shard_walk = lane_all ? 1 : 0;   // (this shard thread's: walk and splits are the whole sampler's)
      rcs[(size_t)g] = rh_sample(models[g], &c, seeds + c0, nc, draws ? draws + (size_t)c0 * per_chain : nullptr,
                                 mass_diag ? mass_diag + (size_t)c0 * nv : nullptr, stats ? stats + c0 : nullptr);
      g_total_chains = 0; g_shard_walk = -1;
      if (rcs[(size_t)g] != RH_OK) errs[(size_t)g] = rh_last_error(models[g]);
    });
  for (auto &t : th) t.join();
  for (int g = 0; g < G; g++)
    if (rcs[(size_t)g] != RH_OK) { g_err = "shard " + std::to_string(g) + ": " + errs[(size_t)g]; return rcs[(size_t)g]; }
  return RH_OK;
}
