/* rainier_hip.h -- C ABI of the MI355X-native HMC engine that drops in behind Rainier's
 * model.sample().  Plain pointers and sizes only; no C++/torch types.  A JVM reaches it through
 * the thin JNI shim in rainier_amd/jni/ (see INTEGRATION.md for the Scala-side binding).
 *
 * Each entry point replaces one reference seam (paths under /root/reference):
 *
 *   rh_model_create     <- Compiler.compileTargets(group): ir.DataFunction
 *                          rainier-compute/src/main/scala/com/stripe/rainier/compute/Compiler.scala:14-30
 *                          (the ASM bytecode back end ir/CompiledFunction.scala:42-120 is what is replaced:
 *                           RIR is lowered once per model to a fused fp64 HIP gradient kernel)
 *   rh_density_eval     <- trait DensityFunction { nVars; update(vars); density; gradient(i) }
 *                          rainier-sampler/src/main/scala/com/stripe/rainier/sampler/DensityFunction.scala:3-8
 *                          as built by Model.density()  rainier-core/.../core/Model.scala:38-50  (batched over chains)
 *   rh_sample           <- Driver.sample(chain, config, density, progress)(rng)
 *                          rainier-sampler/.../sampler/Driver.scala:7-46, called once per chain by
 *                          Model.sample  rainier-core/.../core/Model.scala:13-24   (here: one call, all chains)
 *   rh_config           <- SamplerConfig + the concrete plugin classes
 *                          sampler/Sampler.scala:3-62, HMC.scala:3-33, EHMC.scala:3-74, DualAvg.scala:3-25,
 *                          MassMatrix.scala:120-173
 *   rh_diagnostics      <- Trace.diagnostics  rainier-core/.../core/Trace.scala:11-21,52-120
 *
 * Errors: every function returns an int status (RH_OK == 0); nothing throws or aborts across the
 * ABI.  NaN log-density is data, not an error (LeapFrog.scala:138-142: the proposal is rejected).
 * An out-of-range Lookup index (the reference's generated NullPointerException,
 * ir/MethodGenerator.scala:164-167) is reported as RH_E_LOOKUP after the launch.
 */
#ifndef RAINIER_HIP_H
#define RAINIER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RH_ABI_VERSION 6  /* 2: rh_chain_stats.bfmi, rh_config.rng_next_gaussian, rh_optimize, rh_sampler_progress / mass_dense;
                             3: rh_density_eval_ex, rh_sample_multi, rh_comm_* (RCCL all-gather of the draws);
                             4: rh_model_clone;
                             5: rh_model_engines, rh_compile_count;
                             6: rh_timing.chain_slots / steady_* (the tick engine's gradient launches serve the live chains only);
                                (still 6, additions only: rh_sampler_diagnostics, rh_diagnostics_device, rh_predict_*, rh_*_summary*, rh_generate_*,
                                 rh_sampler_generate, rh_sampler_covariance, rh_covariance_device, rh_covariance_lower_only,
                                 rh_sampler_histogram, rh_histogram_device, rh_sampler_histogram2d, rh_histogram2d_device, rh_histogram_lower_only,
                                 rh_sampler_rank_diagnostics, rh_rank_diagnostics_device, rh_rank_lower_only,
                                 rh_sampler_mcse, rh_mcse_device, rh_mcse_lower_only,
                                 rh_loo_device, rh_sampler_loo, rh_loo_lower_only,
                                 rh_loo_expect_device, rh_sampler_loo_expect, rh_loo_expect_lower_only,
                                 rh_loo_quantile_device, rh_sampler_loo_quantile, rh_loo_quantile_lower_only) */

enum rh_status {
  RH_OK = 0,
  RH_E_INVALID = 1,   /* bad argument / malformed RIR (IllegalArgumentException) */
  RH_E_COMPILE = 2,   /* lowering or hiprtc failed */
  RH_E_DEVICE = 3,    /* HIP runtime error / no usable device */
  RH_E_LOOKUP = 4,    /* Lookup index outside [low, low+size) during evaluation */
  RH_E_UNSUPPORTED = 5
};

typedef struct rh_model rh_model;     /* compiled model + device-resident observation columns */
typedef struct rh_sampler rh_sampler; /* device-resident state of `chains` independent chains */

/* ---- seam 1: compile ------------------------------------------------------------------------ */

enum rh_math_mode {
  RH_MATH_FAST = 0,   /* exp/log nodes -> ROCm device libm / the prelude's fast log, <= 1 ulp measured, like java.lang.Math's bound; the other
                         device math functions measure 0.69-0.85 ulp except tan 1.07, atan 1.32, pow 1.29: inside the
                         stated fp64 tolerance, above java.lang.Math's 1-ulp specification */
  RH_MATH_STRICT = 1  /* exp/log nodes -> fdlibm (java.lang.StrictMath): bit-reproducible across machines */
};

typedef struct rh_compile_opts {
  int32_t struct_size;   /* = sizeof(rh_compile_opts) */
  int32_t device;        /* HIP device ordinal; -1 = current device */
  int32_t math_mode;     /* rh_math_mode */
  int32_t fp_contract;   /* 0 = never fuse a*b+c in model code (JVM semantics, default); 1 = allow FMA */
  /* The three shape fields are UPPER BOUNDS: the engine lowers a model again with a smaller value while a kernel of the requested
     shape is not fit to run on this toolchain (spilled registers / vector code ahead of a join's exec restore: rh_model_engines),
     so a caller never gets a kernel the engine would not launch; the generated source (rh_model_hip_source) says what was built. */
  int32_t rows_unroll;   /* row-loop unroll factor of the chain-per-wavefront kernel; 0 = engine default */
  int32_t grad_chains;   /* tick engine: chains that share one pass over the rows per wavefront; 0 = default (4) */
  int32_t grad_unroll;   /* tick engine: row-loop unroll; 0 = default (2) */
  int32_t factor_outputs; /* 1 = accumulate basis terms t and apply alpha*sum(t) + nrows*beta once per gradient, for outputs of
                            the form alpha*t + beta with alpha, beta parameter-only (changes rounding only; default 0) */
  int32_t with_nuts;      /* sampler-kernel variants to compile now instead of lazily on first use -- bit 0: NUTS, bit 1: dense
                             mass matrix, bit 2: one chain per wavefront for a model whose chains are packed (data-free
                             models; used for EHMC / NUTS below 4096 chains) */
  int32_t reserved;
} rh_compile_opts;

/* rir/rir_len      : RIR blob (include/rainier_hip_rir.h).
 * columns          : host pointers to the observation columns, flattened target by target then column
 *                    by column (DataFunction.data(target)(col), ir/DataFunction.scala:13-16), each nrows[target] long.
 * nrows            : one entry per target (ignored for targets without columns).
 * The engine copies the columns to HBM; the caller keeps ownership of its arrays. */
int rh_model_create(const void *rir, size_t rir_len, const double *const *columns, const int64_t *nrows,
                    const rh_compile_opts *opts, rh_model **out);
/* The same model on another device of this process -- what Model.sample's loop over chains (core/Model.scala:16-22) needs when
 * the chains are spread over several GPUs (rh_sample_multi): the lowered program and its code object are reused as they are
 * (no parsing, no data-dependent passes, no compilation unless the architectures differ) and the observation columns are
 * copied device to device over xGMI; the host arrays rh_model_create was given are not needed again.  device = -1: the
 * current device (a second, independent handle on the same device). */
int rh_model_clone(const rh_model *src, int32_t device, rh_model **out);
void rh_model_destroy(rh_model *m);
int rh_model_nvars(const rh_model *m);
/* the generated HIP source (the analogue of rainier-decompile's view of the generated bytecode) */
const char *rh_model_hip_source(const rh_model *m);
/* Which of the model's engines can run, and why not.  Before a kernel is launched its code object is inspected (no spilled vector
 * registers; no vector instruction ahead of a control-flow join's exec restore -- a fault of the ROCm 7.2 register allocator that
 * produced silent wrong sums) and, at creation, checked against another kernel of the same model on the device.  A
 * kernel that fails is replaced by a lighter build or by the other engine (RH_ENGINE_AUTO); an explicit request for an engine
 * that is out of use returns RH_E_UNSUPPORTED.  The reference has no counterpart: its back end splits any method that is too
 * heavy (ir/Packer.scala:10-71) instead of meeting a register file.
 * *chain_engine / *tick_engine / *density: 1 = usable (rh_sample with that engine / rh_density_eval); why: the reasons of the
 * unusable ones, text (may be NULL); compile_attempts: code objects built or fetched while lowering this model. */
int rh_model_engines(const rh_model *m, int32_t *chain_engine, int32_t *tick_engine, int32_t *density, int32_t *compile_attempts,
                     char *why, size_t why_cap);
/* hiprtc compilations this process has performed so far (kernel-cache misses; model creation costs seconds each) */
int64_t rh_compile_count(void);
/* last error message: of this model, or of the calling thread when m == NULL */
const char *rh_last_error(const rh_model *m);

/* ---- seam 2: DensityFunction, batched --------------------------------------------------------
 * q [chains][nvars] -> logp [chains], grad [chains][nvars] (host pointers).  Stateless, one call at a
 * time per model.  chains = 1 restores the reference trait exactly. */
int rh_density_eval(rh_model *m, const double *q, int32_t chains, double *logp, double *grad);
/* The same seam with the evaluation path chosen by the caller (rh_engine_kind, declared below):
 *   RH_ENGINE_CHAIN : one chain per wavefront streams every row itself (rh_density_kernel; what rh_density_eval does for
 *                     models without a parameter table)
 *   RH_ENGINE_TICK  : the sampler's batched gradient path -- the row-streaming gradient kernel the model was lowered to
 *                     (rh_grad_kernel | rh_grad_glm_kernel | rh_grad_gather_kernel) over `grad_splits` row splits (0 = the
 *                     sampler's default) followed by the fixed-order combine of rh_tick_kernel
 *   RH_ENGINE_AUTO  : rh_density_eval's choice.
 * Results of the two paths agree to rounding (different summation order); both are DensityFunction.update batched. */
int rh_density_eval_ex(rh_model *m, const double *q, int32_t chains, int32_t engine, int32_t grad_splits, double *logp,
                       double *grad);

/* ---- seam 3: SamplerConfig / Driver.sample ---------------------------------------------------- */

/* RH_ENGINE_CHAIN: one chain per wavefront, the whole Driver loop in one persistent kernel (best for models with
 *                  little or no data: cfg 1, cfg 3).
 * RH_ENGINE_TICK : per leapfrog step one batched gradient launch shared by all chains (rows read once per group of
 *                  chains) + one small per-chain automaton launch (best for data-heavy models: cfg 2, 4).
 * RH_ENGINE_AUTO : TICK when the model streams >= 65536 rows, else CHAIN. */
enum rh_engine_kind { RH_ENGINE_AUTO = 0, RH_ENGINE_CHAIN = 1, RH_ENGINE_TICK = 2 };
/* RH_SAMPLER_NUTS is an EXTENSION (the reference has no NUTS): iterative multinomial NUTS
 * (Phan, Pradhan, Jankowiak 2019, App. A) behind the same Sampler plugin point (sampler/Sampler.scala:52-62). */
enum rh_sampler_kind { RH_SAMPLER_HMC = 0, RH_SAMPLER_EHMC = 1, RH_SAMPLER_NUTS = 2 };
enum rh_step_kind { RH_STEP_DUALAVG = 0, RH_STEP_STATIC = 1 };
/* RH_MASS_DENSE_WINDOWED = DenseMassMatrixTuner(initialWindowSize, windowExpansion, skipFirst, skipLast)
 * (sampler/MassMatrix.scala:175-181, CovarianceEstimator + packed Cholesky :15-117); at most 64 parameters. */
enum rh_mass_kind { RH_MASS_IDENTITY = 0, RH_MASS_DIAG_WINDOWED = 1, RH_MASS_STATIC_DIAG = 2, RH_MASS_DENSE_WINDOWED = 3 };

typedef struct rh_config {
  int32_t struct_size;     /* = sizeof(rh_config) */
  int32_t iterations;      /* SamplerConfig.iterations        (DefaultConfig: 1000) */
  int32_t warmup;          /* SamplerConfig.warmupIterations  (DefaultConfig: 1000) */
  int32_t sampler;         /* rh_sampler_kind */
  int32_t hmc_steps;       /* HMCSampler(nSteps) */
  int32_t ehmc_max_steps;  /* EHMCSampler(maxSteps, minSteps = 1, bufSize = 100, pCount = 0.1) */
  int32_t ehmc_min_steps;
  int32_t ehmc_buf_size;   /* <= 256 */
  double ehmc_p_count;
  int32_t step_tuner;      /* rh_step_kind */
  int32_t mass_tuner;      /* rh_mass_kind */
  double dualavg_delta;    /* DualAvgTuner(delta) */
  double static_step;      /* StaticStepSize(stepSize) */
  int32_t mass_init_window; /* DiagonalMassMatrixTuner(initialWindowSize, windowExpansion, skipFirst, skipLast) */
  int32_t mass_skip_first;
  int32_t mass_skip_last;
  int32_t nuts_max_depth;  /* RH_SAMPLER_NUTS: maximum tree depth, 1..12 (10 in BASELINE configs 3-5) */
  double mass_expansion;
  const double *static_mass; /* [nvars] DiagonalMassMatrix.elements for RH_MASS_STATIC_DIAG (host pointer) */
  int32_t engine;          /* rh_engine_kind: how the chains are mapped onto the device (results agree to rounding) */
  int32_t grad_splits;     /* tick engine: row splits per chain group; 0 = engine default */
  /* Continuing an existing ScalaRNG / java.util.Random stream (Driver.sample takes the caller's rng, sampler/Driver.scala:7-11;
   * the SBC goldsets sample from the stream that generated the synthetic data): pass seeds[c] = internalState ^ 0x5DEECE66D
   * and here the stream's pending nextNextGaussian per chain ([chains] doubles, NaN = none pending).  NULL: fresh streams. */
  const double *rng_next_gaussian;
  int64_t reserved[2];
} rh_config;

/* Fills DefaultConfig (sampler/Sampler.scala:17-27): 1000/1000, DualAvgTuner(0.8),
 * DiagonalMassMatrixTuner(50, 1.5, 50, 50), EHMCSampler(1024). */
void rh_config_default(rh_config *cfg);

typedef struct rh_chain_stats {
  int64_t leapfrog_steps;        /* distinct (p,q) updates in the sampling phase */
  int64_t warmup_leapfrog_steps;
  int64_t gradient_evaluations;  /* density evaluations the engine performed (sampling phase) */
  int64_t accepted;              /* sampling phase */
  double mean_accept_prob;       /* sampling-phase mean of exp(logAcceptanceProb) */
  double step_size;              /* stepSizeTuner.stepSize used for sampling */
  int32_t error;                 /* rh_status of this chain (RH_E_LOOKUP ...) */
  int32_t reserved;
  double bfmi;                   /* Stats.bfmi = energyTransitions2 / energyVariance.raw(0) over the sampling phase
                                    (sampler/Stats.scala:14-16, LeapFrog.scala:68-74; HMC and EHMC; NaN for NUTS) */
} rh_chain_stats;

/* One call = Model.sample's loop over chains, run concurrently on the device.
 * seeds [chains]     : chain c behaves as the reference run with ScalaRNG(seeds[c]) and nChains = 1.
 * draws [chains][iterations][nvars], mass_diag [chains][nvars] (1.0 = identity), stats [chains]: host
 * pointers, caller-allocated; mass_diag and stats may be NULL. */
int rh_sample(rh_model *m, const rh_config *cfg, const int64_t *seeds, int32_t chains, double *draws,
              double *mass_diag, rh_chain_stats *stats);

/* Multi-GPU Model.sample: the chains are cut into n_models contiguous shards, shard g = global chains
 * [g*chains/n_models, ...) runs on models[g] -- the SAME program and data compiled once per device (rh_model_create with
 * rh_compile_opts.device = g), driven by one host thread per shard.  seeds / draws / mass_diag / stats are indexed by GLOBAL
 * chain id exactly as in rh_sample, so the result is identical for every n_models (chains never interact:
 * sampler/Driver.scala:13-17); there is no device-to-device traffic, the caller's host buffer is the gather.
 * (bench.py's one-process-per-GPU launch uses rh_sampler_* per rank and one RCCL all-gather of the device-resident draws
 * instead; both forms shard by global chain id.)  Replaces the loop  core/Model.scala:16-22. */
int rh_sample_multi(rh_model *const *models, int32_t n_models, const rh_config *cfg, const int64_t *seeds, int32_t chains,
                    double *draws, double *mass_diag, rh_chain_stats *stats);

/* Multi-PROCESS multi-GPU (one process per device -- what `torch.distributed.run`, MPI or one JVM per GPU give): every
 * rank samples its own shard of the chains (seeds by GLOBAL chain id; no collective on the data path) with rh_sampler_* and
 * the device-resident draws are gathered ONCE with an RCCL all-gather over xGMI.  RCCL is loaded with dlopen on first use;
 * without it these calls return RH_E_UNSUPPORTED.  Bootstrap: rank 0 calls rh_comm_unique_id and hands the 128 bytes to the
 * other ranks by whatever channel the host program has; all ranks then call rh_comm_create (collective). */
#define RH_COMM_ID_BYTES 128
typedef struct rh_comm rh_comm;
int rh_comm_unique_id(unsigned char id[RH_COMM_ID_BYTES]);
int rh_comm_create(const unsigned char id[RH_COMM_ID_BYTES], int32_t world, int32_t rank, int32_t device, rh_comm **out);
void rh_comm_destroy(rh_comm *c);
/* collective: gathers every rank's draws ([chains][iterations][nvars], equal on all ranks) into [world * chains][...],
 * rank-major == global chain id order.  host_out (may be NULL): caller-allocated host buffer; *dev_out (may be NULL): device
 * pointer of the gathered buffer, owned by the communicator (valid until the next gather or rh_comm_destroy). */
int rh_comm_allgather_draws(rh_comm *c, rh_sampler *s, double *host_out, void **dev_out);
/* collective: *value = max over ranks (the timing reduction of a benchmark; doubles as a device-side barrier) */
int rh_comm_allreduce_max(rh_comm *c, double *value);
/* hipDeviceSynchronize on `device` (for hosts that never touch the HIP runtime themselves) */
int rh_device_synchronize(int32_t device);

/* The same, split so that a caller can keep draws on the device, poll progress (sampler/Progress.scala)
 * and time phases.  Typical use: create -> warmup -> run(iterations) -> read stats -> destroy. */
int rh_sampler_create(rh_model *m, const rh_config *cfg, const int64_t *seeds, int32_t chains, rh_sampler **out);
void rh_sampler_destroy(rh_sampler *s);
/* advance every chain through LeapFrog.initialize, the step-size search and all warmup iterations */
int rh_sampler_warmup(rh_sampler *s);
/* advance every chain by n sampling iterations (n <= iterations remaining) */
int rh_sampler_run(rh_sampler *s, int32_t n);
/* copy draws of iterations [first, first+count) to the host: out [chains][count][nvars] */
int rh_sampler_draws(rh_sampler *s, int32_t first, int32_t count, double *out);
/* device pointer to all draws, layout [chains][iterations][nvars] (valid until destroy) */
int rh_sampler_draws_device(rh_sampler *s, void **dev_ptr);
int rh_sampler_stats(rh_sampler *s, rh_chain_stats *stats /*[chains]*/, double *mass_diag /*[chains][nvars] or NULL*/);
/* RH_MASS_DENSE_WINDOWED only: the final DenseMassMatrix.elements of every chain, out [chains][nvars][nvars] */
int rh_sampler_mass_dense(rh_sampler *s, double *out);

typedef struct rh_timing {
  double kernel_ms;          /* device time of the DOMINANT kernel's launches since the last reset (HIP events
                                recorded on the engine's own stream around each launch) */
  double total_ms;           /* device time of all of the engine's launches in the same interval */
  int64_t launches;          /* launches of the dominant kernel */
  int64_t density_evals;     /* chain-level density evaluations in those launches */
  int64_t row_chain_evals;   /* rows streamed x chains: the unit of SURVEY.md 8(d) */
  char dominant_kernel[64];  /* name of the kernel that accounts for kernel_ms */
  /* The tick engine's gradient launches serve the chains that wait for a gradient (under EHMCSampler -- DefaultConfig's,
   * sampler/Sampler.scala:17-27 -- and NUTS the chains' trajectories end at different launches).  chain_slots: the chains listed for
   * those launches, summed (= density_evals when no launch served a chain that did not need it; launches x chains without
   * compaction).  steady_*: the same three figures restricted to the launches that served >= 90 % of the sampler's chains -- the
   * dominant kernel at full occupancy, the tail of a run (few chains left) excluded.  Chain engine: chain_slots = density_evals, steady_* = 0. */
  int64_t chain_slots;
  double steady_kernel_ms;
  int64_t steady_launches;
  int64_t steady_density_evals;
} rh_timing;
int rh_sampler_timing(rh_sampler *s, rh_timing *out, int reset);
/* Progress polling instead of a callback into the caller (Driver.sample's `progress: Progress` argument,
 * sampler/Driver.scala:7-11, sampler/Progress.scala): how far the chains of this handle have been driven.
 * warmed: 1 once the warm-up phase is complete; iterations_done: sampling iterations completed (of cfg.iterations). */
int rh_sampler_progress(const rh_sampler *s, int32_t *warmed, int32_t *iterations_done);
/* the feed of the sampler's gradient launches: 0 = not the lane walk, 1 = the lane walk over the model's columns, 2 = over the
   interleaved copy of the columns (csrc/device/rh_lane.hip.h); negative = error */
int rh_sampler_lane_feed(const rh_sampler *s);

/* ---- after the path: Generator.prepare / Trace.predict (next-row f3) -----------------------------------------------
 * The reference compiles a generator's `requirements` with Compiler.default.compile(parameters, namedReqs) and evaluates
 * them once per draw on the JVM (rainier-core/.../core/Generator.scala:59-94, core/Trace.scala:34-41).  Here the same
 * program is evaluated for every draw on the device, one thread per draw.
 * rir: a "requirements program" = an RIR blob whose header `reserved` word is 1 and whose targets are data-free, one per
 * requirement, with outputs[0] = the requirement (the other outputs are ignored).
 * draws [ndraws][nvars] (host) -> out [ndraws][n_requirements] (host). */
int rh_requirements_eval(const void *rir, size_t rir_len, const rh_compile_opts *opts, const double *draws,
                         int64_t ndraws, double *out);

/* ---- Model.optimize / Optimizer.lbfgs ---------------------------------------------------------------
 * Optimizer.lbfgs(df: DensityFunction): Array[Double]   rainier-sampler/.../optimizer/Optimizer.scala:6-24
 *   (L-BFGS m = 5, eps = 0.1 on f = -density; LBFGS.java:44-632), called by Model.optimize (core/Model.scala:26-30).
 * Batched over independent starting points: x0 [starts][nvars] or NULL (all zeros = the reference's start); every round
 * is one batched device density launch for the starts still searching; the O(m n) vector updates stay on the host.
 * x_out [starts][nvars]; evals_out / status_out [starts] may be NULL.  max_evals <= 0: unlimited (the reference's loop).
 * status_out: RH_OPT_CONVERGED, RH_OPT_NOT_DESCENT (where the reference throws RuntimeException("dginit")),
 * RH_OPT_MAX_EVALS. */
enum rh_opt_status { RH_OPT_CONVERGED = 0, RH_OPT_NOT_DESCENT = 1, RH_OPT_MAX_EVALS = 2 };
int rh_optimize(rh_model *m, const double *x0, int32_t starts, int32_t max_evals, double *x_out, int32_t *evals_out,
                int32_t *status_out);

/* ---- Trace.diagnostics --------------------------------------------------------------------------
 * draws [chains][iterations][nvars] (host) -> rhat [nvars], ess [nvars]   (core/Trace.scala:52-120)
 * One host thread over a host copy: for draws that live on the device use the device form below, which does not move them. */
int rh_diagnostics(const double *draws, int32_t chains, int32_t iterations, int32_t nvars, double *rhat, double *ess);
/* Trace.diagnostics (+ the pooled mean and Trace's v) over iterations [first, first+count) of the sampler's own draws,
 * computed on the device; rhat/ess [nvars]; mean/var [nvars] or NULL.  count <= iterations completed - first.
 * mean = meanMean, var = v of Trace.scala:69,85: sqrt(var / ess) is the Monte-Carlo standard error of the pooled mean.
 * Fixed-order sums: the same window gives the same bits on every call, and the bits of a copy of its rows.  The launches go
 * to the sampler's stream behind its pending work and are not part of rh_timing.  Without a device: RH_E_DEVICE. */
int rh_sampler_diagnostics(rh_sampler *s, int32_t first, int32_t count, double *rhat, double *ess, double *mean, double *var);
/* the same over any device buffer of layout [chains][iterations][nvars] on `device` (-1: the current one), e.g.
 * rh_comm_allgather_draws' *dev_out */
int rh_diagnostics_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars,
                          int32_t first, int32_t count, double *rhat, double *ess, double *mean, double *var);

/* ---- Trace.predict / Trace.thin over device-resident draws (core/Trace.scala:23-41, core/Generator.scala:59-94) ----
 * rh_requirements_eval above takes host draws and compiles on every call.  A predictor is the same requirements program
 * (header kind 1) compiled ONCE for one device -- through the kernel cache, and judged like a model's kernels before it may be
 * launched (no spilled registers, no scratch, the static code check): a program whose kernels fail returns RH_E_UNSUPPORTED
 * with the reason -- and evaluated where the draws are (csrc/device/rh_predict.hip.h).
 * Window and thinning: the kept iterations are first + j*thin, j = 0 .. ceil(count/thin)-1 (Trace.thin keeps i % n == 0,
 * applied to the window); first >= 0, count >= 1, thin >= 1, first + count <= iterations (completed, for a sampler).
 * Result layout [chains][kept][nreq] -- the layout rh_diagnostics_device reads, so R-hat / ESS of a prediction is one more call
 * on *dev_out.  host_out (may be NULL): caller-allocated; *dev_out (may be NULL): the handle's own device buffer, valid until
 * the next predict call on this handle or rh_predict_destroy.  Later calls compile nothing.  With fp_contract = 0 every value
 * has the bits rh_requirements_eval gives for the same row and opts.  An out-of-range Lookup: RH_E_LOOKUP.  No device:
 * RH_E_DEVICE (no CPU fallback).  Handle, sampler or buffer on different devices, a broken window, another nvars: RH_E_INVALID. */
typedef struct rh_predict rh_predict;
int rh_predict_create(const void *rir, size_t rir_len, const rh_compile_opts *opts, rh_predict **out);
void rh_predict_destroy(rh_predict *p);
int rh_predict_nreq(const rh_predict *p);
int rh_predict_nvars(const rh_predict *p);
/* over the sampler's own draws, on its stream behind its pending work; not part of rh_timing; the chains are not altered */
int rh_sampler_predict(rh_sampler *s, rh_predict *p, int32_t first, int32_t count, int32_t thin, double *host_out, void **dev_out);
/* over any device buffer [chains][iterations][nvars] on `device` (-1: the handle's), e.g. rh_comm_allgather_draws' *dev_out;
 * synchronises the device before and after */
int rh_predict_device(rh_predict *p, const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars,
                      int32_t first, int32_t count, int32_t thin, double *host_out, void **dev_out);

/* ---- posterior summaries over device-resident draws: precis / hdpi (rainier-notebook package.scala:327-342, 367-418, 456-469) ----
 * The pooled column of parameter p: x[c][first + j*thin][p], chain-major, j = 0 .. kept-1, kept = ceil(count/thin) (the window
 * and thinning rule of rh_sampler_predict); N = chains * kept.  Every figure reads the column SORTED in java.lang.Double.compare's
 * order (-0.0 before +0.0; every NaN, read as the positive quiet NaN, after +inf); it is sorted on the device
 * (csrc/device/rh_summary.hip.h) and never leaves it.
 *   quantiles[p][k] = sorted[min(N-1, (int64)floor((double)N * probs[k]))], 0 <= probs[k] <= 1, 1 <= nprobs <= 16
 *                     (precis: data(math.floor(data.size * 0.055).toInt)); the indices are computed on the host, in double.
 *   hdpi[p]         = for 0 < hdpi_prob <= 1 and idx = (int64)ceil(hdpi_prob * N): (sorted[0], sorted[N-1]) if idx == N, else the
 *                     pair (sorted[i], sorted[i+idx]) of the smallest width over i in [0, N-idx); widths compare in
 *                     Double.compare's order and the smallest i wins a tie (minBy's first minimum).  A column that holds a NaN
 *                     gives (NaN, NaN): the reference's answer there depends on its comparison order.  hdpi_prob <= 0: not asked
 *                     for, hdpi is not written.
 *   mean[p], sd[p]  = sum x / N and sqrt(sum (x - mean)^2 / N), the population form (computeParamStats), in two passes.
 * Sums run in a fixed order that depends on N alone: the same window gives the same bits on every call.  mean / sd [nvars],
 * quantiles [nvars][nprobs], hdpi [nvars][2]; each may be NULL.  The sort workspace is capped at 128 MiB (the parameters are
 * walked in chunks); a single column beyond it (2 * N * 8 bytes) returns RH_E_UNSUPPORTED.  A broken window, nprobs outside
 * 1 .. 16, a probability outside [0, 1] or hdpi_prob > 1: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).
 * The sampler form goes to the sampler's stream behind its pending work, is not part of rh_timing and does not alter the chains;
 * count <= iterations completed - first. */
int rh_sampler_summary(rh_sampler *s, int32_t first, int32_t count, int32_t thin, const double *probs, int32_t nprobs,
                       double hdpi_prob, double *mean, double *sd, double *quantiles, double *hdpi);
/* the same over any device buffer [chains][iterations][nvars] on `device` (-1: the current one), e.g. a predictor's *dev_out or
 * rh_comm_allgather_draws' *dev_out; synchronises the device before and after */
int rh_summary_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first,
                      int32_t count, int32_t thin, const double *probs, int32_t nprobs, double hdpi_prob, double *mean, double *sd,
                      double *quantiles, double *hdpi);

/* ---- posterior-predictive sampling over device-resident draws: Trace.predict of a Distribution ------------------------------
 * In the reference trace.predict(value) takes any ToGenerator -- a Real, but also a Distribution (core/Trace.scala:34-41,
 * core/Generator.scala:171-174): trace.predict(Normal(mu, sigma)) returns posterior-predictive samples, and SBC.synthesize is the
 * same machinery (core/SBC.scala:53-61).  rh_predict is the deterministic half (the compiled requirements); this is the sampling
 * half (csrc/device/rh_generate.hip.h): a model-independent kernel that turns a device buffer of per-draw distribution parameters
 * in [chains][kept][nin] into per-draw samples out [chains][kept][nout], the layout rh_summary_device / rh_diagnostics_device read.
 * A generator is a table of ops, given as data; output o of flat row r = c * kept + j is out[r * nout + o], nout = nops.
 * Every draw runs the reference's Generator.get(rng, evaluator) on a java.util.Random stream of its own: global draw index
 * d = chain0 * kept + r (unsigned 64-bit; chain0: the global id of the buffer's first chain, so that a shard of a multi-GPU run
 * draws what the whole run would), seed_d = splitmix64's finaliser of seed + (d + 1) * 0x9E3779B97F4A7C15, stream
 * new java.util.Random(seed_d).  The ops of a draw run left to right on that stream (Generator.zip / traverse,
 * Generator.scala:38-47, 145-150), the pending nextNextGaussian carried along.  The results do not depend on tiling or sharding.
 * java.lang.Math follows the oracle's JM_DET policy (fdlibm log / exp, IEEE sqrt; Gamma's Math.pow(u, 1 / a) is
 * exp((1 / a) * log(u))), so every family is bit-comparable.  u = standardUniform, g = standardNormal, * and + separate:
 *   RH_GEN_REAL      a             a                                            Generator.scala:119-122
 *   RH_GEN_NORMAL    loc, scale    g * scale + loc                              Continuous.scala:54-57, 63-67; Injection.scala:50-52, 70-72
 *   RH_GEN_CAUCHY    loc, scale    (g1 / g2) * scale + loc                      Continuous.scala:72-77
 *   RH_GEN_LAPLACE   loc, scale    x * scale + loc, x = (signum(u') * -1) * log(1 - 2 * abs(u')), u' = u - 0.5      :82-89
 *   RH_GEN_UNIFORM   loc, scale    u * scale + loc   (scale = to - from)        :202-215
 *   RH_GEN_LOGNORMAL loc, scale    exp(g * scale + loc)                         :194-197; Injection.scala:89-91
 *   RH_GEN_GAMMA     shape, scale  Marsaglia-Tsang with the a < 1 boost, * scale                                    :94-147
 *   RH_GEN_BETA      a, b          z1 / (z1 + z2), z1 = gamma(a) * 1.0, then z2 = gamma(b) * 1.0                    :163-176
 *   RH_GEN_BERNOULLI p             u <= p ? 1 : 0                               Discrete.scala:38-48
 *   RH_GEN_GEOMETRIC p             (double)(long)floor(log(u) / log(1 - p))     :59-69
 *   RH_GEN_POISSON   lambda        Poisson.small below 30, else Poisson.large   :122-186
 * (Exponential(rate) is RH_GEN_GAMMA(1.0, 1 / rate), Continuous.scala:152-158.)  .toLong is Java's d2l; every output is a double.
 * No parameter can make a loop endless: GAMMA / BETA need every shape finite and > 0 and POISSON lambda finite and >= 0, else the
 * output is NaN, the op draws nothing from the stream and the call reports RH_GEN_F_DOMAIN; every rejection loop stops after 4096
 * passes with NaN and RH_GEN_F_CAP.  The return code stays RH_OK when a flag is set: the NaNs mark the samples.
 *
 * The count families and the composites (csrc/device/rh_generate_ext.hip.h, a kernel of its own: a table that uses nothing of this
 * paragraph launches what it always launched).  rh_gen_op.reserved is a flags word and rh_gen_arg.pad a source; zeros mean what
 * they meant.
 *   reserved bits 0-7, the GUARD: 0 = the op always runs; j + 1 = it runs only in the draws whose SELECTOR is j.  The selector is
 *       the sample of the nearest earlier RH_GEN_CATEGORICAL op that ran in the same draw.  A skipped op draws nothing from the
 *       stream, raises no flag, and its value is the carry (below).  A NaN selector matches no guard.
 *   reserved bit 8, RH_GEN_OP_HIDDEN: the op's value is not stored.  nout is the number of VISIBLE ops; output column c is the
 *       c-th visible op.  Any other bit: RH_E_INVALID.
 *   pad == RH_GEN_ARG_PREV (col must be -1): the argument is the draw's CARRY, the value of op o - 1 of this draw -- a skipped op's
 *       value being the carry before it.  Not at op 0.
 * New families are numbered from 16.  Where the reference builds an argument out of Reals, the contract is the plain left-to-right
 * double expression written here: it differs from the reference's evaluation by rounding only, but unlike Gamma's pow it feeds
 * a .toLong.  pow(x, 0.5) is the IEEE square root.
 *   RH_GEN_BINOMIAL (p, k)                                                                                Discrete.scala:194-230
 *       k >= 100 && k * p <= 10:                          min(Poisson(p * k), (long)k)                    :205-208, 223-224
 *       else k >= 100 && k * p >= 9 && k * (1 - p) >= 9:  min(max((long)(g * sqrt(k * p * (1 - p)) + k * p), 0), (long)k)   :209-214, 225-226
 *       else: (int)k trials (Java's saturating d2i), each one u, counting  p + 0.0 >= u   :215-217; Multinomial.scala:26-29; Generator.scala:49-57, 129-141
 *   RH_GEN_NEGBINOMIAL (p, n)                                                                             Discrete.scala:81-109
 *       p < -100 / n + 1 && p > 100 / n - .25:            max((long)(g * (sqrt(n * p) / (1 - p)) + n * p / (1 - p)), 0)      :95-97, 103-104
 *       else: the sum of (long)n draws of (long)floor(log(u) / log(1 - (1 - p))), a 64-bit sum that wraps as the JVM's      :88-94, 59-69
 *   RH_GEN_CATEGORICAL (a = the first of m consecutive weight columns, b = the immediate m, an integer in 2 .. 255)   Generator.scala:129-141
 *       one u; cdf_i = w_i + cdf_(i-1), cdf_(-1) = 0.0; the value is the first i (from 0) with cdf_i >= u, else m - 1
 * Composites are tables, not families.  BetaBinomial(a, b, k) (Discrete.scala:240-244) is [BETA(a, b) hidden, BINOMIAL(PREV, k)].  A
 * mixture of m components (Discrete.scala:270-273, Continuous.scala's Mixture: Generator.categorical(components).flatMap(_.generator),
 * the categorical's uniform first, then only the chosen component's draws) is [CATEGORICAL hidden, component 0's ops with guard 1,
 * ..., component m - 1's ops with guard m], every component op but the last one hidden: skipped ops pass the carry through, so the
 * last op's column is the mixture's sample in every draw -- also where a component is itself a two-op BetaBinomial.
 * BINOMIAL / NEGBINOMIAL need p finite in [0, 1] and k / n finite and >= 0, CATEGORICAL every weight finite and >= 0: otherwise NaN,
 * RH_GEN_F_DOMAIN and nothing drawn.  An exact path of more than 4096 trials gives NaN and RH_GEN_F_CAP and draws nothing; the
 * Poisson and normal draws inside keep their own caps. */
enum rh_gen_family { RH_GEN_REAL = 0, RH_GEN_NORMAL = 1, RH_GEN_CAUCHY = 2, RH_GEN_LAPLACE = 3, RH_GEN_UNIFORM = 4, RH_GEN_LOGNORMAL = 5,
                     RH_GEN_GAMMA = 6, RH_GEN_BETA = 7, RH_GEN_BERNOULLI = 8, RH_GEN_GEOMETRIC = 9, RH_GEN_POISSON = 10,
                     RH_GEN_BINOMIAL = 16, RH_GEN_NEGBINOMIAL = 17, RH_GEN_CATEGORICAL = 18 };
#define RH_GEN_OP_GUARD(j) ((j) + 1)   /* rh_gen_op.reserved bits 0-7: run only where the selector is j */
#define RH_GEN_OP_HIDDEN 0x100         /* rh_gen_op.reserved bit 8 */
#define RH_GEN_ARG_PREV 1              /* rh_gen_arg.pad */
#define RH_GEN_F_DOMAIN 1
#define RH_GEN_F_CAP 2
typedef struct rh_gen_arg { int32_t col; int32_t pad; double value; } rh_gen_arg;  /* col >= 0: column of `in`; col == -1: `value`, or with pad == RH_GEN_ARG_PREV the carry */
typedef struct rh_gen_op  { int32_t family; int32_t reserved; rh_gen_arg a, b; } rh_gen_op;
typedef struct rh_generate rh_generate;
/* A generator as a table (what Generator.zip / traverse compose, core/Generator.scala:38-47, 145-150).  Validates without a device and
 * touches none: nops in 1 .. 4096, nin >= 0, a known family, every col in -1 .. nin-1, the second
 * argument of the one-argument families (REAL, BERNOULLI, GEOMETRIC, POISSON) unused (col -1, value 0); otherwise RH_E_INVALID with
 * a message that names the op.  Likewise refused: a guard with no earlier CATEGORICAL op or beyond its m, RH_GEN_ARG_PREV at op 0 or
 * with col != -1, a table with no visible op, a CATEGORICAL whose a is no column, whose b is no integer immediate in 2 .. 255 or whose
 * weights end beyond nin.  device: where the generator will run (-1: the device of its first call). */
int rh_generate_create(const rh_gen_op *ops, int32_t nops, int32_t nin, int32_t device, rh_generate **out);
void rh_generate_destroy(rh_generate *g);
/* the outputs per draw: the visible ops (= nops without RH_GEN_OP_HIDDEN: one sample per op, as Generator.traverse returns one value
 * per generator, Generator.scala:145-150) */
int rh_generate_nout(const rh_generate *g);
/* Trace.predict's sampling (Trace.scala:34-41) over any device buffer dev_in [chains][kept][nin] on `device` (-1: the handle's), e.g. a
 * predictor's *dev_out: on the null stream, synchronising the device before and after.  nin must be the handle's; a buffer on
 * another device is refused.  host_out (may be NULL): caller-allocated [chains][kept][nout]; *dev_out (may be NULL): the generator's
 * own buffer, valid until its next call; *flags (may be NULL): RH_GEN_F_* of the whole call.  No device: RH_E_DEVICE. */
int rh_generate_device(rh_generate *g, const void *dev_in, int32_t device, int32_t chains, int32_t kept, int32_t nin,
                       int64_t seed, int64_t chain0, double *host_out, void **dev_out, int32_t *flags);
/* trace.predict(distribution) over the sampler's own draws (Trace.scala:34-41, Generator.scala:171-174): rh_sampler_predict's window
 * through p, then g over p's output, on the sampler's stream with one synchronisation; the predictions stay in p's buffer.  p's nreq
 * must be g's nin and the three objects on one device, else RH_E_INVALID. */
int rh_sampler_generate(rh_sampler *s, rh_predict *p, rh_generate *g, int32_t first, int32_t count, int32_t thin,
                        int64_t seed, int64_t chain0, double *host_out, void **dev_out, int32_t *flags);
/* No device needed: the sampling kernel's code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a launch
 * (the generators of core/Continuous.scala:54-215 and core/Discrete.scala:38-186 above); *code_out is malloc'ed, freed with rh_free. */
int rh_generate_lower_only(const char *arch, void **code_out, size_t *code_size);
/* the same for the kernel of the count families, guards, hidden ops and carries (csrc/device/rh_generate_ext.hip.h) */
int rh_generate_ext_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- posterior covariance and correlation over device-resident draws --------------------------------------------------------
 * How two parameters move together: the reference's notebooks plot pairs (rainier-notebook package.scala:79-98); this is the pooled
 * sample covariance of the kept draws with the divisor of CovarianceEstimator.covariance (MassMatrixEstimator.scala:38-47), and
 * optionally the correlation, computed where the draws are (csrc/device/rh_cov.hip.h: X^T X of the centred draws on the fp64
 * matrix cores).  Window, thinning and flat rows are rh_sampler_summary's: kept = ceil(count/thin), N = chains * kept, flat row
 * r = c * kept + j is draw (c, first + j*thin).  Column k of the result is parameter cols[k] (duplicates allowed); cols == NULL:
 * all nvars in order, and ncols must be 0 or nvars.  K = ncols, or nvars without a list.
 * The sums run in a fixed order that depends on N alone.  A split is 4096 consecutive flat rows, S = ceil(N/4096):
 *   mean[k]    = (sum over s ascending of (sum over the rows r of split s ascending of x[r][k])) / (double)N, every sum one
 *                accumulator from +0.0 with plain adds;
 *   d[r][k]    = x[r][k] - mean[k], one rounding (two passes: a mean many standard deviations from zero costs no digits);
 *   P_s[a][b]  = one accumulator from +0.0, r ascending in split s: acc = fma(d[r][a], d[r][b], acc);
 *   cov[a][b]  = (sum over s ascending of P_s[a][b]) / (double)(N - 1), bitwise symmetric;
 *   corr[a][b] = cov[a][b] / (sqrt(cov[a][a]) * sqrt(cov[b][b])), IEEE operations in that order; the diagonal is exactly 1.0 where
 *                cov[a][a] is finite and > 0, else NaN, and so is an entry whose two columns are one parameter (a list that names
 *                it twice); not clamped, so |corr| may exceed 1 by rounding.
 * A NaN in a column makes that row and column NaN and touches nothing else.  Nothing depends on tiling, chunking, the order of the
 * column list or the launch: entry (a, b) of a call over cols has the bits of entry (cols[a], cols[b]) of the call over all columns.
 * mean [K], cov [K][K], corr [K][K]: caller-allocated on the host; each may be NULL, not all three.
 * The partial sums live in a bounded device workspace (128 MiB, walked in chunks of tile pairs of 64 x 64 columns); a shape whose
 * single tile pair is beyond it (S * 32 KiB) returns RH_E_UNSUPPORTED before any launch.  A broken window, N < 2, an index outside
 * [0, nvars), ncols < 1 with a list: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).
 * The sampler form goes to the sampler's stream behind its pending work, is not part of rh_timing and does not alter the chains;
 * count <= iterations completed - first. */
int rh_sampler_covariance(rh_sampler *s, int32_t first, int32_t count, int32_t thin, const int32_t *cols, int32_t ncols,
                          double *mean, double *cov, double *corr);
/* the same over any device buffer [chains][iterations][nvars] on `device` (-1: the current one), e.g. a predictor's *dev_out or
 * rh_comm_allgather_draws' *dev_out; synchronises the device before and after */
int rh_covariance_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first,
                         int32_t count, int32_t thin, const int32_t *cols, int32_t ncols, double *mean, double *cov, double *corr);
/* No device needed: the covariance kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_covariance_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- posterior histograms and joint count grids over device-resident draws ----------------------------------------------------
 * The shape of a posterior: the reference's density(seq, bounds) -- a histogram of one parameter's pooled draws between doubles.min
 * and doubles.max or between given bounds -- and scatter / contour of a pair (rainier-notebook package.scala:63-98), computed where
 * the draws are (csrc/device/rh_hist.hip.h: one binning pass, LDS integer adds); only the counts come back.  Window, thinning and
 * flat rows are rh_sampler_summary's: kept = ceil(count/thin), N = chains * kept, flat row r = c * kept + j is draw
 * (c, first + j*thin).  Column k of the result is parameter cols[k] (duplicates allowed); cols == NULL: all nvars in order, and ncols
 * must be 0 or nvars.  K = ncols, or nvars without a list.  1 <= nbins <= 1024.
 * Bounds: range is [K][2] on the host or NULL.  Column k takes (lo, hi) = range[k] unless range is NULL or both entries are NaN; then
 * lo and hi are the smallest and largest FINITE value of the pooled column, found on the device (2K doubles return; a -0.0 extreme
 * is returned as +0.0; a column with no finite value gets NaN edges, zero counts in every bin, and its rows land in under / over /
 * nan).  lo == hi, given or automatic: lo -= 0.5, hi += 0.5 (numpy's rule).  Where that changes nothing (a constant of magnitude 2^53 or
 * more) the width stays 0: all edges are equal and every row counts in the last, closed bin.  Given bounds must be finite with lo <= hi and hi - lo
 * finite, else RH_E_INVALID.
 * Edges: built on the host in double and returned.  With w = hi - lo: e[0] = lo, e[i] = min(hi, max(e[i-1], lo + ((double)i * w) /
 * (double)nbins)) for 0 < i < nbins, e[nbins] = hi: non-decreasing; they may repeat where w is a few ulps of lo.
 * Counts are defined against the returned edges and by nothing else (IEEE comparisons): counts[k][b] is the number of rows with
 * e[b] <= x < e[b+1] for b < nbins-1; the last bin is closed, e[nbins-1] <= x <= e[nbins]; under[k]: x < e[0] (-inf too); over[k]:
 * x > e[nbins] (+inf too); nan[k]: the NaNs; sum(counts[k]) + under[k] + over[k] + nan[k] == N.  That is np.histogram(finite values,
 * bins = e).  Nothing depends on tiling, chunking, the order of the column list or the launch: entry k of a call over cols equals
 * entry cols[k] of the call over all columns given the same bounds.
 * edges [K][nbins+1], counts [K][nbins] (int64), under / over / nan [K] (each may be NULL): caller-allocated on the host.
 * The partial counts live in a bounded device workspace (128 MiB, walked in chunks of column tiles); a shape whose single tile is
 * beyond it returns RH_E_UNSUPPORTED before any launch.  A broken window, N < 1, an index outside [0, nvars), nbins out of range, bad
 * bounds, ncols < 1 with a list: RH_E_INVALID, the message names the argument.  No device: RH_E_DEVICE (no CPU fallback).
 * The sampler form goes to the sampler's stream behind its pending work, is not part of rh_timing and does not alter the chains. */
int rh_sampler_histogram(rh_sampler *s, int32_t first, int32_t count, int32_t thin, const int32_t *cols, int32_t ncols, int32_t nbins,
                         const double *range, double *edges, int64_t *counts, int64_t *under, int64_t *over, int64_t *nan);
/* the same over any device buffer [chains][iterations][nvars] on `device` (-1: the current one); synchronises the device before and after */
int rh_histogram_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first,
                        int32_t count, int32_t thin, const int32_t *cols, int32_t ncols, int32_t nbins, const double *range,
                        double *edges, int64_t *counts, int64_t *under, int64_t *over, int64_t *nan);
/* Pairs: pairs is [npairs][2] parameter indices (npairs >= 1, a == b allowed); nbx, nby >= 1 with nbx * nby <= 4096; range is
 * [npairs][2][2] ((lo, hi) of x, then of y) or NULL, with the rules above per axis and the edge formula per axis.  grid[p][bx][by]
 * counts the rows whose x falls in bin bx of xedges[p] and whose y falls in bin by of yedges[p]; outside[p] (may be NULL) the rows where
 * either coordinate is out of range or NaN; sum(grid[p]) + outside[p] == N.  That is np.histogram2d(x, y, bins = [xedges, yedges]).
 * xedges [npairs][nbx+1], yedges [npairs][nby+1], grid [npairs][nbx][nby] (int64), outside [npairs]. */
int rh_sampler_histogram2d(rh_sampler *s, int32_t first, int32_t count, int32_t thin, const int32_t *pairs, int32_t npairs, int32_t nbx,
                           int32_t nby, const double *range, double *xedges, double *yedges, int64_t *grid, int64_t *outside);
int rh_histogram2d_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first,
                          int32_t count, int32_t thin, const int32_t *pairs, int32_t npairs, int32_t nbx, int32_t nby,
                          const double *range, double *xedges, double *yedges, int64_t *grid, int64_t *outside);
/* No device needed: the histogram kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_histogram_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- rank-normalised split R-hat, bulk ESS and tail ESS over device-resident draws ----------------------------------------------
 * Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), computed where the draws are (csrc/device/rh_rank.hip.h).  rh_diagnostics
 * and rh_sampler_diagnostics keep the reference's numbers (an unsplit R-hat on the raw values, a variogram ESS cut at lag 99); these
 * see what those cannot: a trend all chains share, a chain of another scale, a posterior without a variance.
 * Input: draws [chains][iterations][nvars], the window [first, first + count) of every chain, count >= 4, no thinning; column k of
 * the result is parameter cols[k] (duplicates allowed); cols == NULL: all nvars in order, and ncols must be 0 or nvars.
 * Split: h = count / 2 (floored).  Sequence q = 2c is (c, first + i), q = 2c + 1 is (c, first + count - h + i), i = 0 .. h-1: an odd
 * count leaves the middle draw out.  M = 2 chains sequences, S = M h values, flat index s = q h + i.
 * Order and ranks: Double.compare's order (-0.0 before +0.0), the summaries' key order.  The average rank of y_s among the S values is
 * r_s = (L_s + U_s + 1) / 2, L_s the number of values below it, U_s the number at or below it; z_s = Phi^-1((r_s - 3/8) / (S + 1/4)),
 * Phi^-1 by Wichura's AS 241 (PPND16).
 * Four series per column, each [M][h]: 1. z(y), the bulk series; 2. z(|y - med|), med = 0.5 sorted[S/2 - 1] + 0.5 sorted[S/2], the
 * folded series, ranked among themselves; 3. I(y <= sorted[floor(0.05 S)]); 4. I(y <= sorted[floor(0.95 S)]).  The thresholds are
 * order statistics (precis'), not interpolated quantiles: exact, and O(1/S) from the paper's.
 * Estimator on a series u [M][h], L = min(h - 1, 255):
 *   m_q = mean_i u[q][i];  g_q(t) = (1/h) sum_{i=0}^{h-1-t} (u[q][i] - m_q)(u[q][i+t] - m_q), t = 0 .. L, i ascending, one accumulator
 *   g(t) = mean_q g_q(t);  W = g(0) h / (h-1);  B = sum_q (m_q - mean_q m_q)^2 / (M-1);  V = (h-1)/h W + B;  rhat = sqrt(V / W)
 *   rho_0 = 1; rho_t = 1 - (W - g(t)) / V;  P_k = rho_2k + rho_2k+1, k = 0 .. K, K = (L-1)/2
 *   tau = -1; prev = +inf; for k = 0 .. K: if !(P_k > 0) { tau += max(rho_2k, 0); stop }  P = min(P_k, prev); prev = P; tau += 2P
 *   tau = max(tau, 1 / log10(S));  ess = S / tau;  truncated: the loop ran out of pairs without stopping
 * Outputs [K] each, caller-allocated on the host, none NULL: rhat_bulk and ess_bulk of series 1, rhat_folded of series 2, ess_tail
 * the smaller ESS of series 3 and 4 (NaN if either is NaN), truncated (int32) bit 0 bulk, bit 1 lower tail, bit 2 upper tail: where a
 * bit is set that ESS is an upper bound (the lags stop at 255: lag t is thread t of the chain kernel; seen on chains that do not mix).
 * NaN: a column whose window holds a NaN or an infinity gives NaN in all four (truncated 0), other columns are untouched; a series
 * whose W is not > 0 (a constant column, an indicator that is constant over all S -- the upper one whenever S < 20) gives NaN.
 * Deterministic: no floating-point atomics, every sum in an order that depends on the shape alone; a second call, a window and its
 * copy, and any chunking of the columns give the same bits.
 * The workspace (per column 32 S bytes and 8 M (L + 2)) is bounded by 128 MiB and walked in chunks of columns; a single column beyond
 * it returns RH_E_UNSUPPORTED from the shape alone, before any launch.  A broken window, count < 4, an index outside [0, nvars),
 * ncols < 1 with a list, a NULL output: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).
 * The sampler form goes to the sampler's stream behind its pending work, is not part of rh_timing and does not alter the chains. */
int rh_sampler_rank_diagnostics(rh_sampler *s, int32_t first, int32_t count, const int32_t *cols, int32_t ncols, double *rhat_bulk,
                                double *rhat_folded, double *ess_bulk, double *ess_tail, int32_t *truncated);
/* the same over any device buffer [chains][iterations][nvars] on `device` (-1: the current one); synchronises the device before and after */
int rh_rank_diagnostics_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first,
                               int32_t count, const int32_t *cols, int32_t ncols, double *rhat_bulk, double *rhat_folded, double *ess_bulk,
                               double *ess_tail, int32_t *truncated);
/* No device needed: the rank diagnostics kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_rank_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- Monte Carlo standard errors and ESS of the reported figures over device-resident draws ------------------------------------------
 * How many digits of a mean, an sd or a quantile survive the Monte Carlo error (Vehtari et al. 2021, section 4), computed where the
 * draws are (csrc/device/rh_mcse.hip.h): what stands next to rh_*_summary's table as the rank diagnostics stand next to a run.
 * Input: draws [chains][iterations][nvars], the window [first, first + count) of every chain, count >= 4, no thinning; cols / ncols as
 * for the rank diagnostics.  probs [nprobs], 0 <= nprobs <= 16, 0 < p < 1 (NULL with nprobs 0); nlags, 0 <= nlags <= 255.
 * Split, M, h, S, the flat index, the key order and L = min(h - 1, 255) are exactly rh_rank_diagnostics_device's.
 * Pooled figures per column, fixed-order sums whose order depends on S alone:
 *   m = sum y / S;  E2 = sum (y - m)^2 / S;  E4 = sum (y - m)^4 / S;  sd = sqrt(S E2 / (S - 1))
 * Series per column, each [M][h], each through the rank diagnostics' estimator unchanged (m_q, g_q(t), W, B, V, Geyer's pairs, tau_min,
 * truncated):  A: y;  B: |y - m|;  C: (y - m)^2;  D_k: I(key(y) <= sorted[j_k]), j_k = min(S - 1, (int64) floor((double) S probs[k])),
 * the summaries' quantile index.
 * Outputs, caller-allocated on the host, [K] or [K][nprobs], each may be NULL:
 *   mean = m;  sd;  ess_mean = ESS(A);  ess_sd = ESS(B);  mcse_mean = sd / sqrt(ess_mean);
 *   mcse_sd = sqrt((E4 - E2^2) / ESS(C) / E2 / 4)  (the delta method, the form the `posterior` package uses);
 *   quantile[k] = sorted[j_k];  ess_quantile[k] = ESS(D_k);
 *   mcse_quantile[k] = (sorted[i2] - sorted[i1]) / 2 with e = ess_quantile[k], a = qbeta(0.15865525393145707; e p + 1, e (1 - p) + 1),
 *   b = qbeta(0.8413447460685429; the same shapes), i1 = max(floor(a S), 1) - 1, i2 = min(ceil(b S), S) - 1  (qbeta: the inverse
 *   regularised incomplete beta function, on the host: csrc/qbeta.hpp);
 *   acf [K][nlags + 1]: rho_t of series A, rho_0 = 1, rho_t = 1 - (W - g(t)) / V, NaN beyond L;
 *   truncated [K] (int32): bit 0 A, bit 1 B, bit 2 C, bit 3 + k D_k.
 * NaN: a NaN or an infinity in the window turns every figure of that column into NaN (truncated 0), other columns are untouched; a
 * series without W > 0 gives a NaN ESS, and every figure derived from it (the acf with series A) is NaN.
 * Deterministic: no floating-point atomics; a second call, a window and its copy, a duplicated column and any chunking of the columns
 * give the same bits.
 * The workspace (per column 24 S bytes and 8 (3 + nprobs) M (L + 2): no derived series is ever written to memory) is bounded by
 * 128 MiB and walked in chunks of columns; a single column beyond it returns RH_E_UNSUPPORTED from the shape alone, before any
 * launch.  A broken window, count < 4, an index outside [0, nvars), ncols < 1 with a list, nprobs outside 0 .. 16, a probability
 * outside (0, 1), nlags outside 0 .. 255: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).
 * The sampler form goes to the sampler's stream behind its pending work, is not part of rh_timing and does not alter the chains. */
int rh_sampler_mcse(rh_sampler *s, int32_t first, int32_t count, const int32_t *cols, int32_t ncols, const double *probs, int32_t nprobs,
                    int32_t nlags, double *mean, double *sd, double *ess_mean, double *ess_sd, double *mcse_mean, double *mcse_sd,
                    double *quantile, double *ess_quantile, double *mcse_quantile, double *acf, int32_t *truncated);
/* the same over any device buffer [chains][iterations][nvars] on `device` (-1: the current one); synchronises the device before and after */
int rh_mcse_device(const void *dev_draws, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first, int32_t count,
                   const int32_t *cols, int32_t ncols, const double *probs, int32_t nprobs, int32_t nlags, double *mean, double *sd,
                   double *ess_mean, double *ess_sd, double *mcse_mean, double *mcse_sd, double *quantile, double *ess_quantile,
                   double *mcse_quantile, double *acf, int32_t *truncated);
/* No device needed: the standard error kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_mcse_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- pointwise WAIC and PSIS-LOO over device-resident log-likelihood draws --------------------------------------------------------
 * Which of two models predicts better (Vehtari, Gelman, Gabry 2017), computed where the draws are (csrc/device/rh_loo.hip.h).
 * Input: ll [chains][iterations][nvars], column i holding l_s = log p(y_i | theta_s); the kept iterations first + j * thin of every
 * chain, kept = ceil(count / thin) (rh_sampler_summary's window); one column has S = chains * kept pooled values, S >= 2.  Column k of
 * the result is column cols[k] (duplicates allowed); cols == NULL: all nvars in order, and ncols must be 0 or nvars.
 * WAIC per column:
 *   lpd = max + log(sum_s exp(l_s - max)) - log(S);  p_waic = sum_s (l_s - mean)^2 / (S - 1), mean = sum_s l_s / S, in two passes
 *   (elpd_waic = lpd - p_waic is the caller's).
 * PSIS per column (Vehtari, Simpson, Gelman, Yao, Gabry, as the `loo` package computes it):
 *   1. r_s = -l_s, sorted in the summaries' key order, r_(1) <= .. <= r_(S);  x = r - r_(S) <= 0.  (The device sorts l ascending and
 *      reads it backwards: the same subtraction l_(1) - l, the same bits.)
 *   2. M = ceil(min(S / 5, 3 sqrt(S))).
 *   3. lc = max(x_(S - M), log DBL_MIN).
 *   4. The tail: the n sorted values with x > lc (n <= M).  n <= 4: no smoothing, k = +inf.
 *   5. t_j = exp(x_(S - n + j)) - exp(lc), j = 1 .. n, ascending.
 *   6. Zhang & Stephens (2009): m = 30 + floor(sqrt(n));  b_j = [1 - sqrt(m / (j - 1/2))] / (3 t_(floor(n/4 + 1/2))) + 1 / t_(n), j = 1 .. m;
 *      k_j = mean_i log1p(-b_j t_i) (i ascending, one accumulator);  L_j = n (log(-b_j / k_j) - k_j - 1);  w_j = exp(L_j - logsumexp L),
 *      logsumexp L = max L + log(sum_j exp(L_j - max L)), no weight dropped;  bbar = sum_j b_j w_j;  khat = mean_i log1p(-bbar t_i);
 *      sigma = -khat / bbar;  the reported and used k = (n khat + 5) / (n + 10).
 *   7. p_j = (j - 1/2) / n;  q_j = sigma expm1(-k log1p(-p_j)) / k  (k == 0: -sigma log1p(-p_j));  the new log weight is
 *      lw_j = min(log(q_j + exp(lc)), 0).
 *   8. A k or a sigma that is not finite leaves the tail as it is and reports k = +inf.
 *   9. elpd_loo = log(sum_s exp(l_s + lw_s)) - log(sum_s exp(lw_s)), lw = x outside the tail and the smoothed value inside; outside the
 *      tail (and in a tail left as it is) l_s + lw_s = -r_(S) exactly, so it is evaluated as
 *        -r_(S) + log((S - n) + sum_j exp(lw_j - x_j)) - log(sum_{outside} exp(x_s) + sum_j exp(lw_j))     (an unsmoothed tail: lw_j = x_j)
 *      off the sorted column alone: no permutation is kept.
 * Sums over a column: thread t of 256 adds the sorted values i = t, t + 256, .. in ascending i, then a fixed binary tree; the m
 * weights are added in candidate order.  exp and log are fdlibm 5.3's, written out; log1p(x) = log(u) x / (u - 1) with u = fl(1 + x)
 * (x where u == 1) and expm1(x) = (u - 1) x / log(u) with u = exp(x) (x where u == 1, -1 where u - 1 == -1).
 * Outputs [K] each, caller-allocated on the host, none NULL: lpd, p_waic, elpd_loo, pareto_k, tail_n (int32, the n above).
 * A column whose window holds a NaN or an infinity gives NaN in the four doubles and tail_n = 0; other columns are untouched.  A
 * constant column gives p_waic = 0 (its mean is taken to be the value itself), k = +inf, tail_n = 0 and elpd_loo = lpd = l.
 * Deterministic: no floating-point atomics, every sum in an order that depends on the shape alone; a second call, a window and its
 * copy, any chunking of the columns and a shuffled column list give the same bits per column.
 * The workspace (16 S bytes per column) is bounded by 128 MiB and walked in chunks of columns; a single column beyond it, and one
 * whose M is beyond the 8064 tail values a workgroup's LDS holds (S above about 7.2 million), return RH_E_UNSUPPORTED from the shape
 * alone, before any launch.  A broken window, S < 2, an index outside [0, nvars), ncols < 1 with a list, a NULL output: RH_E_INVALID.
 * No device: RH_E_DEVICE (no CPU fallback).  Synchronises the device before and after. */
int rh_loo_device(const void *dev_ll, int32_t device, int32_t chains, int32_t iterations, int32_t nvars, int32_t first, int32_t count,
                  int32_t thin, const int32_t *cols, int32_t ncols, double *lpd, double *p_waic, double *elpd_loo, double *pareto_k,
                  int32_t *tail_n);
/* rh_sampler_predict's window through predictor p (whose requirements are the pointwise log-likelihoods), then the reduction above
 * over p's buffer [chains][kept][nreq] (cols index its requirements) behind it on the sampler's stream: one synchronisation, nothing
 * copied to the host but the figures.  Not part of rh_timing; the chains are not altered. */
int rh_sampler_loo(rh_sampler *s, rh_predict *p, int32_t first, int32_t count, int32_t thin, const int32_t *cols, int32_t ncols, double *lpd,
                   double *p_waic, double *elpd_loo, double *pareto_k, int32_t *tail_n);
/* No device needed: the WAIC / PSIS-LOO kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_loo_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- PSIS leave-one-out expectations and LOO-PIT over device-resident draws ---------------------------------------------------------
 * Is the model calibrated: the leave-one-out predictive distribution of each observation (the `loo` package's E_loo and loo_pit),
 * computed where the draws are (csrc/device/rh_loo_expect.hip.h) with the smoothed importance weights rh_loo_device fits.
 * Input: ll [chains][iterations][nll] (column i: l_s = log p(y_i | theta_s)) and val [chains][iterations][nval] (a prediction or a
 * replicated observation per draw) on one device -- they may be one buffer -- over rh_loo_device's window and thinning; S = chains *
 * kept >= 2 draws, flat index s = c * kept + j.  Result k pairs log-likelihood column ll_cols[k] with value column val_cols[k]; both
 * lists are required, duplicates are allowed.  Per pair:
 *   a. The tail fit: steps 1 - 8 of rh_loo_device on the log-likelihood column, bit for bit: pareto_k and tail_n are what rh_loo_device
 *      returns for that column.
 *   b. The weight of draw s.  a: the ascending sorted column, n the tail's length, [p_lo, p_hi) the positions whose key equals the key
 *      of l_s (a group of equal keys lies wholly inside or wholly outside the tail, which is cut by value).  Outside the tail, or in a
 *      tail left unsmoothed: W_s = exp(a[0] - l_s).  Inside a smoothed tail: W_s = (sum_{p = p_lo}^{p_hi - 1} exp(lw_{n - p})) / (p_hi -
 *      p_lo), added in ascending p with one accumulator: draws with equal log-likelihoods (mostly rejected proposals, that is, repeated
 *      draws) share their group's mean weight, which does not depend on the draws' order and keeps the total weight.  W_s <= 1.
 *   c. Sums over s: thread t of 256 adds s = t, t + 256, .. in ascending order, then a fixed binary tree.  den = sum W;
 *      mean = sum W v / den (where every draw has one value, that value itself, as rh_loo_device takes a constant column's mean: the
 *      variance is then 0);  var = sum W (v - mean)^2 / den, in a second pass;  pit = sum W [v <= y_k] / den;  pit_lt the same with <
 *      (a discrete y_rep is randomised between the two on the host);  ess = den^2 / sum W^2.
 * y [ncols] or NULL: without it pit and pit_lt may be NULL and are not written; a NaN y[k] gives NaN in both; y = +inf gives exactly 1
 * (the sums den runs, in den's order), y = -inf exactly 0.  Outputs [ncols] each, caller-allocated on the host: mean, var, pit,
 * pit_lt, ess, pareto_k, tail_n (int32).
 * A NaN or an infinity in the log-likelihood window gives NaN in all doubles and tail_n = 0, as in rh_loo_device; one in the value
 * window gives NaN in mean, var, pit and pit_lt and leaves ess, pareto_k and tail_n intact.  A constant log-likelihood column gives k =
 * +inf, n = 0 and W = 1: the plain mean and variance, ess = S.  Other pairs are never touched.
 * Deterministic: no floating-point atomics, every sum in an order fixed by the shape; a second call, a window and its copy, any
 * chunking and any order of the pair list give the same bits per pair.
 * The workspace (per pair 16 S bytes, the two key buffers, of which the spare one then holds the draws' weights, and 8 M for the tail's
 * weights) is bounded by 128 MiB and walked in chunks of pairs; a single pair beyond it, and one whose M is beyond the 8064 tail values a
 * workgroup's LDS holds, return RH_E_UNSUPPORTED from the shape alone, before any launch.  A broken window, S < 2, an index out of
 * range, ncols < 1, a NULL list or a NULL output (pit, pit_lt: with y): RH_E_INVALID; the two buffers on different devices:
 * RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).  Synchronises the device before and after. */
int rh_loo_expect_device(const void *dev_ll, int32_t nll, const void *dev_val, int32_t nval, int32_t device, int32_t chains, int32_t iterations,
                         int32_t first, int32_t count, int32_t thin, const int32_t *ll_cols, const int32_t *val_cols, int32_t ncols, const double *y,
                         double *mean, double *var, double *pit, double *pit_lt, double *ess, double *pareto_k, int32_t *tail_n);
/* rh_sampler_predict's window through p_ll (the pointwise log-likelihoods) and p_val (they may be one predictor); with g (may be NULL),
 * g runs over p_val's output exactly as rh_sampler_generate runs it with chain0 = 0 -- the same seed gives the same y_rep bits -- and
 * the values are the generator's outputs, which val_cols then index.  The reduction above follows on the sampler's stream: one
 * synchronisation, nothing copied to the host but the figures.  Not part of rh_timing; the chains are not altered.  p_ll, p_val and g
 * on different devices, or g's width not p_val's: RH_E_INVALID. */
int rh_sampler_loo_expect(rh_sampler *s, rh_predict *p_ll, rh_predict *p_val, rh_generate *g, int64_t seed, int32_t first, int32_t count,
                          int32_t thin, const int32_t *ll_cols, const int32_t *val_cols, int32_t ncols, const double *y, double *mean,
                          double *var, double *pit, double *pit_lt, double *ess, double *pareto_k, int32_t *tail_n);
/* No device needed: the leave-one-out expectation kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as
 * before a launch; *code_out is malloc'ed, freed with rh_free. */
int rh_loo_expect_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- leave-one-out predictive quantiles and CRPS over device-resident draws ----------------------------------------------------------
 * What the leave-one-out predictive distribution of each observation looks like beyond its first two moments: its quantiles (the `loo`
 * package's E_loo(type = "quantile"), the input of ppc_loo_intervals), its continuous ranked probability score against y and its spread
 * E|X - X'| -- functionals of the weighted empirical distribution function of a value column, computed where the draws are
 * (csrc/device/rh_loo_quantile.hip.h).
 * Input: as rh_loo_expect_device's: ll [chains][iterations][nll] and val [chains][iterations][nval] on one device over its window and
 * thinning, S = chains * kept >= 2; result k pairs ll_cols[k] with val_cols[k].  probs [nprobs], 1 <= nprobs <= 16, each in [0, 1].
 * Plain mode: dev_ll == NULL (ll_cols is then not read): every weight is 1, no log-likelihood is sorted or fitted, and pareto_k and
 * tail_n are not written and may be NULL.  Per pair:
 *   a. Weights.  W_s is rh_loo_expect_device's (a) and (b), bit for bit: the same tail cut, the same fit, the same mean over a group of
 *      equal keys, exp(a[0] - l_s) outside the tail.  pareto_k and tail_n are rh_loo_device's.
 *   b. Order.  The S pairs (key of v_s, bits of W_s) -- the key is rh_summary's: Double.compare's order, -0.0 before +0.0 -- are sorted
 *      ascending, lexicographically: x_(1) <= .. <= x_(S) with W_(j) beside them.  W >= 0, so the bits' order is the numeric one, and the
 *      sorted sequence is a function of the multiset alone: no result depends on the draws' order.
 *   c. Cumulative weight.  C_j = W_(1) + .. + W_(j), added in an order fixed by S alone (a running sum over a contiguous segment
 *      of the sorted pairs on top of the sum of the segments before it; csrc/device/rh_loo_quantile.hip.h states the segments, which
 *      are not part of this contract).  What is promised: C is non-decreasing in j as computed, C_S is the last of them, and the same
 *      S and multiset give the same bits.
 *   d. Quantile at p: t = p C_S (one multiplication), j the smallest index with C_j >= t (a binary search along C).  j = 1: x_(1).
 *      Otherwise x_(j-1) + (x_(j) - x_(j-1)) ((t - C_(j-1)) / (C_j - C_(j-1))), and x_(j) itself where t == C_j (the fraction is then 1:
 *      the knot is returned with its own bits).  The divisor is > 0 by the choice of j.  p = 0 gives x_(1), p = 1 the largest value of
 *      positive weight (of a weight that still moves C: behind a draw that carries all but 2^-53 of it an addition absorbs the
 *      rest).  quantiles [k * nprobs + i].
 *   e. Scores.  F_j = C_j / C_S and G_j = 1 - F_j; for each gap [a, b) = [x_(j), x_(j+1)), j = 1 .. S - 1, with m = min(max(y, a), b):
 *        crps   = sum_j ((m - a) F_j^2 + (b - m) G_j^2) + max(x_(1) - y, 0) + max(y - x_(S), 0)
 *        spread = 2 sum_j (b - a) F_j G_j                                         (= E|X - X'|;  crps = E|X - y| - spread / 2)
 *      G_j is evaluated as R_j / C_S, R_j = W_(j+1) + .. + W_(S) the weight above x_(j), summed from behind as C is from the front,
 *      again in an order fixed by S alone: the subtraction 1 - F_j loses every digit where a few draws carry nearly all the weight, a quotient of sums of
 *      non-negative terms loses none.  Every term is non-negative; the terms are added in an order fixed by S alone.  crps >= 0, smaller is better (the `loo` package reports the negative).  y = +-inf gives crps = +inf.
 * y [ncols] or NULL; crps [ncols] (needs y) and spread [ncols] may be NULL and are then not computed for output.
 * A NaN or an infinity in the log-likelihood window gives NaN in every double of the pair and tail_n = 0; one in the value window gives
 * NaN in the pair's quantiles, crps and spread and leaves pareto_k and tail_n intact; a NaN y[k] gives NaN in crps[k] only.  Every NaN is
 * the positive quiet one.  A constant value column c falls out of the formulas: every quantile is c, spread = 0, crps = |c - y|.  Other
 * pairs are never touched.
 * Deterministic: no floating-point atomics; a second call, a window and its copy, any chunking, any order of the pair list and any
 * order of the draws give the same bits per pair.
 * The workspace (per pair 32 S bytes, two buffers of keys and payloads -- the log-likelihood side sorts inside the second and leaves
 * the draws' weights there until the first merge pass over pairs --, and 8 M for the tail's weights) is bounded by 128 MiB and walked
 * in chunks of pairs; a single pair beyond it, and one whose M is beyond the 8064 tail values a workgroup's LDS holds, return
 * RH_E_UNSUPPORTED from the shape alone, before any launch.  A broken window, S < 2, an index out of range, ncols < 1, nprobs outside
 * 1 .. 16, a probability outside [0, 1] (a NaN included), a NULL list or a NULL output (pareto_k, tail_n: with dev_ll), crps without y:
 * RH_E_INVALID; the two buffers on different devices: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback).  Synchronises the
 * device before and after. */
int rh_loo_quantile_device(const void *dev_ll, int32_t nll, const void *dev_val, int32_t nval, int32_t device, int32_t chains, int32_t iterations,
                           int32_t first, int32_t count, int32_t thin, const int32_t *ll_cols, const int32_t *val_cols, int32_t ncols, const double *y,
                           const double *probs, int32_t nprobs, double *quantiles, double *crps, double *spread, double *pareto_k, int32_t *tail_n);
/* rh_sampler_loo_expect's arrangement: the window through p_ll (NULL: plain mode) and p_val (they may be one predictor); with g (may be
 * NULL), g runs over p_val's output exactly as rh_sampler_generate runs it with chain0 = 0 -- the same seed gives the same y_rep bits --
 * and the values are the generator's outputs.  The sorts and the scan follow on the sampler's stream: one synchronisation, nothing
 * copied to the host but the figures.  Not part of rh_timing; the chains are not altered.  p_ll, p_val and g on different devices, or
 * g's width not p_val's: RH_E_INVALID. */
int rh_sampler_loo_quantile(rh_sampler *s, rh_predict *p_ll, rh_predict *p_val, rh_generate *g, int64_t seed, int32_t first, int32_t count,
                            int32_t thin, const int32_t *ll_cols, const int32_t *val_cols, int32_t ncols, const double *y, const double *probs,
                            int32_t nprobs, double *quantiles, double *crps, double *spread, double *pareto_k, int32_t *tail_n);
/* No device needed: the leave-one-out quantile kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before
 * a launch; *code_out is malloc'ed, freed with rh_free. */
int rh_loo_quantile_lower_only(const char *arch, void **code_out, size_t *code_size);

/* ---- posterior predictive checks over device-resident replicated draws -------------------------------------------------------------
 * Does the fitted model reproduce the features of the data that were observed -- its spread, its extremes, its share of zeros, group
 * by group (Gelman, Meng and Stern 1996; bayesplot's ppc_stat and ppc_stat_grouped) -- computed where the replicated observations are
 * (csrc/device/rh_ppc.hip.h).  Input: rep [chains][iterations][nin], a row being one replicated data set (rh_sampler_generate's
 * buffer); the kept iterations first + j * thin of every chain, kept = ceil(count / thin), S = chains * kept draws, flat row
 * r = c * kept + j (rh_sampler_predict's window).  The one call that reduces along a row, over the observations.
 * A check is a table.  cols [K]: columns of the row, duplicates allowed; NULL: all nin in order (K 0 or nin).  seg_off [nseg + 1] cuts
 * that list into nseg non-empty runs: seg_off[0] = 0, strictly ascending, seg_off[nseg] = K; NULL: one segment (nseg 0 or 1).  Segment g
 * of a draw is the values row[cols[seg_off[g] .. seg_off[g+1])], n_g of them.  stats [nstat], nstat >= 1, are evaluated on every
 * segment: nout = nseg * nstat outputs per draw, T[r][g * nstat + k] -- the layout [chains][kept][nout] every other device call reads.
 *   RH_PPC_MEAN         sum v / n
 *   RH_PPC_SD           sqrt(sum (v - mean)^2 / (n - 1)), in two passes; n = 1: NaN (the formula's 0 / 0)
 *   RH_PPC_MIN, _MAX    in the summaries' key order (Double.compare's): -0.0 before +0.0
 *   RH_PPC_QUANTILE(p)  the order statistic sorted[min(n - 1, (int64)floor((double)n * p))], 0 <= p <= 1: precis' rule, the index
 *                       computed on the host in double per (segment, statistic)
 *   RH_PPC_FRAC_LE(c)   #{v <= c} / n, c finite: the share of zeros of count data, exceedance shares
 * arg is p or c, and 0 for the kinds that take none; reserved is 0.
 * Rules.  A segment that holds a NaN gives NaN in every statistic of that draw and segment, and nothing else is touched: no result
 * depends on where a NaN sorts.  Infinities follow IEEE arithmetic (a segment with +inf: mean +inf, sd NaN).  Every NaN returned is the
 * positive quiet NaN.  Where all keys of a segment are equal the mean is that value and, for n >= 2, the sd is 0, as rh_loo_device
 * treats a constant column: sum c / n does not always round back to c.  Sums: with w(n) = clamp(2^ceil(log2 n) / 16, 1, 256), partial
 * t of w(n_g) adds the segment's values i = t, t + w, .. in ascending i from +0.0, then the partials are added as a fixed binary tree
 * (p[t] += p[t + s], s = w/2, w/4, .. 1): the order depends on n_g alone -- not on K, the other segments, the tiling or the call.  No
 * floating-point atomics.
 * The observed statistics.  y [nin] (indexed by input column; may be NULL): t_obs [nout] is made by the same device routine on y as a
 * buffer of one row, so both sides of every comparison went through identical arithmetic.  For each output three counts over the S
 * draws, plain double comparisons: n_bad = #{T is NaN}, n_gt = #{T > t_obs}, n_eq = #{T == t_obs}; a NaN t_obs gives n_gt = n_eq = 0.
 * The Bayesian p-value is the caller's: (n_gt + n_eq) / (S - n_bad), or with half of n_eq.  With y == NULL, t_obs and the three counts
 * are not written and may be NULL.
 * Caps, refused from the shape alone before any launch with RH_E_UNSUPPORTED: K above 4096 (one row is staged in the workgroup's LDS;
 * there is no tiled-row path), nstat above 16, nout above 4096. */
enum rh_ppc_kind { RH_PPC_MEAN = 0, RH_PPC_SD = 1, RH_PPC_MIN = 2, RH_PPC_MAX = 3, RH_PPC_QUANTILE = 4, RH_PPC_FRAC_LE = 5 };
typedef struct rh_ppc_stat { int32_t kind; int32_t reserved; double arg; } rh_ppc_stat;
typedef struct rh_ppc rh_ppc;
/* Validates without a device and touches none: a known kind, arg in its domain, reserved 0, every cols entry in 0 .. nin-1, the
 * seg_off rules; otherwise RH_E_INVALID with a message that names the offending entry (the caps: RH_E_UNSUPPORTED).  device: where
 * the check will run (-1: the device of its first call). */
int rh_ppc_create(const rh_ppc_stat *stats, int32_t nstat, const int32_t *cols, int32_t K, const int32_t *seg_off, int32_t nseg, int32_t nin,
                  int32_t device, rh_ppc **out);
void rh_ppc_destroy(rh_ppc *h);
/* the outputs per draw, nseg * nstat */
int rh_ppc_nout(const rh_ppc *h);
/* over any device buffer dev_rep [chains][iterations][nin] on `device` (-1: the handle's), e.g. a generator's *dev_out: on the null
 * stream, synchronising the device before and after.  nin must be the handle's; a buffer on another device is refused.  t_obs [nout]
 * (double), n_gt, n_eq, n_bad [nout] (int64): caller-allocated on the host, required with y.  host_out (may be NULL): caller-allocated
 * [chains][kept][nout]; *dev_out (may be NULL): the handle's own buffer of that shape, valid until the handle's next call.  A broken
 * window, another nin, a NULL: RH_E_INVALID.  No device: RH_E_DEVICE (no CPU fallback). */
int rh_ppc_device(rh_ppc *h, const void *dev_rep, int32_t device, int32_t chains, int32_t iterations, int32_t nin, int32_t first, int32_t count,
                  int32_t thin, const double *y, double *t_obs, int64_t *n_gt, int64_t *n_eq, int64_t *n_bad, double *host_out, void **dev_out);
/* rh_sampler_generate's path -- p over the window, g over p's output with the same seed rule, so the same y_rep bits -- then the check
 * over the generator's buffer [chains][kept][g's nout], all on the sampler's stream with one synchronisation; nothing is copied to
 * the host but what is asked for.  g's nout must be h's nin (and p's nreq g's nin) and all four objects on one device, else
 * RH_E_INVALID.  Not part of rh_timing; the chains are not altered.  The generator's RH_GEN_F_* flags are not reported by this call:
 * a sample outside its family's domain and a capped rejection loop are both NaN samples, so they make their segment's statistics NaN
 * and are counted in n_bad; a caller who wants to tell the two apart runs rh_sampler_generate with the same seed. */
int rh_sampler_ppc(rh_sampler *s, rh_predict *p, rh_generate *g, rh_ppc *h, int64_t seed, int64_t chain0, int32_t first, int32_t count, int32_t thin,
                   const double *y, double *t_obs, int64_t *n_gt, int64_t *n_eq, int64_t *n_bad, double *host_out, void **dev_out);
/* No device needed: the predictive check kernels' code object for `arch` (NULL: gfx950) through the kernel cache, judged as before a
 * launch; *code_out is malloc'ed, freed with rh_free. */
int rh_ppc_lower_only(const char *arch, void **code_out, size_t *code_size);

int rh_abi_version(void);
/* number of visible HIP devices, or a negative rh_status */
int rh_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
