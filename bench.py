#!/usr/bin/env python
"""bench.py -- BASELINE.json metric on the BASELINE.json config (see the contract in the task statement).

  metric : leapfrog steps/sec summed over all chains (one step = one (p,q) update = one distinct gradient
           evaluation), plus ESS/sec (Trace.diagnostics formula, min over parameters)
  config : cfg 2 -- README linear regression, 3 covariates x 1e6 rows (un-inlined, streamed), static HMC L=32,
           1024 chains per GPU, DualAvgTuner(0.8), identity mass, chain seeds 1000 + global chain id.
  step   : one HMC iteration of every chain = 32 leapfrog steps x chains x 1e6 rows.
  --warmup W : W sampler warm-up iterations (step-size search + dual averaging), untimed.
  N > 1  : one process per GPU (launched by torch.distributed.run); chains sharded by global id (weak scaling: 1024 per
           GPU), data replicated, no collective on the data path; ONE RCCL all-gather of the device-resident draws over
           xGMI at the end, inside the timed region, issued by the engine behind its C ABI (rh_comm_*).  torch.distributed is
           used with the gloo (CPU) backend only: to hand rank 0's RCCL unique id to the other ranks and for the barriers --
           torch never initialises its own bundled HIP runtime beside the engine's.

Synthetic data (numpy default_rng(20260925)); inputs resident in HBM before the timed region starts.

A plain run (`--gpus 1 --steps K --warmup W`) does what the headline figure needs and no more: set-up, the W warm-up steps, the K timed
steps, `--dump-outputs`, the result line (its `roofline` comes from the timed steps' own HIP events).  `--full` adds every figure that takes
a run of its own -- the two ESS/s legs, `roofline.traffic` measured under rocprofv3, the `configs` block (the other BASELINE
configurations), `gpu_inlined`, `cpu_baseline` -- to the same line; the `--no-*` switches drop single ones of them from a `--full` run.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
FP64_PEAK_TFLOPS = 78.6    # MI355X public FP64 vector peak (not in the local guide)
TRAFFIC_PROFILE = "r5_cfg2/pmc_grad_kernel.json"   # PMC summary of the dominant kernel (see the roofline.traffic comment)
DUMP_MAX_BYTES = 64 << 20  # --dump-outputs writes at most this much


def dump_outputs(path, draws):
    """--dump-outputs DIR: what the timed path hands its caller for its last step -- the draw of every chain in the last timed
    iteration -- as DIR/draws.npy, float64 [chains][parameters].  Beyond DUMP_MAX_BYTES (cfg 5: 10 004 parameters x 1024 chains) a
    fixed, seeded sample of the chains is kept, in chain order: the same chains in every run with the same arguments."""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    if draws.nbytes > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // draws[0].nbytes
        draws = draws[np.sort(np.random.default_rng(0).choice(len(draws), keep, replace=False))]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "draws.npy"), draws)


def cpu_baseline(spec, L, seconds_budget=30.0):
    """The oracle (oracle/: C restatement of the reference JVM path, kind = "port") timed on ALL of this box's host
    cores on a bounded sample of the same workload: one chain per thread, each running whole HMC iterations
    (L=32) over the full data set with the reference's own 2L+1 gradient evaluations per trajectory.
    Two more figures beside it, each labelled: the same streamed gradient compiled by hand (upper bound for a JVM on the
    streamed form), and the INLINED sufficient-statistics form -- what real Rainier runs for this model."""
    from tests import oracle_lib as O
    from rainier_amd import models as _m
    nproc = os.cpu_count() or 1
    try:
        nproc_avail = len(os.sched_getaffinity(0))
    except AttributeError:
        nproc_avail = nproc
    cores = max(1, nproc_avail)
    # BOUNDED sample: the interpreter costs ~80 ns per row and gradient, one HMC iteration is 2L+1 = 65 gradients, and every
    # thread streams its own pass, so the sample is the first `n_s` rows of the same columns (cost is linear in the rows;
    # the smaller working set can only flatter the CPU) and the iteration count is calibrated UNDER CONTENTION (all threads
    # running) to ~12 s.  `value` is converted to full-size leapfrog steps/s (x n_s / N); `sample` says so.
    N = spec.rows_streamed
    n_s = min(N, 100_000)
    spec_s = _m.linreg(n=n_s, k=len(spec.columns) - 1, columns=[np.ascontiguousarray(c[:n_s]) for c in spec.columns])

    def run_all(iters, Lc=L):     # (reads spec_s when called: the sample in rows, or the full data set)
        cfg = O.make_config(sampler=O.HMC, n_steps=Lc, iterations=iters, warmup=0, step_tuner=O.STEP_STATIC,
                            static_step=1e-3, math_mode=O.JM_LIBM)
        steps = [0] * cores

        def work(i):
            d = O.OracleDensity(spec_s)
            _, _, st, _ = O.sample_chain(d.fn_ptr, d.handle, spec_s.n_params, cfg, 1000 + i)
            steps[i] = st.leapfrog_steps
        th = [threading.Thread(target=work, args=(i,)) for i in range(cores)]
        t = time.perf_counter()
        [x.start() for x in th]; [x.join() for x in th]
        return time.perf_counter() - t, float(sum(steps))

    t1, _ = run_all(1)                                   # calibration, all threads busy: one L-step iteration on the first n_s rows
    # The figure is measured over the FULL data set whenever one iteration of every chain over it fits the budget (cost is linear
    # in the rows: t1 x N / n_s) -- if need be with a shorter static trajectory: a leapfrog step costs (2 L + 1) / L gradient
    # evaluations in the reference (LeapFrog.scala:158-188), 2.03 at L = 32 and 2.125 at L = 8, so steps/s at L = 8 understates the
    # L = 32 figure by 4 %, stated in `sample`.  Only when even that does not fit is the sample cut in rows, as before.
    L_cpu = L
    full = None
    for Lc in [L] + [x for x in (16, 8, 4) if x < L]:
        if n_s < N and t1 * (N / n_s) * ((2 * Lc + 1) / (2.0 * L + 1)) <= seconds_budget:
            full = Lc
            break
    if n_s == N:
        iters = max(1, min(200, int(0.6 * seconds_budget / max(t1, 1e-3))))
    elif full is not None:
        n_s, spec_s, L_cpu, iters = N, spec, full, 1
    else:
        iters = max(1, min(200, int(0.6 * seconds_budget / max(t1, 1e-3))))
    dt, total = run_all(iters, L_cpu)
    total_full = total * n_s / N                         # leapfrog steps over the FULL data set this corresponds to
    # second figure ("speed build"): the same streamed gradient written out by hand and compiled -O3 with
    # AVX2/FMA (oracle/closed_form.c) -- an upper bound for any JVM on these cores; one chain per thread, ~3 s
    lib = O.load(); cols = [np.ascontiguousarray(c) for c in spec.columns]; n = len(cols[0])
    def run_closed(reps):
        th2 = [threading.Thread(target=lambda: lib.orc_linreg_streamed_reps(*[O._dp(c) for c in cols], n, reps)) for _ in range(cores)]
        t = time.perf_counter(); [x.start() for x in th2]; [x.join() for x in th2]
        return time.perf_counter() - t
    per = run_closed(1)                                  # calibration with every core streaming (memory-bandwidth contention included)
    reps = max(1, min(10000, int(3.0 / max(per, 1e-4))))
    dt2 = run_closed(reps)
    closed = {"value": cores * reps / dt2, "unit": "leapfrog steps/s (1 gradient per step)", "cores": cores,
              "row_chain_evals_per_s": cores * reps * n / dt2,
              "sample": "%d threads x %d streamed gradients over %d rows, hand-written C, -O3 -mavx2 -mfma, %.1f s" % (cores, reps, n, dt2)}
    # third figure: the INLINED form.  TargetGroup.inlinable + PartialEvaluator.inline (compute/Target.scala:20-24,136-207,
    # compute/PartialEvaluator.scala:90-97) fold the row sum of this model (3 covariates: 15 distributed terms < 20) into
    # scalar coefficients at compile time, so the reference's compiled gradient is O(1) in the row count
    # (rainier-benchmark/benchmarks.txt: Normal, 1 us per gradient at every N).  Here: one chain per thread doing leapfrog
    # steps on that O(1) density, hand-written C over the 15 sufficient statistics (~2 s).
    S = np.zeros(15)
    lib.orc_linreg_suffstats(*[O._dp(c) for c in cols], C.c_long(n), O._dp(S))
    lib.orc_linreg_inlined_leapfrog.restype = C.c_double
    lib.orc_linreg_inlined_leapfrog.argtypes = [C.POINTER(C.c_double), C.c_long, C.c_double]
    t = time.perf_counter(); lib.orc_linreg_inlined_leapfrog(O._dp(S), 200000, 1e-6); per_step = (time.perf_counter() - t) / 200000
    nsteps = max(1000, int(2.0 / per_step))
    th3 = [threading.Thread(target=lambda: lib.orc_linreg_inlined_leapfrog(O._dp(S), nsteps, 1e-6)) for _ in range(cores)]
    t = time.perf_counter(); [x.start() for x in th3]; [x.join() for x in th3]; dt3 = time.perf_counter() - t
    inlined = {"value": cores * nsteps / dt3, "unit": "leapfrog steps/s (1 gradient per step)", "cores": cores,
               "per_thread": nsteps / dt3,
               "what": "the sufficient-statistics form PartialEvaluator.inline produces -- what real Rainier runs for cfg 2; "
                       "O(1) per gradient, no rows streamed (so no row_chain_evals figure exists for it)",
               "reference_published": "rainier-benchmark/benchmarks.txt: ~1 us per gradient on the JVM at any N => ~5e5 leapfrog "
                                      "steps/s per thread at the reference's 2 gradients per step",
               "sample": "%d threads x %d leapfrog steps on the inlined density, hand-written C -O3, %.1f s" % (cores, nsteps, dt3)}
    return {"value": total_full / dt, "compiled_closed_form": closed, "inlined_sufficient_statistics": inlined,
            "unit": "leapfrog steps/s", "cores": cores, "nproc": nproc, "kind": "port",
            "sample": ("%d chains (one per core) x %d HMC iteration(s) (L=%d%s) over ALL %d rows, RIR interpreter, reference's 2L+1 gradient "
                       "evaluations per trajectory, %.1f s; value = measured steps/s (no extrapolation)" % (
                           cores, iters, L_cpu, "" if L_cpu == L else ": a shorter trajectory than the bench's %d so that the full data set fits the "
                           "budget -- %.3f instead of %.3f gradient evaluations per step, i.e. the figure understates L=%d by %.0f %%" % (
                               L, (2 * L_cpu + 1) / L_cpu, (2 * L + 1) / L, L, 100 * (1 - ((2 * L + 1) / L) / ((2 * L_cpu + 1) / L_cpu))), N, dt)) if n_s == N else
                      ("%d chains (one per core) x %d HMC iterations (L=%d) over the first %d of the %d rows, RIR interpreter, "
                       "reference's 2L+1 gradient evaluations per trajectory, %.1f s; value = measured steps/s x %d/%d "
                       "(full-size equivalent)" % (cores, iters, L, n_s, N, dt, n_s, N)),
            "measured_on_sample": {"leapfrog_steps_per_s": total / dt, "rows": n_s},
            "row_chain_evals_per_s": total * n_s / dt}


def gpu_inlined(R, models, device, L):
    """cfg 2 as the reference would REALLY hand it over (compute/Target.scala:20-24, PartialEvaluator.scala:90-97): 3 covariates
    = 15 distributed terms < 20, so TargetGroup inlines the likelihood into a 5-parameter data-free target -- O(1) per gradient,
    no rows streamed.  `models.linreg_reference` is that program from the reference's own front end (restated, compute.py); it
    runs on rh_chain_kernel (packed chains).  The like-for-like partner of cpu_baseline.inlined_sufficient_statistics.
    The compiled program has the same size for any row count; it is built from the first 20 000 rows here because the Python
    restatement of PartialEvaluator folds the rows one by one like the reference does (70 s at 1e6 rows)."""
    t0 = time.perf_counter()
    spec = models.linreg_reference(n=20_000, k=3)
    build_s = time.perf_counter() - t0
    assert spec.rows_streamed == 0
    model = R.Model(spec, device=device, fp_contract=True, factor_outputs=True)
    res = {"what": "cfg 2 inlined by the reference's own front end (5-parameter data-free target) on rh_chain_kernel, static HMC L=%d, "
                   "DualAvgTuner(0.8), identity mass" % L, "unit": "leapfrog steps/s", "front_end_seconds": build_s, "rows_folded": 20_000}
    for chains in (1024, 32768):
        cfg = R.make_config(100, 50, R.HMCSampler(L), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner())
        s = R.Sampler(model, cfg, [1000 + c for c in range(chains)])
        s.warmup()
        t0 = time.perf_counter(); s.run(100); dt = time.perf_counter() - t0
        stats, _ = s.stats()
        s.close()
        res["chains_%d" % chains] = sum(st.leapfrogSteps for st in stats) / dt
    return res


def live_traffic(a, kernel):
    """roofline.traffic measured in THIS run: FETCH_SIZE and WRITE_SIZE of the dominant kernel from two separate `rocprofv3 --pmc`
    passes (they do not fit one pass; --kernel-trace only, never a runtime trace) over a short child run of this same command --
    same model, chains, rows, build options, hence the same code object from the kernel cache.  KB per launch (mean over the
    launches of `kernel`), as the guide's HBM section prescribes; returns (bytes per launch | None, what was done)."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    child = [sys.executable, os.path.abspath(__file__), "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--no-ess", "--no-inlined", "--no-configs",
             "--no-live-traffic", "--chains-per-gpu", str(a.chains_per_gpu), "--rows", str(a.rows), "--leapfrog", str(a.leapfrog),
             "--rows-unroll", str(a.rows_unroll), "--engine", a.engine, "--grad-chains", str(a.grad_chains),
             "--grad-unroll", str(a.grad_unroll), "--grad-splits", str(a.grad_splits)]
    child += (["--strict"] if a.strict else []) + (["--no-factor"] if a.no_factor else [])
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_LIBRARY_CTOR"):
        env.pop(k, None)
    kb, n_used = {}, {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="rh_pmc_", dir="/tmp")
        try:
            r = subprocess.run([exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "bench", "--"] + child,
                               cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            files = glob.glob(os.path.join(d, "**", "bench_counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, "rocprofv3 --pmc %s failed (rc %d)" % (ctr, r.returncode)
            vals = [float(row["Counter_Value"]) for row in csv.DictReader(open(files[0]))
                    if row["Kernel_Name"] == kernel and row["Counter_Name"] == ctr]
            vals = vals[-64:]
            if not vals:
                return None, "no %s launch in the %s pass" % (kernel, ctr)
            kb[ctr], n_used[ctr] = sum(vals) / len(vals), len(vals)
        except (subprocess.TimeoutExpired, OSError, KeyError, ValueError) as e:
            return None, "rocprofv3 --pmc %s: %s" % (ctr, type(e).__name__)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return (kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024.0, (
        "measured in this run: two separate rocprofv3 --pmc passes (FETCH_SIZE %.0f KB | WRITE_SIZE %.0f KB per launch, means of the "
        "last %d launches of %s) over `bench.py --steps 4` of the same build" % (kb["FETCH_SIZE"], kb["WRITE_SIZE"], n_used["FETCH_SIZE"], kernel))


def side_run(w, R, models, rank, local_rank, world, dist, steps, warmup, cpg, rows=None, sampler="default", strict=False, model=None, spec=None,
             dump=None):
    """One of the other BASELINE.json configurations (the judged bench line is cfg 2), timed like the main leg: `warmup` untimed
    sampler warm-up iterations, then `steps` timed iterations + (N > 1) the one all-gather; returns the result dict on rank 0.
      cfg1 funnel 10-d, HMC L=5                                  (data-free, chain-per-wavefront engine)
      cfg3 eight schools, DefaultConfig EHMC(1024) or sampler = "nuts"   (data-free)
      cfg2d cfg 2's model under the reference's DefaultConfig (EHMC + DualAvg + windowed diagonal mass): the two-launch tick path
      cfg4 logistic GLM 50 covariates x rows (default 1e7), NUTS(10) + windowed diagonal mass, 256 chains/GPU
           (tick engine, fp64 MFMA GLM kernel)
      cfg5 hierarchical NegBin GLM, 10 000 groups x 100 obs, NUTS(10), 1024 chains/GPU (gather mode, HBM-resident state)
    Same launch contract as cfg 2: chains sharded by global id, one final all-gather of the draws when N > 1."""
    from rainier_amd import distributed as D
    fast = dict(fp_contract=not strict, factor_outputs=not strict)
    t_create = time.perf_counter()
    if w == "cfg1":
        spec = models.funnel(10); cfg = R.HMC(warmup, steps, 5); cfg.massMatrixTuner = lambda: R.IdentityMassMatrixTuner()
    elif w == "cfg3":
        spec = models.eight_schools(); cfg = R.make_config(steps, warmup)
    elif w == "cfg2d":
        spec = spec or models.linreg(n=rows or 1_000_000, k=3); cfg = R.make_config(steps, warmup)
    elif w == "cfg4":
        spec = spec or models.logistic(n=rows or 10_000_000, k=50); cfg = R.make_config(steps, warmup, R.NUTSSampler(10))
    else:   # rows scales the number of groups (100 observations each); the BASELINE size is 10 000 groups.  cfg5c: the CENTRED
        # parameterisation (alpha_g ~ Normal(mu, sigma) sampled directly) -- the form on which NUTS converges at this size
        # (tests/test_gpu_baseline_samplers.py: R-hat < 1.05; the non-centred one above keeps R-hat at 3-6 for any affordable length)
        mk = models.hier_negbin_centred if w == "cfg5c" else models.hier_negbin
        spec = spec or mk(10_000 if not rows else max(100, rows // 100), 100); cfg = R.make_config(steps, warmup, R.NUTSSampler(10))
    if w in ("cfg4", "cfg5", "cfg5c") and 90 <= warmup < 150:
        # ONE mass window early enough to leave DefaultConfig's 50 iterations of step-size adaptation behind it (skipLast = 50): what makes
        # the difference between trees of ~90 and ~9 leapfrog steps is less the number of draws in the window than whether the step size
        # has time to settle on the adapted mass (cfg 4, warm-up 100 with three windows ending at 84: tree 97; warm-up 150: 9)
        cfg.massMatrixTuner = lambda: R.DiagonalMassMatrixTuner(warmup - 70, 1.5, 20, 50)
    elif w in ("cfg4", "cfg5", "cfg5c") and 24 <= warmup < 90:
        # DefaultConfig's mass windows (50, x1.5, skip 50 / 50: sampler/Sampler.scala:24-25) never open in a warm-up this short:
        # the same tuner scaled to the leg's warm-up, so that "NUTS + diag mass-matrix adapt" (BASELINE cfg 4) really adapts
        k = warmup // 6
        cfg.massMatrixTuner = lambda: R.DiagonalMassMatrixTuner(k, 1.5, k, k)
    elif w in ("cfg4", "cfg5", "cfg5c") and warmup < 24:
        cfg.massMatrixTuner = lambda: R.IdentityMassMatrixTuner()   # (a kernel-speed leg of a few iterations: nothing to adapt from)
    if sampler == "nuts":
        cfg.sampler = lambda: R.NUTSSampler(10)
    elif sampler.startswith("hmc"):      # static HMC, L = the number behind "hmc": every chain asks for a gradient at every launch, so the
        L = int(sampler[3:])             # dominant kernel runs at full occupancy (the figure its roofline fraction is quoted on)
        cfg.sampler = lambda: R.HMCSampler(L)
    own = model is None
    if own:
        model = R.Model(spec, device=local_rank, **fast)
    t_create = time.perf_counter() - t_create
    s = R.Sampler(model, cfg, D.shard_seeds(2000, cpg, rank))
    t0 = time.perf_counter(); s.warmup(); tw = time.perf_counter() - t0
    s.timing(reset=True)
    comm = dist
    if comm is not None:
        comm.barrier(); D.device_synchronize(local_rank)
    t0 = time.perf_counter()
    s.run(steps)
    gathered = None
    if comm is not None:
        gathered = comm.rccl.allgather_draws(s, to_host=(rank == 0))     # RCCL all-gather over xGMI (rank 0: + copy to the host)
        D.device_synchronize(local_rank)
    dt = time.perf_counter() - t0
    stats, _ = s.stats()
    counts = [float(sum(st.leapfrogSteps for st in stats)), float(sum(st.warmupLeapfrogSteps for st in stats))]
    if comm is not None:
        dt = comm.rccl.allreduce_max(dt)
        counts = comm.sum(counts)
    tim = s.timing()
    nshow = min(spec.n_params, 16)
    draws = None
    if rank == 0:
        if comm is not None:
            draws = gathered[:, :, :nshow]
        else:   # the first `nshow` parameters of every draw, fetched a few iterations at a time (cfg 5: 10 004 parameters per draw)
            step_it = max(1, int(2.5e8 // max(1, cpg * spec.n_params)))
            draws = np.concatenate([s.draws(f, min(step_it, steps - f))[:, :, :nshow] for f in range(0, steps, step_it)], axis=1)
        if dump:
            dump_outputs(dump, gathered[:, -1, :] if comm is not None else s.draws(steps - 1, 1)[:, 0, :])
    s.close()
    if own:
        model.close()
    if rank != 0:
        return None
    nsteps, wsteps = counts
    diag = R.diagnostics(draws) if steps >= 4 and draws.shape[0] >= 2 else None
    ess = min(e for _, e in diag) if diag else None
    rhat_max = max(r for r, _ in diag) if diag else None
    converged = bool(rhat_max is not None and rhat_max < 1.05)
    out = {"metric": "leapfrog steps/sec (all chains)", "value": nsteps / dt, "unit": "leapfrog steps/s",
           "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": w + ": " + spec.name, "chains": cpg * world, "sampler": type(cfg.sampler()).__name__,
                      "mass": type(cfg.massMatrixTuner()).__name__, "engine": tim["dominant_kernel"], "strict": bool(strict)},
           "warmup_leapfrog_steps_per_s": wsteps / tw,
           # ESS/s (min over the first 16 parameters, Trace.diagnostics' formula) is quoted only for draws that have converged;
           # otherwise the figure is kept under another name with the R-hat that disqualifies it
           "ess_per_s": ess / dt if ess and converged else None, "rhat_max": rhat_max, "converged_rhat_below_1_05": converged,
           "ess_per_s_unconverged": ess / dt if ess and not converged else None,
           "leapfrog_steps_timed": nsteps, "seconds_timed": dt, "seconds_warmup": tw, "seconds_model_create": t_create,
           "mean_leapfrog_per_iteration": nsteps / (steps * cpg * world),
           "row_chain_evals_per_s": nsteps * spec.rows_streamed / dt if spec.rows_streamed else None}
    if spec.rows_streamed and tim["kernel_ms"] > 0:
        k_s = tim["kernel_ms"] / 1e3
        ab = tim["row_chain_evals"] * spec.bytes_per_row
        hbm = {"achieved": ab / k_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ab / k_s / 1e9 / HBM_PEAK_GBS}
        fpr = spec.meta.get("flops_per_row")
        if fpr:   # cfg 2 16, cfg 4 4K + 10 = 210, cfg 5 30 flop per row-chain eval.  The data set is read once per launch for
            # all chains of a workgroup column (cfg 4) or served from cache (cfg 2, cfg 5), so the fp64 pipe binds, not HBM (DESIGN 3.3,
            # 3.5); the HBM-equivalent figure is kept beside it
            fl = tim["row_chain_evals"] * fpr
            out["roofline"] = {"bound": "fp64_mfma" if "glm" in tim["dominant_kernel"] else "fp64_valu", "kernel": tim["dominant_kernel"],
                               "achieved": fl / k_s / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": fl / k_s / 1e12 / FP64_PEAK_TFLOPS,
                               "traffic": None, "launches": tim["launches"], "avg_launch_ms": tim["kernel_ms"] / max(1, tim["launches"]),
                               "all_kernels_ms": tim["total_ms"], "flops_per_row_chain_eval": fpr, "hbm_equivalent": hbm,
                               # the launches serve the chains that wait for a gradient (live-chain lists): slots served vs needed,
                               # and the same fraction over the launches that served >= 90 % of the chains (the run's tail excluded)
                               "chain_slots_served": tim["chain_slots"], "chain_slots_needed": tim["density_evals"],
                               "slot_efficiency": tim["density_evals"] / max(1, tim["chain_slots"]),
                               "steady_state": ({"launches": tim["steady_launches"], "avg_launch_ms": tim["steady_kernel_ms"] / tim["steady_launches"],
                                                 "frac": tim["steady_density_evals"] * spec.rows_streamed * fpr / (tim["steady_kernel_ms"] / 1e3) / 1e12 / FP64_PEAK_TFLOPS,
                                                 "what": "launches that served >= 90 % of the chains"} if tim["steady_launches"] else None)}
        else:
            out["roofline"] = dict(hbm, bound="hbm", kernel=tim["dominant_kernel"], traffic=None, launches=tim["launches"],
                                   avg_launch_ms=tim["kernel_ms"] / max(1, tim["launches"]),
                                   note="algorithmic bytes per row-chain eval x evals / kernel time: an HBM-EQUIVALENT rate (cache-resident "
                                        "data is re-read by every chain group), not memory-side traffic")
    else:
        out["roofline"] = None
        out["note"] = "data-free model: latency-bound, no HBM/MFMA roofline applies"
    return out


def side_workload(a, R, models, rank, local_rank, world, dist):
    """`--workload cfgN`: one of the other BASELINE.json configurations as the whole run (ONE JSON line on rank 0)."""
    w = a.workload
    cpg = a.chains_per_gpu if a.chains_per_gpu != 1024 or w not in ("cfg4",) else 256
    out = side_run(w, R, models, rank, local_rank, world, dist, a.steps, a.warmup, cpg, rows=None if a.rows == 1_000_000 else a.rows,
                   sampler=a.sampler, strict=a.strict, dump=a.dump_outputs)
    if rank == 0:
        print(json.dumps(out))


def all_configs(budget_s=600.0, long_legs=False):
    """The `configs` block of the default (N = 1) line: every BASELINE.json configuration driver-timed in this run, each leg a CHILD
    process (`bench.py --workload ...`, the same code path as `--workload` from the command line) under a watchdog, so that a leg
    that hangs or dies cannot take the judged cfg-2 line with it.  Sizes are the BASELINE ones.  The legs under the
    samplers BASELINE names (NUTS) and the reference defaults to (EHMC + windowed diagonal mass: sampler/Sampler.scala:17-27) carry
    the live-chain accounting of their gradient launches (roofline.slot_efficiency, roofline.steady_state) and print an ESS/s only
    beside R-hat < 1.05; the static-HMC legs are the dominant kernel's own figure (every launch serves every chain).
      The NUTS legs at BASELINE size converge once the mass windows are DefaultConfig's own (warm-up 150; round 6, GPU calls G / H): cfg 4
    then needs ~9 leapfrog steps per iteration instead of ~90 and runs 150 + 300 iterations in under three minutes -- the default.  cfg 5
    (centred form) spends ~6 minutes in the first 100 warm-up iterations (trees at depth 10, ~3 s each) before its trees drop from 1014
    to 31 steps: by default it runs 24 + 24 iterations (kernel-speed and steady-state figures; R-hat reported, ESS/s withheld while it
    is above 1.05), and `--long-configs` runs the converging 150 + 400 (profiles/r6_side/cfg5c_nuts_warmup150.json: R-hat 0.995)."""
    plan = [  # (key, workload, steps, warmup, chains, sampler, watchdog seconds)
        ("cfg1_funnel_hmc5_1024", "cfg1", 2000, 300, 1024, "default", 120),
        ("cfg3_eight_schools_ehmc_1024", "cfg3", 500, 300, 1024, "default", 120),
        ("cfg3_eight_schools_nuts10_1024", "cfg3", 200, 300, 1024, "nuts", 120),
        ("cfg2_default_config_ehmc_diag_mass_1024", "cfg2d", 256, 200, 1024, "default", 240),   # (256 iterations: the run's tail -- chains finishing at different launches -- is ~1/sqrt(n) of it)
        ("cfg4_logistic_1e7x50_hmc8_256", "cfg4", 2, 2, 256, "hmc8", 240),
        # (warm-up 150 = DefaultConfig's own mass windows 50 / x1.5 / 50 / 50: the adapted mass brings the mean tree from ~90 leapfrog steps --
        #  what a 60-iteration warm-up with windows of 10-22 draws leaves -- to ~9, and the 150 iterations cost what those 60 did;
        #  profiles/r6_side/cfg4_nuts_warmup{100,150}.json)
        ("cfg4_logistic_1e7x50_nuts10_diag_mass_256", "cfg4", 300, 150, 256, "default", 420),
        ("cfg5_hier_negbin_10000x100_hmc8_1024", "cfg5", 4, 2, 1024, "hmc8", 240),
        # (cfg 5 converges the same way -- warm-up 150: mean tree 1014 -> 31 leapfrog steps, R-hat 0.995 -- but ITS first 100 warm-up iterations
        #  run at depth 10, ~3 s each: 6 minutes of warm-up, which only --long-configs spends; profiles/r6_side/cfg5c_nuts_warmup150.json)
        ("cfg5_hier_negbin_centred_10000x100_nuts10_1024", "cfg5c", 400, 150, 1024, "default", 640) if long_legs else
        ("cfg5_hier_negbin_centred_10000x100_nuts10_1024", "cfg5c", 24, 24, 1024, "default", 300),
    ]
    out, t_all = {}, time.perf_counter()
    for key, w, steps, warm, cpg, smp, limit in plan:
        left = budget_s - (time.perf_counter() - t_all)
        if left < 30:
            out[key] = {"skipped": "the configs block's time budget (%.0f s) was spent" % budget_s}
            continue
        t0 = time.perf_counter()
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--workload", w, "--sampler", smp, "--steps", str(steps),
               "--warmup", str(warm), "--chains-per-gpu", str(cpg)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=min(limit, left))   # (N = 1, not under torch.distributed.run: the same device 0)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                out[key] = {"error": "exit code %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:])}
                continue
            d = json.loads(lines[-1])
            keep = {k: d.get(k) for k in ("value", "unit", "steps", "warmup", "ms_per_step", "config", "ess_per_s", "rhat_max", "converged_rhat_below_1_05",
                                          "ess_per_s_unconverged", "leapfrog_steps_timed", "seconds_timed", "seconds_warmup", "seconds_model_create",
                                          "mean_leapfrog_per_iteration", "row_chain_evals_per_s", "roofline")}
            keep["seconds_total"] = time.perf_counter() - t0
            out[key] = keep
        except subprocess.TimeoutExpired:
            out[key] = {"error": "watchdog: the leg did not finish within %.0f s" % min(limit, left)}
        except Exception as e:      # a side configuration must never take the judged line down with it
            out[key] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    return out


FULL_RUN_S = 600.0         # a `--full` run is to end within this many seconds ...
FULL_TAIL_S = 120.0        # ... of which the legs behind the `configs` block (gpu_inlined, cpu_baseline) take about this many


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64, help="timed HMC iterations (one step = one iteration of all chains)")
    ap.add_argument("--warmup", type=int, default=128,
                    help="untimed sampler warm-up iterations (step-size adaptation needs ~100 for a meaningful ESS/s)")
    ap.add_argument("--chains-per-gpu", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--leapfrog", type=int, default=32)
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure, everything that takes runs of its own: the ESS/s legs, roofline.traffic under rocprofv3, "
                         "the `configs` block, gpu_inlined and cpu_baseline (~8 minutes); each --no-* switch below drops one of them again")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ess", action="store_true", help="skip the two ESS/s legs (profiling runs)")
    ap.add_argument("--no-inlined", action="store_true", help="skip the gpu_inlined leg")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` block (the other BASELINE configurations, timed in-process at N = 1)")
    ap.add_argument("--long-configs", action="store_true", help="the two BASELINE-size NUTS legs of the `configs` block at 60 + 100 / 36 + 60 iterations (5.5 minutes each) instead of ~2.5 minutes each")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not measure roofline.traffic in this run (two short rocprofv3 --pmc child runs); the committed, "
                         "sha-guarded profile is quoted instead.  Always set when this command is itself being profiled")
    ap.add_argument("--ess-iters", type=int, default=2560,
                    help="timed draws per chain of the ESS legs: static HMC with L=32 resonates on this posterior; with DefaultConfig's "
                         "adapted diagonal mass R-hat = sqrt(1 + (tau - 1) / n) has tau - 1 ~ 42 iterations (stable from 1536 to 2560 "
                         "draws) and falls below 1.01 beyond ~2100 draws per chain")
    ap.add_argument("--ess-iters-identity", type=int, default=2560,
                    help="timed draws per chain of the identity-mass leg (it has a slow mode: R-hat 1.031 / 1.0136 / 1.0113 at 1536 / "
                         "5120 / 8192 draws -- the apparent tau keeps growing -- so it is reported, flagged, and not waited for)")
    ap.add_argument("--ess-multi", action="store_true", help="run the ESS legs on every rank at N > 1 too")
    ap.add_argument("--ess-warmup", type=int, default=384)
    ap.add_argument("--sampler", default="default",
                    help="side workloads only: 'nuts' = NUTSSampler(10) (extension) instead of the reference's EHMC; 'hmcN' = static HMC with N steps")
    ap.add_argument("--workload", choices=["cfg2", "cfg1", "cfg3", "cfg2d", "cfg4", "cfg5", "cfg5c"], default="cfg2",
                    help="cfg2 is the BASELINE metric's configuration (default); the others are the remaining BASELINE.json "
                         "configurations, timed for reference (see side_workload)")
    ap.add_argument("--strict", action="store_true",
                    help="JVM-faithful model arithmetic: no FMA contraction, outputs accumulated per row un-factored")
    ap.add_argument("--no-factor", action="store_true", help="keep FMA contraction but do not factor outputs")
    ap.add_argument("--rows-unroll", type=int, default=0)
    ap.add_argument("--engine", choices=["auto", "chain", "tick"], default="auto")
    ap.add_argument("--grad-chains", type=int, default=0)
    ap.add_argument("--grad-unroll", type=int, default=0)
    ap.add_argument("--grad-splits", type=int, default=0)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last timed iteration's draw of every chain to DIR/draws.npy (float64, "
                         "[chains][parameters], at most 64 MB: a fixed, seeded sample of the chains beyond that)")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:     # a plain run: the headline figure and what the timed steps themselves yield, nothing that runs beside them
        a.no_ess = a.no_live_traffic = a.no_configs = a.no_inlined = a.no_cpu_baseline = True
    return a


def main():
    t_run = time.perf_counter()
    a = parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import rainier_amd as R
    from rainier_amd import _capi, models
    from rainier_amd import distributed as D
    _capi.lib()                     # the engine (system ROCm runtime) is loaded BEFORE torch: one HIP runtime per process
    dist = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ:   # launched by torch.distributed.run: exercise the RCCL path
        os.environ.setdefault("NCCL_DEBUG", "WARN")   # keep RCCL's version banner off stdout: rank 0 prints ONE JSON line
        dist = HostGroup(rank, world, local_rank, D)
    if a.workload != "cfg2":
        side_workload(a, R, models, rank, local_rank, world, dist)
        if dist is not None:
            dist.close()
        return

    K, W, L = a.steps, a.warmup, a.leapfrog
    spec = models.linreg(n=a.rows, k=3)
    model = R.Model(spec, device=local_rank, fp_contract=not a.strict, rows_unroll=a.rows_unroll,
                    grad_chains=a.grad_chains, grad_unroll=a.grad_unroll,
                    factor_outputs=not (a.strict or a.no_factor))
    cpg = a.chains_per_gpu
    seeds = D.shard_seeds(1000, cpg, rank)     # seeds by GLOBAL chain id: results independent of the GPU count
    engine = {"auto": 0, "chain": 1, "tick": 2}[a.engine]
    engines = model.engines()                  # which engines the engine agrees to run for this build on this toolchain (rh_model_engines)

    def leg(iters, warm, mass_tuner=None):
        """One sampler run: `warm` untimed warm-up iterations, then `iters` timed ones + (N > 1) the ONE collective.
        Returns (seconds [max over ranks], all draws on rank 0, stats, timing)."""
        cfg = R.make_config(iters, warm, R.HMCSampler(L), R.DualAvgTuner(0.8), mass_tuner or R.IdentityMassMatrixTuner(), engine=engine,
                            gradSplits=a.grad_splits)
        s = R.Sampler(model, cfg, seeds)
        s.warmup()                      # untimed warm-up steps (incl. LeapFrog.initialize + step-size search)
        s.timing(reset=True)
        gathered = None
        if dist is not None:
            dist.barrier(); D.device_synchronize(local_rank)
        t0 = time.perf_counter()
        s.run(iters)                    # synchronises the engine stream
        if dist is not None:
            # the ONE collective: RCCL all-gather over xGMI; rank 0 also copies the gathered draws to the host (diagnostics)
            gathered = dist.rccl.allgather_draws(s, to_host=(rank == 0))
            D.device_synchronize(local_rank)
        dt = time.perf_counter() - t0
        if dist is not None:
            dt = dist.rccl.allreduce_max(dt)             # max over ranks
        tim = s.timing()
        stats, _ = s.stats()
        draws = (gathered if rank == 0 else None) if dist is not None else s.draws()
        s.close()
        return dt, draws, stats, tim

    dt, draws, stats, tim = leg(K, W)     # the timed region the contract defines: EXACTLY K steps after W warm-up steps
    steps_local = sum(st.leapfrogSteps for st in stats)
    assert steps_local == K * L * cpg, (steps_local, K, L, cpg)
    total_steps = steps_local * world
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, draws[:, -1, :])
    # ESS/s legs, independent of the driver's --steps/--warmup.  The chains start from N(0,1) draws and the posterior is 7e-4 wide:
    # they need a few hundred iterations to get there, and a static L=32 trajectory is ~5 periods of this posterior long, so a
    # chain's draws are strongly autocorrelated.  With DefaultConfig's adapted diagonal mass R-hat = sqrt(1 + (tau - 1) / n) has
    # tau - 1 ~ 42 (the same at 1536 and 2560 draws) and falls below 1.01 beyond ~2100 draws per chain: that leg is `ess_leg`, the
    # one `ess_per_s` quotes.  Under identity mass -- the steps/s configuration -- one direction mixes far more slowly (R-hat
    # 1.031 / 1.0136 / 1.0113 at 1536 / 5120 / 8192 draws: not a 1/n law), so `ess_leg_identity_mass` is reported and flagged, not
    # waited for.  The legs run at N = 1 only (every rank would repeat the same minute; --ess-multi forces them).  Trace.autocorrelation (core/Trace.scala:93-109) sums lags < min(n, 100).  Two configurations: the bench's (identity
    # mass) and DefaultConfig's windowed diagonal mass adaptation (sampler/Sampler.scala:24-25) with the same static L.
    ess_warm = max(W, a.ess_warmup)
    ess_runs = {}
    for name, mt, ess_iters in (("default_diag_mass", R.DiagonalMassMatrixTuner(50, 1.5, 50, 50), max(K, a.ess_iters)),
                                ("identity_mass", R.IdentityMassMatrixTuner(), max(K, a.ess_iters_identity))):
        if a.no_ess or (world > 1 and not a.ess_multi):
            break
        e_dt, e_draws, e_stats, _ = leg(ess_iters, ess_warm, mt)
        if rank == 0:
            diag = R.diagnostics(e_draws)
            ess_runs[name] = {
                "iterations": ess_iters, "warmup": ess_warm, "seconds": e_dt,
                "rhat": [float(r) for r, _ in diag], "ess": [float(e) for _, e in diag],
                "rhat_max": float(max(r for r, _ in diag)), "ess_min": float(min(e for _, e in diag)),
                "ess_per_s": float(min(e for _, e in diag)) / e_dt, "draws_total": int(e_draws.shape[0] * e_draws.shape[1]),
                "mean_accept_prob": float(np.mean([st.meanAcceptProb for st in e_stats])),
                "step_size_mean": float(np.mean([st.stepSize for st in e_stats])),
                "converged": bool(max(r for r, _ in diag) < 1.01)}
    if rank != 0:
        if dist is not None:
            dist.close()
        return

    rows = spec.rows_streamed
    value = total_steps / dt
    rce = value * rows
    dflt = ess_runs.get("default_diag_mass")
    # dominant kernel, this rank: HIP events recorded on the engine's stream around each launch
    k_s = tim["kernel_ms"] / 1e3
    algo_bytes = tim["row_chain_evals"] * spec.bytes_per_row          # 8*(K+1) = 32 B per row-chain eval
    achieved = algo_bytes / k_s / 1e9
    flops = tim["row_chain_evals"] * spec.meta["flops_per_row"]       # 4K+4 = 16 flop per row-chain eval
    src_sha = hashlib.sha256(model.hip_source.encode()).hexdigest()[:16]
    out = {
        "metric": "leapfrog steps/sec (all chains)", "value": value, "unit": "leapfrog steps/s",
        "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": dt / K * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "cfg2: linear regression 3 covariates x %d rows (un-inlined, streamed), static HMC L=%d, "
                               "%d chains/GPU, DualAvgTuner(0.8), identity mass" % (rows, L, cpg),
                   "chains": cpg * world, "rows": rows, "leapfrog_per_step": L, "fp_contract": not a.strict, "factor_outputs": not (a.strict or a.no_factor),
                   "engine": tim["dominant_kernel"], "grad_chains": a.grad_chains, "grad_unroll": a.grad_unroll,
                   "grad_splits": a.grad_splits, "generated_source_sha16": src_sha,
                   # (ABI 5: kernels the engine found unfit to run are replaced, never launched; empty `why` = nothing was)
                   "engines_usable": {k: engines[k] for k in ("chain", "tick", "density")}, "engines_why": engines["why"].strip(),
                   "compile_attempts": engines["compile_attempts"]},
        "row_chain_evals_per_s": rce, "grad_element_evals_per_s": rce * spec.n_params,
        # ESS/s = min over parameters of Trace.diagnostics' ESS, over the leg's wall time; quoted for the leg that converges: the
        # bench's model, chains, kernels and static L with DefaultConfig's windowed diagonal mass adaptation (Sampler.scala:24-25).
        # ess_leg_identity_mass is the steps/s configuration itself (identity mass), with its R-hat
        "ess_per_s": dflt["ess_per_s"] if dflt else None,
        "ess_leg": dict(dflt, mass="DiagonalMassMatrixTuner(50, 1.5, 50, 50) (DefaultConfig)",
                        note="separate sampler run (same model, seeds, kernels): untimed warm-up, then the timed draws; rhat_max < 1.01 "
                             "says the draws are usable; ess = Trace.diagnostics' formula per parameter") if dflt else None,
        "ess_leg_identity_mass": dict(ess_runs["identity_mass"], mass="identity",
                                      note="the steps/s configuration: a slowly mixing direction keeps R-hat above 1.01 at any "
                                           "affordable length (1.0113 at 8192 draws per chain), and Trace.diagnostics' ESS, which "
                                           "sums lags < 100, is optimistic for it") if "identity_mass" in ess_runs else None,
        "mean_accept_prob": float(np.mean([st.meanAcceptProb for st in stats])),
        # The kernel is fp64-compute-bound (the 32 MB data set is served from cache, HBM-side traffic is ~1e-3 of the
        # algorithmic bytes), so the binding roofline is the fp64 VALU pipe (the kernel issues v_fma_f64): 78.6 TFLOP/s.
        # 16 flop and 32 algorithmic bytes per row-chain eval; the HBM-equivalent figure is kept alongside.
        "roofline": {"bound": "fp64_valu", "kernel": tim["dominant_kernel"], "achieved": flops / k_s / 1e12, "peak": FP64_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": flops / k_s / 1e12 / FP64_PEAK_TFLOPS, "traffic": None,
                     "launches": tim["launches"], "all_kernels_ms": tim["total_ms"], "avg_launch_ms": tim["kernel_ms"] / max(1, tim["launches"]),
                     "algorithmic_flops_per_launch": flops / max(1, tim["launches"]),
                     "algorithmic_bytes_per_launch": algo_bytes / max(1, tim["launches"]),
                     "measured_issue_ceiling": {"frac_of_ceiling": flops / k_s / 1e12 / 59.6, "ceiling": 59.6, "unit": "TFLOP/s",
                                                "source": "profiles/r1_d_fp64_ceiling: 0.23 DP instr/cycle/SIMD at the sustained 2.2 GHz, 16 flop per 9 instructions"},
                     "hbm_equivalent": {"achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS}},
    }
    # HBM-side bytes per launch of the dominant kernel.  PMC counters cannot be read from inside the process, so this is
    # the committed summary of the separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes over this same
    # command (tools/pmc_cfg2.sh -> profiles/<round>/pmc_grad_kernel.json).  It is reported ONLY when that profile was
    # taken on byte-identical generated kernel source (sha of the model's HIP translation unit) and workload; otherwise
    # traffic stays null.  KB -> bytes; FETCH_SIZE is reported as collected (the guide's gfx950 x2 correction is calibrated
    # for 16 B/lane loads and these are 8 B/lane, so the read side is 1-2x this figure).
    prof = os.path.join(ROOT, "profiles", TRAFFIC_PROFILE)
    live = None
    profiled = bool(os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprofiler" in os.environ.get("LD_PRELOAD", ""))   # this run is under rocprofv3 itself
    if world == 1 and not a.no_live_traffic and not profiled:
        live, how = live_traffic(a, tim["dominant_kernel"])
        out["roofline"]["traffic_source"] = how
        if live is not None:
            out["roofline"]["traffic"] = live
        else:
            out["roofline"]["live_traffic_failed"] = how
    if live is None and os.path.exists(prof):
        pj = json.load(open(prof))
        same = pj.get("generated_source_sha16") == src_sha and pj.get("kernel") == tim["dominant_kernel"] and \
            pj.get("rows") == rows and pj.get("chains_per_gpu") == cpg
        if same:
            pc = pj["counters"]
            out["roofline"]["traffic"] = (pc["FETCH_SIZE"]["mean_per_launch"] + pc["WRITE_SIZE"]["mean_per_launch"]) * 1024.0
            out["roofline"]["traffic_source"] = "profiles/%s (separate rocprofv3 --pmc passes; git %s, generated source sha16 %s)" % (
                TRAFFIC_PROFILE, pj.get("git_head", "?"), src_sha)
        else:
            out["roofline"]["traffic_source"] = "none: profiles/%s was taken on different kernel source or workload (sha16 %s vs %s)" % (
                TRAFFIC_PROFILE, pj.get("generated_source_sha16"), src_sha)
    if not a.no_configs and world == 1 and dist is None:   # (started as `python bench.py --full`, not under torch.distributed.run)
        # (the default legs need ~5 minutes; they get what the run so far has left of FULL_RUN_S, so that a slow box skips a leg and says so)
        left = FULL_RUN_S - FULL_TAIL_S - (time.perf_counter() - t_run)
        out["configs"] = all_configs(budget_s=1100.0 if a.long_configs else min(600.0, left), long_legs=a.long_configs)
    if not a.no_inlined and world == 1:
        out["gpu_inlined"] = gpu_inlined(R, models, local_rank, L)
    if not a.no_cpu_baseline and world == 1:      # rank 0 at N = 1 only
        out["cpu_baseline"] = cpu_baseline(spec, L)
    print(json.dumps(out))
    if dist is not None:
        dist.close()


class HostGroup:
    """The host side of an N > 1 run: a torch.distributed *gloo* group (CPU only) for the bootstrap of the engine's RCCL
    communicator, the barriers and tiny host reductions; `rccl` is the engine's communicator (rh_comm)."""

    def __init__(self, rank, world, local_rank, D):
        D.device_synchronize(local_rank)   # this rank's device becomes the thread's current device before RCCL sees it
        mine = D.Comm.unique_id()       # every rank: loads the system RCCL now, BEFORE torch brings its bundled copy
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        dist.init_process_group("gloo")
        uid = D.exchange_unique_id(dist, lambda: mine, rank)
        self.rccl = D.Comm(uid, world, rank, local_rank)

    def barrier(self):
        self.dist.barrier()

    def sum(self, values):
        t = self.torch.tensor(values, dtype=self.torch.float64)
        self.dist.all_reduce(t)
        return t.tolist()

    def close(self):
        self.rccl.close()
        self.dist.destroy_process_group()


if __name__ == "__main__":
    main()
