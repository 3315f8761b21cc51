"""Host-side mirror of rainier-sampler's plugin surface over the C ABI (include/rainier_hip.h).

Same names, argument meaning and defaults as the reference (rainier-sampler/.../sampler/):
  SamplerConfig / DefaultConfig            Sampler.scala:3-27
  HMCSampler(nSteps), HMC(warmIt, it, n)   HMC.scala:3-33
  EHMCSampler(maxSteps, minSteps, bufSize, pCount), EHMC(...)   EHMC.scala:3-74
  DualAvgTuner(delta), StaticStepSize      DualAvg.scala:3-25, Sampler.scala:36-40
  IdentityMassMatrixTuner, DiagonalMassMatrixTuner(50,1.5,50,50), StaticMassMatrix   MassMatrix.scala:120-173
  DensityFunction { nVars, update, density, gradient }         DensityFunction.scala:3-8
  Model.sample(config, nChains) -> Trace; Trace.diagnostics    core/Model.scala:13-24, core/Trace.scala:11-21

All compute happens in librainier_hip.so on the GPU; this module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import RainierHipError  # noqa: F401  (re-export)


# ---- plugin classes (pure configuration, like the reference's) -------------------------------------
@dataclass
class HMCSampler:
    nSteps: int


@dataclass
class EHMCSampler:
    maxSteps: int
    minSteps: int = 1
    bufSize: int = 100
    pCount: float = 0.1


@dataclass
class NUTSSampler:
    """Extension (not in the reference): iterative multinomial NUTS behind the Sampler plugin point."""
    maxDepth: int = 10


@dataclass
class DualAvgTuner:
    delta: float


@dataclass
class StaticStepSize:
    stepSize: float


@dataclass
class IdentityMassMatrixTuner:
    pass


@dataclass
class DiagonalMassMatrixTuner:
    initialWindowSize: int = 50
    windowExpansion: float = 1.5
    skipFirst: int = 50
    skipLast: int = 50


@dataclass
class DenseMassMatrixTuner:
    """DenseMassMatrixTuner (MassMatrix.scala:175-181): CovarianceEstimator + packed Cholesky; at most 64 parameters."""
    initialWindowSize: int = 50
    windowExpansion: float = 1.5
    skipFirst: int = 50
    skipLast: int = 50


@dataclass
class DiagonalMassMatrix:
    elements: Sequence[float]

    def __post_init__(self):
        if any(float(x) == 0.0 for x in self.elements):   # require(!elements.contains(0.0)) MassMatrix.scala:8
            raise ValueError("requirement failed")


@dataclass
class StaticMassMatrix:
    mass: DiagonalMassMatrix


class SamplerConfig:
    """trait SamplerConfig (Sampler.scala:3-11); defaults = DefaultConfig (Sampler.scala:17-27)."""

    iterations = 1000
    warmupIterations = 1000
    statsWindow = 100
    engine = _capi.ENGINE_AUTO   # engine extension: device mapping (rh_engine_kind); not part of the reference trait
    gradSplits = 0

    def stepSizeTuner(self): return DualAvgTuner(0.8)
    def massMatrixTuner(self): return DiagonalMassMatrixTuner(50, 1.5, 50, 50)
    def sampler(self): return EHMCSampler(1024)


DefaultConfig = SamplerConfig


def make_config(iterations=1000, warmupIterations=1000, sampler=None, stepSizeTuner=None, massMatrixTuner=None,
                engine=_capi.ENGINE_AUTO, gradSplits=0):
    cfg = SamplerConfig()
    cfg.iterations, cfg.warmupIterations = iterations, warmupIterations
    cfg.engine, cfg.gradSplits = engine, gradSplits
    if sampler is not None: cfg.sampler = lambda: sampler
    if stepSizeTuner is not None: cfg.stepSizeTuner = lambda: stepSizeTuner
    if massMatrixTuner is not None: cfg.massMatrixTuner = lambda: massMatrixTuner
    return cfg


def HMC(warmIt: int, it: int, nSteps: int) -> SamplerConfig:          # HMC.scala:26-33
    return make_config(it, warmIt, sampler=HMCSampler(nSteps))


def EHMC(warmIt: int, it: int, minSteps: int = 1, numLengths: int = 100) -> SamplerConfig:  # EHMC.scala:64-74
    return make_config(it, warmIt, sampler=EHMCSampler(1000, minSteps, numLengths, 0.1))


def to_c_config(config: SamplerConfig, nvars: int):
    c = _capi.Config()
    _capi.lib().rh_config_default(C.byref(c))
    c.iterations, c.warmup = int(config.iterations), int(config.warmupIterations)
    c.engine, c.grad_splits = int(getattr(config, 'engine', 0)), int(getattr(config, 'gradSplits', 0))
    s, st, mt = config.sampler(), config.stepSizeTuner(), config.massMatrixTuner()
    keep = None
    if isinstance(s, HMCSampler):
        c.sampler, c.hmc_steps = _capi.SAMPLER_HMC, int(s.nSteps)
    elif isinstance(s, EHMCSampler):
        c.sampler = _capi.SAMPLER_EHMC
        c.ehmc_max_steps, c.ehmc_min_steps, c.ehmc_buf_size, c.ehmc_p_count = s.maxSteps, s.minSteps, s.bufSize, s.pCount
    elif isinstance(s, NUTSSampler):
        c.sampler, c.nuts_max_depth = _capi.SAMPLER_NUTS, int(s.maxDepth)
    else:
        raise TypeError("unsupported Sampler %r" % (s,))
    if isinstance(st, DualAvgTuner):
        c.step_tuner, c.dualavg_delta = _capi.STEP_DUALAVG, float(st.delta)
    elif isinstance(st, StaticStepSize):
        c.step_tuner, c.static_step = _capi.STEP_STATIC, float(st.stepSize)
    else:
        raise TypeError("unsupported StepSizeTuner %r" % (st,))
    if isinstance(mt, IdentityMassMatrixTuner):
        c.mass_tuner = _capi.MASS_IDENTITY
    elif isinstance(mt, DiagonalMassMatrixTuner):
        c.mass_tuner = _capi.MASS_DIAG_WINDOWED
        c.mass_init_window, c.mass_expansion = mt.initialWindowSize, mt.windowExpansion
        c.mass_skip_first, c.mass_skip_last = mt.skipFirst, mt.skipLast
    elif isinstance(mt, DenseMassMatrixTuner):
        c.mass_tuner = _capi.MASS_DENSE_WINDOWED
        c.mass_init_window, c.mass_expansion = mt.initialWindowSize, mt.windowExpansion
        c.mass_skip_first, c.mass_skip_last = mt.skipFirst, mt.skipLast
    elif isinstance(mt, StaticMassMatrix):
        keep = np.ascontiguousarray(mt.mass.elements, dtype=np.float64)
        assert keep.shape == (nvars,)
        c.mass_tuner, c.static_mass = _capi.MASS_STATIC_DIAG, _capi.dptr(keep)
    else:
        raise TypeError("unsupported MassMatrixTuner %r" % (mt,))
    return c, keep


# ---- model / density / trace ---------------------------------------------------------------------------
class DensityFunction:
    """trait DensityFunction (DensityFunction.scala:3-8) as built by Model.density() (core/Model.scala:38-50)."""

    def __init__(self, model: "Model"):
        self._m = model
        self.nVars = model.nVars
        self._out = np.zeros(self.nVars + 1)

    def update(self, vars: Sequence[float]) -> None:
        lp, g = self._m.density_batch(np.asarray(vars, dtype=np.float64).reshape(1, self.nVars))
        self._out[0], self._out[1:] = lp[0], g[0]

    @property
    def density(self) -> float: return float(self._out[0])
    def gradient(self, index: int) -> float: return float(self._out[index + 1])


@dataclass
class Stats:
    leapfrogSteps: int
    warmupLeapfrogSteps: int
    gradientEvaluations: int
    accepted: int
    meanAcceptProb: float
    stepSize: float
    bfmi: float = float("nan")   # Stats.bfmi (sampler/Stats.scala:14-16)


class Trace:
    """case class Trace(chains, mass, stats, model) (core/Trace.scala:6-9); chains [nChains][iterations][nVars]."""

    def __init__(self, chains: np.ndarray, mass: np.ndarray, stats: List[Stats]):
        self.chains, self.mass, self.stats = chains, mass, stats

    def diagnostics(self):
        """List of (rHat, effectiveSampleSize) per parameter -- Trace.diagnostics (core/Trace.scala:11-21)."""
        return diagnostics(self.chains)

    def thin(self, n: int) -> "Trace":
        """Trace.thin(n) (core/Trace.scala:23-32): every chain keeps the iterations with i % n == 0."""
        if int(n) < 1:
            raise ValueError("thin: n must be at least 1")
        return Trace(np.ascontiguousarray(self.chains[:, ::int(n), :]), self.mass, self.stats)

    def predict(self, requirements_rir: bytes, n_requirements: int, device: int = -1, math_mode: int = _capi.MATH_FAST) -> np.ndarray:
        """Trace.predict (core/Trace.scala:34-41) for a compiled requirements program: [nChains][iterations][n_requirements]."""
        return predict(requirements_rir, self.chains, n_requirements, device=device, math_mode=math_mode)


def diagnostics(chains: np.ndarray):
    ch = np.ascontiguousarray(chains, dtype=np.float64)
    m, n, k = ch.shape
    if m < 2:
        raise ValueError("requirement failed: diagnostics requires multiple chains")
    rhat, ess = np.zeros(k), np.zeros(k)
    _capi.check(_capi.lib().rh_diagnostics(_capi.dptr(ch), m, n, k, _capi.dptr(rhat), _capi.dptr(ess)))
    return list(zip(rhat.tolist(), ess.tolist()))


def _diag_result(rhat, ess, mean, var, moments):
    diag = list(zip(rhat.tolist(), ess.tolist()))
    return (diag, mean, var) if moments else diag


def diagnostics_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0,
                       count: Optional[int] = None, moments: bool = False):
    """Trace.diagnostics over a device buffer [chains][iterations][nvars] (a sampler's draws, Comm.allgather_draws(to_host=False)),
    computed where the draws are: the list of (rHat, effectiveSampleSize) over iterations [first, first + count); with moments
    also the pooled mean and Trace's v per parameter (sqrt(v / ess) = the Monte-Carlo standard error of the mean)."""
    count = int(iterations) - int(first) if count is None else int(count)
    rhat, ess, mean, var = (np.zeros(nvars) for _ in range(4))
    _capi.check(_capi.lib().rh_diagnostics_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count,
                                                  _capi.dptr(rhat), _capi.dptr(ess), _capi.dptr(mean), _capi.dptr(var)))
    return _diag_result(rhat, ess, mean, var, moments)


def predict(requirements_rir: bytes, draws: np.ndarray, n_requirements: int, device: int = -1,
            math_mode: int = _capi.MATH_FAST) -> np.ndarray:
    """Trace.predict's compiled part (core/Trace.scala:34-41, core/Generator.scala:59-94): evaluate the requirements
    program for every draw on the device.  draws [..., nVars] -> [..., n_requirements]."""
    d = np.ascontiguousarray(draws, dtype=np.float64)
    flat = d.reshape(-1, d.shape[-1])
    out = np.zeros((flat.shape[0], n_requirements))
    blob = C.create_string_buffer(requirements_rir, len(requirements_rir))
    opts = _capi.compile_opts(device, math_mode)
    _capi.check(_capi.lib().rh_requirements_eval(blob, len(requirements_rir), C.byref(opts), _capi.dptr(flat), flat.shape[0], _capi.dptr(out)))
    return out.reshape(d.shape[:-1] + (n_requirements,))


class Predictor:
    """rh_predict: a requirements program (Generator.prepare's compiled part, core/Generator.scala:59-94) compiled once for one
    device, for Trace.predict over draws that stay there: Sampler.predict, predict_device, Comm.predict."""

    def __init__(self, requirements_rir: bytes, device: int = -1, math_mode: int = _capi.MATH_FAST, fp_contract: bool = False):
        self._h = C.c_void_p()
        blob = C.create_string_buffer(requirements_rir, len(requirements_rir))
        opts = _capi.compile_opts(device, math_mode, fp_contract)
        _capi.check(_capi.lib().rh_predict_create(blob, len(requirements_rir), C.byref(opts), C.byref(self._h)))
        self.nreq = _capi.lib().rh_predict_nreq(self._h)
        self.nvars = _capi.lib().rh_predict_nvars(self._h)

    def close(self):
        if self._h:
            _capi.lib().rh_predict_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def _kept(count: int, thin: int) -> int:
    return max(0, -(-int(count) // max(1, int(thin))))


def _predict_result(call, predictor, chains, count, thin, device, to_host, diagnostics, model=None):
    """shared by Sampler.predict and predict_device: call(host_out or None, byref(dev_out)) -> rc"""
    kept = _kept(count, thin)
    out = np.zeros((chains, kept, predictor.nreq)) if to_host else None
    ptr = C.c_void_p()
    _capi.check(call(_capi.dptr(out) if to_host else None, C.byref(ptr)), model)
    values = out if to_host else ptr.value
    if not diagnostics:
        return values
    # the handle's output buffer has rh_diagnostics_device's layout [chains][kept][nreq]: analysed where it is, no copy
    diag, mean, var = diagnostics_device(ptr.value, chains, kept, predictor.nreq, device=device, moments=True)
    return values, diag, mean, var


def predict_device(predictor: Predictor, ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0,
                   count: Optional[int] = None, thin: int = 1, to_host: bool = True, diagnostics: bool = False):
    """Trace.predict (with Trace.thin applied to the window) over a device buffer [chains][iterations][nvars]: the kept iterations
    are first + j * thin.  Returns [chains][kept][nreq] (to_host = False: the device pointer of the predictor's own buffer, valid
    until its next call); with diagnostics = True (values, diag, mean, var) of the predictions."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda host, dev: _capi.lib().rh_predict_device(predictor._h, C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars),
                                                           int(first), count, int(thin), host, dev)
    return _predict_result(call, predictor, int(chains), count, thin, int(device), to_host, diagnostics)


class gen:
    """Op constructors of a Generator's table (rh_gen_op): the reference's generators that Trace.predict accepts as a Distribution
    (core/Trace.scala:34-41, core/Generator.scala:171-174).  Each argument is a gen.col(i) -- column i of the per-draw parameter
    buffer, e.g. requirement i of a predictor -- or a float.  Uniform(from, to) passes the kernel scale = to - from and
    Exponential(rate) passes 1 / rate, which this front end computes only from floats: with columns the caller supplies the SCALE
    column itself (Uniform(from, scale_column), Exponential(scale_column)), e.g. as one more requirement of the predictor.
    The composites -- BetaBinomial, Mixture, ZeroInflated -- return LISTS of ops (hidden ops, guards and gen.PREV arguments:
    csrc/device/rh_generate_ext.hip.h), which Generator flattens; each adds ONE output column, its last op's.  A mixture's weights are
    m consecutive columns of the caller's, like every other column: e.g. m more requirements of the predictor."""

    class col(NamedTuple):
        index: int

    class _Prev:
        def __repr__(self): return "gen.PREV"
    PREV = _Prev()   # as an argument: the value of the op before this one in the same draw (RH_GEN_ARG_PREV)

    @staticmethod
    def _arg(x) -> "_capi.GenArg":
        if x is gen.PREV:
            return _capi.GenArg(-1, _capi.GEN_ARG_PREV, 0.0)
        return _capi.GenArg(int(x.index), 0, 0.0) if isinstance(x, gen.col) else _capi.GenArg(-1, 0, float(x))

    @staticmethod
    def _op(family, a, b=0.0) -> "_capi.GenOp":
        return _capi.GenOp(family, 0, gen._arg(a), gen._arg(b))

    @staticmethod
    def Real(a): return gen._op(_capi.GEN_REAL, a)                                      # Generator.scala:119-122
    @staticmethod
    def Normal(location, scale): return gen._op(_capi.GEN_NORMAL, location, scale)     # Continuous.scala:63-67
    @staticmethod
    def Cauchy(location, scale): return gen._op(_capi.GEN_CAUCHY, location, scale)     # :72-77
    @staticmethod
    def Laplace(location, scale): return gen._op(_capi.GEN_LAPLACE, location, scale)   # :82-89
    @staticmethod
    def LogNormal(location, scale): return gen._op(_capi.GEN_LOGNORMAL, location, scale)   # :194-197
    @staticmethod
    def Gamma(shape, scale): return gen._op(_capi.GEN_GAMMA, shape, scale)             # :94-147
    @staticmethod
    def Beta(a, b): return gen._op(_capi.GEN_BETA, a, b)                                # :163-176
    @staticmethod
    def Bernoulli(p): return gen._op(_capi.GEN_BERNOULLI, p)                            # Discrete.scala:38-48
    @staticmethod
    def Geometric(p): return gen._op(_capi.GEN_GEOMETRIC, p)                            # :59-69
    @staticmethod
    def Poisson(lam): return gen._op(_capi.GEN_POISSON, lam)                            # :122-186

    @staticmethod
    def Uniform(from_, to):                                                             # Continuous.scala:202-215
        """to: a float with a float `from_` (scale = to - from_); with a column on either side `to` IS the scale: float or column"""
        if isinstance(from_, gen.col) or isinstance(to, gen.col):
            return gen._op(_capi.GEN_UNIFORM, from_, to)
        return gen._op(_capi.GEN_UNIFORM, from_, float(to) - float(from_))

    @staticmethod
    def Exponential(rate):                                                              # Continuous.scala:152-158
        """rate: a float (scale = 1 / rate); a column is taken as the SCALE 1 / rate itself"""
        return gen._op(_capi.GEN_GAMMA, 1.0, rate if isinstance(rate, gen.col) else 1.0 / float(rate))

    # ---- the count families and the composites (csrc/device/rh_generate_ext.hip.h)
    @staticmethod
    def Binomial(p, k): return gen._op(_capi.GEN_BINOMIAL, p, k)                        # Discrete.scala:194-230
    @staticmethod
    def NegativeBinomial(p, n): return gen._op(_capi.GEN_NEGBINOMIAL, p, n)             # :81-109

    @staticmethod
    def Categorical(first_col, m):                                                      # Generator.scala:129-141
        """the index (0 .. m - 1) drawn with the weights in the m consecutive columns from first_col (a gen.col or an int)"""
        first = first_col if isinstance(first_col, gen.col) else gen.col(int(first_col))
        return gen._op(_capi.GEN_CATEGORICAL, first, int(m))

    @staticmethod
    def _copy(op, guard=None, hidden=None) -> "_capi.GenOp":
        out = _capi.GenOp.from_buffer_copy(bytes(op))
        if guard is not None:
            out.reserved = (out.reserved & ~0xff) | int(guard)
        if hidden is not None:
            out.reserved = (out.reserved | _capi.GEN_OP_HIDDEN) if hidden else (out.reserved & ~_capi.GEN_OP_HIDDEN)
        return out

    @staticmethod
    def hidden(op):
        """the op with RH_GEN_OP_HIDDEN: it runs on the draw's stream, its value is not an output column"""
        return gen._copy(op, hidden=True)

    @staticmethod
    def BetaBinomial(a, b, k):                                                          # Discrete.scala:240-244
        """Beta(a, b).generator.flatMap(p => Binomial(p, k).generator): two ops, one column"""
        return [gen.hidden(gen.Beta(a, b)), gen.Binomial(gen.PREV, k)]

    @staticmethod
    def Mixture(first_col, components):                                                 # Discrete.scala:270-273, Continuous.scala's Mixture
        """Generator.categorical(components).flatMap(_.generator): the weights are the len(components) consecutive columns from
        first_col, in the components' order; a component is an op, a composite's list of ops, or a float (gen.Real).  One column."""
        comps = [[gen.Real(c)] if isinstance(c, (int, float)) else (list(c) if isinstance(c, (list, tuple)) else [c]) for c in components]
        if any(op.family == _capi.GEN_CATEGORICAL or (op.reserved & 0xff) for comp in comps for op in comp):
            raise ValueError("gen.Mixture: a component may not be a mixture itself")
        if any(not comp for comp in comps):
            raise ValueError("gen.Mixture: an empty component")
        ops = [gen.hidden(gen.Categorical(first_col, len(comps)))]
        for j, comp in enumerate(comps):
            ops += [gen._copy(op, guard=j + 1, hidden=True) for op in comp]
        ops[-1] = gen._copy(ops[-1], hidden=False)   # skipped ops pass the carry on: the last op's column is the sample in every draw
        return ops

    @staticmethod
    def ZeroInflated(first_col, component):                                             # Discrete.zeroInflated
        """0 with the weight in column first_col (psi), `component` with the weight in the next column (1 - psi, the caller's)"""
        return gen.Mixture(first_col, [gen.Real(0.0), component])


class Generator:
    """rh_generate: a table of gen.* ops over `nin` per-draw parameter columns, for posterior-predictive samples of draws that stay on
    the device (Sampler.generate, generate_device).  Output o of a draw is op o's sample; every draw has a java.util.Random stream
    of its own and runs its ops left to right on it.  flags: GEN_F_DOMAIN | GEN_F_CAP of the last call (NaN samples mark the draws).
    An entry of `ops` may be a composite's list of ops (gen.BetaBinomial, gen.Mixture, gen.ZeroInflated): one level of nesting is
    flattened.  nout counts the visible ops: one column per plain op and per composite."""

    def __init__(self, ops, nin: int, device: int = -1):
        self._h = C.c_void_p()
        ops = [op for entry in ops for op in (entry if isinstance(entry, (list, tuple)) else [entry])]
        arr = (_capi.GenOp * max(1, len(ops)))(*ops)
        _capi.check(_capi.lib().rh_generate_create(arr, len(ops), int(nin), int(device), C.byref(self._h)))
        self.nin = int(nin)
        self.nout = _capi.lib().rh_generate_nout(self._h)
        self.flags = 0

    def close(self):
        if self._h:
            _capi.lib().rh_generate_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def _generate_result(call, generator, chains, kept, to_host, model=None):
    """shared by Sampler.generate and generate_device: call(host_out or None, byref(dev_out), byref(flags)) -> rc"""
    out = np.zeros((chains, kept, generator.nout)) if to_host else None
    ptr, flags = C.c_void_p(), C.c_int32(0)
    _capi.check(call(_capi.dptr(out) if to_host else None, C.byref(ptr), C.byref(flags)), model)
    generator.flags = int(flags.value)
    return out if to_host else ptr.value


def generate_device(generator: Generator, ptr: int, chains: int, kept: int, nin: int, seed: int, chain0: int = 0, device: int = 0,
                    to_host: bool = True):
    """Posterior-predictive samples over a device buffer [chains][kept][nin] of per-draw distribution parameters (a predictor's
    to_host = False result): draw r = c * kept + j samples on the stream of global draw chain0 * kept + r, so a shard whose first
    chain is chain0 draws what the whole run would.  Returns [chains][kept][nout] (to_host = False: the device pointer of the
    generator's own buffer, valid until its next call -- what summary_device / diagnostics_device take)."""
    call = lambda host, dev, fl: _capi.lib().rh_generate_device(generator._h, C.c_void_p(ptr), int(device), int(chains), int(kept), int(nin),
                                                                int(seed), int(chain0), host, dev, fl)
    return _generate_result(call, generator, int(chains), int(kept), to_host)


class Summary(NamedTuple):
    """precis / hdpi of every parameter (rainier-notebook package.scala:327-342, 367-418): mean [nvars], sd [nvars] (population
    form), quantiles [nvars][nprobs] (the order statistics at floor(N * q)), hdpi [nvars][2] (None when not asked for), and the
    probabilities they were asked at."""
    mean: np.ndarray
    sd: np.ndarray
    quantiles: np.ndarray
    hdpi: Optional[np.ndarray]
    probs: Tuple[float, ...] = (0.055, 0.945)
    hdpi_prob: Optional[float] = 0.89


def _summary_result(call, nvars, probs, hdpi, model=None):
    """shared by Sampler.summary and summary_device: call(probs, nprobs, hdpi_prob, mean, sd, quantiles, hdpi) -> rc"""
    pr = np.ascontiguousarray([float(q) for q in probs], dtype=np.float64)
    mean, sd, quant, hd = np.zeros(nvars), np.zeros(nvars), np.zeros((nvars, len(pr))), np.zeros((nvars, 2))
    hp = 0.0 if hdpi is None else float(hdpi)
    _capi.check(call(_capi.dptr(pr), len(pr), hp, _capi.dptr(mean), _capi.dptr(sd), _capi.dptr(quant), _capi.dptr(hd)), model)
    asked = hp > 0.0
    return Summary(mean, sd, quant, hd if asked else None, tuple(pr.tolist()), hp if asked else None)


def summary_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
                   thin: int = 1, probs: Sequence[float] = (0.055, 0.945), hdpi: Optional[float] = 0.89) -> Summary:
    """precis' figures and hdpi over a device buffer [chains][iterations][nvars] (a sampler's draws, a predictor's to_host = False
    result, Comm.allgather_draws(to_host=False)), computed where the draws are (rh_summary_device): every parameter's pooled column
    over the kept iterations first + j * thin is sorted on the device.  hdpi = None: no highest-density interval."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_summary_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count,
                                                    int(thin), *a)
    return _summary_result(call, int(nvars), probs, hdpi)


class Covariance(NamedTuple):
    """How the parameters move together: mean [K], cov [K][K] (the pooled sample covariance of the kept draws, divisor N - 1 as in
    MassMatrixEstimator.scala:38-47), corr [K][K] (None when not asked for; the diagonal is 1.0, or NaN for a column without
    variance) and the columns they are about (parameter cols[k] is row and column k)."""
    mean: np.ndarray
    cov: np.ndarray
    corr: Optional[np.ndarray]
    cols: Tuple[int, ...]


def _covariance_result(call, nvars, cols, corr, model=None):
    """shared by Sampler.covariance and covariance_device: call(cols, ncols, mean, cov, corr) -> rc"""
    sel = None if cols is None else np.ascontiguousarray([int(c) for c in cols], dtype=np.int32)
    k = int(nvars) if sel is None else len(sel)
    mean, cov, cr = np.zeros(k), np.zeros((k, k)), np.zeros((k, k)) if corr else None
    buf = sel if sel is None or k else np.zeros(1, dtype=np.int32)       # an empty list is a list (refused), not "all columns"
    _capi.check(call(buf.ctypes.data_as(C.POINTER(C.c_int32)) if sel is not None else None, k if sel is not None else 0, _capi.dptr(mean),
                     _capi.dptr(cov), _capi.dptr(cr) if corr else None), model)
    return Covariance(mean, cov, cr, tuple(range(k)) if sel is None else tuple(sel.tolist()))


def covariance_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
                      thin: int = 1, cols: Optional[Sequence[int]] = None, corr: bool = False) -> Covariance:
    """The pooled sample covariance (and, with corr = True, the correlation) of the kept iterations first + j * thin over a device
    buffer [chains][iterations][nvars] (a sampler's draws, a predictor's to_host = False result, Comm.allgather_draws(to_host=False)),
    computed where the draws are (rh_covariance_device); cols: the parameters asked for, in the result's order (None: all)."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_covariance_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count,
                                                       int(thin), *a)
    return _covariance_result(call, nvars, cols, corr)


class Histogram(NamedTuple):
    """The shape of single parameters (the reference's density(seq, bounds), rainier-notebook package.scala:63-77): for column k
    (parameter cols[k]) edges [K][nbins + 1], counts [K][nbins] (int64; bin b holds edges[b] <= x < edges[b + 1], the last bin is
    closed), and the rows that are in no bin: under [K] (x < edges[0], -inf too), over [K] (x > edges[nbins], +inf too), nan [K]."""
    cols: Tuple[int, ...]
    edges: np.ndarray
    counts: np.ndarray
    under: np.ndarray
    over: np.ndarray
    nan: np.ndarray

    @property
    def density(self) -> np.ndarray:
        """counts / (counts.sum(axis=1) * widths): np.histogram(..., density=True); a zero-width bin gives NaN"""
        with np.errstate(invalid="ignore", divide="ignore"):
            dens = self.counts / (self.counts.sum(axis=1, keepdims=True) * np.diff(self.edges, axis=1))
        return np.where(np.diff(self.edges, axis=1) == 0.0, np.nan, dens)


class Histogram2d(NamedTuple):
    """The joint shape of pairs of parameters (the reference's scatter / contour, rainier-notebook package.scala:79-98): for pair p
    = (a, b) xedges [P][nbx + 1], yedges [P][nby + 1], grid [P][nbx][nby] (int64; the rows whose a falls in bin bx and whose b falls
    in bin by) and outside [P] (the rows with a coordinate out of range or NaN)."""
    pairs: Tuple[Tuple[int, int], ...]
    xedges: np.ndarray
    yedges: np.ndarray
    grid: np.ndarray
    outside: np.ndarray

    @property
    def density(self) -> np.ndarray:
        """grid / (grid.sum() * bin areas) per pair: np.histogram2d(..., density=True); a zero-area bin gives NaN"""
        area = np.diff(self.xedges, axis=1)[:, :, None] * np.diff(self.yedges, axis=1)[:, None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            dens = self.grid / (self.grid.sum(axis=(1, 2), keepdims=True) * area)
        return np.where(area == 0.0, np.nan, dens)


def _depth(r):
    """nesting depth of bounds as written: a number or None 0, (lo, hi) 1, ((xlo, xhi), (ylo, yhi)) 2, a list of those one more
    (a None stands for any entry, so the deepest entry decides)"""
    if isinstance(r, np.ndarray):
        return r.ndim
    if not isinstance(r, (list, tuple)):
        return 0
    return 1 + max((_depth(ri) for ri in r), default=0)


def _bounds(r, unit):
    """one entry's bounds -> a float64 array of shape `unit` ((2,) or (2, 2)); None, at any level: automatic (NaN)"""
    if r is None:
        return np.full(unit, np.nan)
    if len(r) != unit[0]:
        raise ValueError("bounds are (lo, hi)%s" % (" per axis" if len(unit) == 2 else ""))
    if len(unit) == 1:
        return np.array([np.nan if v is None else float(v) for v in r])
    return np.stack([_bounds(ri, unit[1:]) for ri in r])


def _range_arg(rng, shape, what):
    """None, one set of bounds for every entry, or one per entry (None: automatic) -> a float64 array of `shape` or None.  Which
    of the two it is is read from the nesting depth, never from the lengths: bounds as deep as one entry's ((lo, hi); for pairs
    ((xlo, xhi), (ylo, yhi))) hold for all entries, one level more is a list with one set per entry.  So with two columns
    [(0, 1), (2, 3)] is one set per column and (0, 1) is one set for both; a list of nothing but None is written None."""
    if rng is None:
        return None
    unit = shape[1:]
    if isinstance(rng, np.ndarray) and rng.dtype != object:      # an array holds no None: its shape says it all
        if rng.shape != unit and rng.shape != shape:
            raise ValueError("%s: a range array has the shape of one entry's bounds %s or of all entries' %s" % (what, unit, shape))
        return np.ascontiguousarray(np.broadcast_to(rng, shape), dtype=np.float64)
    depth = _depth(rng)
    if depth == len(unit):
        a = np.broadcast_to(_bounds(rng, unit), shape)
    elif depth == len(unit) + 1:
        if len(rng) != shape[0]:
            raise ValueError("%s: range holds %d sets of bounds for %d entries" % (what, len(rng), shape[0]))
        a = np.stack([_bounds(r, unit) for r in rng])
    else:
        raise ValueError("%s: range must be bounds for all entries or a list with one set per entry" % what)
    return np.ascontiguousarray(a, dtype=np.float64)


def _histogram_result(call, nvars, cols, bins, rng, model=None):
    """shared by Sampler.histogram and histogram_device: call(cols, ncols, nbins, range, edges, counts, under, over, nan) -> rc"""
    sel = None if cols is None else np.ascontiguousarray([int(c) for c in cols], dtype=np.int32)
    k, nb = int(nvars) if sel is None else len(sel), int(bins)
    r = _range_arg(rng, (k, 2), "histogram")
    edges, counts = np.zeros((k, max(nb, 0) + 1)), np.zeros((k, max(nb, 0)), dtype=np.int64)
    under, over, nan = (np.zeros(k, dtype=np.int64) for _ in range(3))
    buf = sel if sel is None or k else np.zeros(1, dtype=np.int32)       # an empty list is a list (refused), not "all columns"
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    _capi.check(call(buf.ctypes.data_as(C.POINTER(C.c_int32)) if sel is not None else None, k if sel is not None else 0, nb,
                     _capi.dptr(r) if r is not None else None, _capi.dptr(edges), lp(counts), lp(under), lp(over), lp(nan)), model)
    return Histogram(tuple(range(k)) if sel is None else tuple(sel.tolist()), edges, counts, under, over, nan)


def _histogram2d_result(call, pairs, bins, rng, model=None):
    """shared by Sampler.histogram2d and histogram2d_device: call(pairs, npairs, nbx, nby, range, xedges, yedges, grid, outside) -> rc"""
    pr = np.ascontiguousarray([[int(a), int(b)] for a, b in pairs], dtype=np.int32).reshape(-1, 2)
    p = len(pr)
    nbx, nby = (int(bins), int(bins)) if np.ndim(bins) == 0 else (int(bins[0]), int(bins[1]))
    r = _range_arg(rng, (p, 2, 2), "histogram2d")
    xe, ye = np.zeros((p, max(nbx, 0) + 1)), np.zeros((p, max(nby, 0) + 1))
    grid, outside = np.zeros((p, max(nbx, 0), max(nby, 0)), dtype=np.int64), np.zeros(p, dtype=np.int64)
    buf = pr if p else np.zeros((1, 2), dtype=np.int32)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    _capi.check(call(buf.ctypes.data_as(C.POINTER(C.c_int32)), p, nbx, nby, _capi.dptr(r) if r is not None else None, _capi.dptr(xe),
                     _capi.dptr(ye), lp(grid), lp(outside)), model)
    return Histogram2d(tuple((int(a), int(b)) for a, b in pr), xe, ye, grid, outside)


class RankDiagnostics(NamedTuple):
    """Rank-normalised split R-hat, bulk and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) per selected column.
    rhat = max(rhat_bulk, rhat_folded) (NaN where either is); truncated: bit 0 bulk, bit 1 lower tail, bit 2 upper tail -- where a bit
    is set the lags ran out at 255 before the autocorrelations did and that ESS is an upper bound."""
    rhat: np.ndarray
    rhat_bulk: np.ndarray
    rhat_folded: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    truncated: np.ndarray
    cols: Tuple[int, ...]


def _rank_result(call, nvars, cols, model=None):
    """shared by Sampler.rank_diagnostics and rank_diagnostics_device: call(cols, ncols, rhat_bulk, rhat_folded, ess_bulk, ess_tail, truncated) -> rc"""
    sel = None if cols is None else np.ascontiguousarray([int(c) for c in cols], dtype=np.int32)
    k = int(nvars) if sel is None else len(sel)
    rb, rf, eb, et = (np.zeros(max(k, 1)) for _ in range(4))
    tr = np.zeros(max(k, 1), dtype=np.int32)
    buf = sel if sel is None or k else np.zeros(1, dtype=np.int32)       # an empty list is a list (refused), not "all columns"
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _capi.check(call(ip(buf) if sel is not None else None, k if sel is not None else 0, _capi.dptr(rb), _capi.dptr(rf), _capi.dptr(eb),
                     _capi.dptr(et), ip(tr)), model)
    rb, rf, eb, et, tr = rb[:k], rf[:k], eb[:k], et[:k], tr[:k]
    rhat = np.where(np.isnan(rb) | np.isnan(rf), np.nan, np.maximum(rb, rf))
    return RankDiagnostics(rhat, rb, rf, eb, et, tr, tuple(range(k)) if sel is None else tuple(sel.tolist()))


def rank_diagnostics_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
                            cols: Optional[Sequence[int]] = None) -> RankDiagnostics:
    """Rank-normalised split R-hat, bulk ESS and tail ESS over the window [first, first + count) (count >= 4, each chain split in two
    halves) of a device buffer [chains][iterations][nvars] (a sampler's draws, a predictor's to_host = False result,
    Comm.allgather_draws(to_host=False)), computed where the draws are (rh_rank_diagnostics_device).  cols: the parameters asked for,
    in the result's order (None: all).  diagnostics_device keeps the reference's unsplit R-hat and variogram ESS."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_rank_diagnostics_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count, *a)
    return _rank_result(call, nvars, cols)


class Mcse(NamedTuple):
    """Monte Carlo standard errors and effective sample sizes of the reported figures (Vehtari et al. 2021, section 4) per selected
    column: how many digits of mean, sd and quantile [K][nprobs] survive the Monte Carlo error.  mcse_sd is the delta method's (the
    `posterior` package's form); mcse_quantile half the distance of the order statistics at the 16 % and 84 % points of
    Beta(ess p + 1, ess (1 - p) + 1); acf [K][nlags + 1] the autocorrelations of the values (NaN beyond lag min(h - 1, 255));
    truncated: bit 0 mean, bit 1 sd, bit 2 the squares behind mcse_sd, bit 3 + k quantile k -- where a bit is set the lags ran out at
    255 before the autocorrelations did and that ESS is an upper bound."""
    mean: np.ndarray
    sd: np.ndarray
    ess_mean: np.ndarray
    ess_sd: np.ndarray
    mcse_mean: np.ndarray
    mcse_sd: np.ndarray
    quantile: np.ndarray
    ess_quantile: np.ndarray
    mcse_quantile: np.ndarray
    acf: np.ndarray
    truncated: np.ndarray
    cols: Tuple[int, ...]
    probs: Tuple[float, ...]


def _mcse_result(call, nvars, cols, probs, nlags, model=None):
    """shared by Sampler.mcse and mcse_device: call(cols, ncols, probs, nprobs, nlags, the ten double outputs, truncated) -> rc"""
    sel = None if cols is None else np.ascontiguousarray([int(c) for c in cols], dtype=np.int32)
    k = int(nvars) if sel is None else len(sel)
    pr = np.ascontiguousarray([float(p) for p in probs], dtype=np.float64)
    npr, nl = len(pr), int(nlags)
    kk = max(k, 1)
    six = [np.zeros(kk) for _ in range(6)]
    three = [np.zeros((kk, npr)) for _ in range(3)]
    acf = np.zeros((kk, max(nl, 0) + 1))
    tr = np.zeros(kk, dtype=np.int32)
    buf = sel if sel is None or k else np.zeros(1, dtype=np.int32)       # an empty list is a list (refused), not "all columns"
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _capi.check(call(ip(buf) if sel is not None else None, k if sel is not None else 0, _capi.dptr(pr) if npr else None, npr, nl,
                     *[_capi.dptr(a) for a in six + three + [acf]], ip(tr)), model)
    return Mcse(*[a[:k] for a in six + three + [acf, tr]], tuple(range(k)) if sel is None else tuple(sel.tolist()), tuple(pr.tolist()))


def mcse_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
                cols: Optional[Sequence[int]] = None, probs: Sequence[float] = (0.05, 0.5, 0.95), nlags: int = 0) -> Mcse:
    """Monte Carlo standard errors and ESS of the mean, the sd and the quantiles at `probs` (at most 16) over the window
    [first, first + count) (count >= 4, each chain split in two halves as for rank_diagnostics_device) of a device buffer
    [chains][iterations][nvars], computed where the draws are (rh_mcse_device).  cols: the parameters asked for, in the result's
    order (None: all); nlags (0 .. 255): the lags of the autocorrelation function returned with them."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_mcse_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count, *a)
    return _mcse_result(call, nvars, cols, probs, nlags)


class Loo(NamedTuple):
    """Pointwise WAIC and PSIS-LOO (Vehtari, Gelman, Gabry 2017) per selected observation: lpd, p_waic, elpd_waic = lpd - p_waic,
    elpd_loo, p_loo = lpd - elpd_loo, the Pareto shape pareto_k of the importance ratios' tail (above 0.7: that elpd_loo is not to be
    trusted; +inf: a tail too short to fit) and its length tail_n.  A column with a NaN or an infinity is NaN."""
    lpd: np.ndarray
    p_waic: np.ndarray
    elpd_waic: np.ndarray
    elpd_loo: np.ndarray
    p_loo: np.ndarray
    pareto_k: np.ndarray
    tail_n: np.ndarray
    cols: Tuple[int, ...]

    @staticmethod
    def _total(pointwise):
        n = len(pointwise)
        return float(np.sum(pointwise)), float(np.sqrt(n * np.var(pointwise, ddof=1))) if n > 1 else float("nan")

    def loo(self) -> Tuple[float, float]:
        """(sum of elpd_loo, its standard error sqrt(n var(pointwise, ddof=1)))"""
        return self._total(self.elpd_loo)

    def waic(self) -> Tuple[float, float]:
        """(sum of elpd_waic, its standard error)"""
        return self._total(self.elpd_waic)

    def p_loo_total(self) -> Tuple[float, float]:
        """(the effective number of parameters sum of p_loo, its standard error)"""
        return self._total(self.p_loo)

    def p_waic_total(self) -> Tuple[float, float]:
        """(sum of p_waic, its standard error)"""
        return self._total(self.p_waic)


def _loo_result(call, nvars, cols, model=None):
    """shared by Sampler.loo and loo_device: call(cols, ncols, lpd, p_waic, elpd_loo, pareto_k, tail_n) -> rc"""
    sel = None if cols is None else np.ascontiguousarray([int(c) for c in cols], dtype=np.int32)
    k = int(nvars) if sel is None else len(sel)
    lpd, pw, el, pk = (np.zeros(max(k, 1)) for _ in range(4))
    tn = np.zeros(max(k, 1), dtype=np.int32)
    buf = sel if sel is None or k else np.zeros(1, dtype=np.int32)       # an empty list is a list (refused), not "all columns"
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _capi.check(call(ip(buf) if sel is not None else None, k if sel is not None else 0, _capi.dptr(lpd), _capi.dptr(pw), _capi.dptr(el),
                     _capi.dptr(pk), ip(tn)), model)
    lpd, pw, el, pk, tn = lpd[:k], pw[:k], el[:k], pk[:k], tn[:k]
    return Loo(lpd, pw, lpd - pw, el, lpd - el, pk, tn, tuple(range(k)) if sel is None else tuple(sel.tolist()))


def loo_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
               thin: int = 1, cols: Optional[Sequence[int]] = None) -> Loo:
    """Pointwise WAIC and PSIS-LOO over the kept iterations first + j * thin of a device buffer [chains][iterations][nvars] of
    log-likelihoods, column i holding log p(y_i | theta_s) (a predictor's to_host = False result), computed where they are
    (rh_loo_device): only five figures per observation return.  cols: the observations asked for, in the result's order (None: all)."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_loo_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count, int(thin), *a)
    return _loo_result(call, nvars, cols)


def loo_compare(a: Loo, b: Loo) -> Tuple[float, float]:
    """(elpd_diff, se_diff) of model a against model b over the same observations: the sum of the pointwise differences of elpd_loo
    (positive: a predicts better) and sqrt(n var(differences, ddof=1))."""
    d = np.asarray(a.elpd_loo) - np.asarray(b.elpd_loo)
    return float(np.sum(d)), float(np.sqrt(len(d) * np.var(d, ddof=1)))


class LooExpect(NamedTuple):
    """PSIS leave-one-out expectations per selected pair (log-likelihood column ll_cols[k], value column val_cols[k]): the mean and
    variance of the leave-one-out predictive distribution of the value (the `loo` package's E_loo), the LOO probability integral
    transform pit = P(value <= y | y_-i) and pit_lt (the same with <: a discrete y_rep is randomised between the two) -- None
    without y --, the PSIS effective sample size ess, and the Pareto shape pareto_k and tail length tail_n that Loo reports for the
    column (above 0.7: not to be trusted).  A NaN or an infinity among the log-likelihoods makes every figure of the pair NaN; one
    among the values makes mean, var, pit and pit_lt NaN."""
    mean: np.ndarray
    var: np.ndarray
    pit: Optional[np.ndarray]
    pit_lt: Optional[np.ndarray]
    ess: np.ndarray
    pareto_k: np.ndarray
    tail_n: np.ndarray
    ll_cols: Tuple[int, ...]
    val_cols: Tuple[int, ...]


def _loo_expect_result(call, nll, nval, ll_cols, val_cols, y, model=None):
    """shared by Sampler.loo_expect and loo_expect_device: call(ll_cols, val_cols, ncols, y, mean, var, pit, pit_lt, ess, pareto_k,
    tail_n) -> rc; without lists column i is paired with column i up to the narrower width"""
    both = range(max(0, min(int(nll), int(nval))))
    lc = np.ascontiguousarray([int(c) for c in (both if ll_cols is None else ll_cols)], dtype=np.int32)
    vc = np.ascontiguousarray([int(c) for c in (both if val_cols is None else val_cols)], dtype=np.int32)
    if len(lc) != len(vc):
        raise ValueError("loo_expect: ll_cols and val_cols pair up: %d against %d entries" % (len(lc), len(vc)))
    k = len(lc)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yy is not None and len(yy) != k:
        raise ValueError("loo_expect: y has %d entries for %d pairs" % (len(yy), k))
    mean, var, pit, plt, ess, pk = (np.zeros(max(k, 1)) for _ in range(6))
    tn = np.zeros(max(k, 1), dtype=np.int32)
    ip = lambda a: (a if len(a) else np.zeros(1, dtype=np.int32)).ctypes.data_as(C.POINTER(C.c_int32))   # an empty list is a list (refused)
    yp = None if yy is None else _capi.dptr(yy if k else np.zeros(1))
    _capi.check(call(ip(lc), ip(vc), k, yp, _capi.dptr(mean), _capi.dptr(var), _capi.dptr(pit) if yy is not None else None,
                     _capi.dptr(plt) if yy is not None else None, _capi.dptr(ess), _capi.dptr(pk), tn.ctypes.data_as(C.POINTER(C.c_int32))), model)
    return LooExpect(mean[:k], var[:k], pit[:k] if yy is not None else None, plt[:k] if yy is not None else None, ess[:k], pk[:k], tn[:k],
                     tuple(lc.tolist()), tuple(vc.tolist()))


def loo_expect_device(ll_ptr: int, val_ptr: int, chains: int, iterations: int, nll: int, nval: int, ll_cols: Sequence[int],
                      val_cols: Sequence[int], y: Optional[Sequence[float]] = None, device: int = 0, first: int = 0,
                      count: Optional[int] = None, thin: int = 1) -> LooExpect:
    """Is the model calibrated: PSIS leave-one-out expectations over the kept iterations first + j * thin of two buffers on one
    device, log-likelihoods [chains][iterations][nll] and values [chains][iterations][nval] (predictions or replicated observations;
    the two may be one buffer), computed where they are (rh_loo_expect_device).  Result k pairs log-likelihood column ll_cols[k]
    with value column val_cols[k]; y [len(ll_cols)]: the observations, for the LOO-PIT."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_loo_expect_device(C.c_void_p(ll_ptr), int(nll), C.c_void_p(val_ptr), int(nval), int(device), int(chains),
                                                       int(iterations), int(first), count, int(thin), *a)
    return _loo_expect_result(call, nll, nval, ll_cols, val_cols, y)


class LooQuantile(NamedTuple):
    """Leave-one-out predictive quantiles and scores per selected pair (log-likelihood column ll_cols[k], value column val_cols[k]):
    quantiles [K][len(probs)] of the PSIS-weighted predictive distribution of the value (the `loo` package's E_loo(type =
    "quantile")), its continuous ranked probability score crps against y (>= 0, smaller is better; None without y), its spread
    E|X - X'|, and the Pareto shape pareto_k and tail length tail_n that Loo reports for the column.  Without a log-likelihood
    predictor (plain mode) every draw weighs the same, ll_cols is empty and pareto_k and tail_n are None.  A NaN or an infinity among
    the log-likelihoods makes every figure of the pair NaN; one among the values makes its quantiles, crps and spread NaN."""
    probs: Tuple[float, ...]
    quantiles: np.ndarray
    crps: Optional[np.ndarray]
    spread: np.ndarray
    pareto_k: Optional[np.ndarray]
    tail_n: Optional[np.ndarray]
    ll_cols: Tuple[int, ...]
    val_cols: Tuple[int, ...]

    @property
    def abs_err(self) -> Optional[np.ndarray]:
        """E|X - y| = crps + spread / 2"""
        return None if self.crps is None else self.crps + 0.5 * self.spread

    @property
    def scrps(self) -> Optional[np.ndarray]:
        """the scaled CRPS, -E|X - y| / E|X - X'| - log(E|X - X'|) / 2 (larger is better)"""
        if self.crps is None:
            return None
        with np.errstate(all="ignore"):
            return -self.abs_err / self.spread - 0.5 * np.log(self.spread)


def _loo_quantile_result(call, plain, nll, nval, ll_cols, val_cols, y, probs, model=None):
    """shared by Sampler.loo_quantile and loo_quantile_device: call(ll_cols, val_cols, ncols, y, probs, nprobs, quantiles, crps, spread,
    pareto_k, tail_n) -> rc; without lists column i is paired with column i up to the narrower width (plain mode: every value column)"""
    both = range(max(0, int(nval) if plain else min(int(nll), int(nval))))
    vc = np.ascontiguousarray([int(c) for c in (both if val_cols is None else val_cols)], dtype=np.int32)
    lc = vc[:0] if plain else np.ascontiguousarray([int(c) for c in (both if ll_cols is None else ll_cols)], dtype=np.int32)
    if not plain and len(lc) != len(vc):
        raise ValueError("loo_quantile: ll_cols and val_cols pair up: %d against %d entries" % (len(lc), len(vc)))
    if plain and ll_cols is not None and len(ll_cols):
        raise ValueError("loo_quantile: ll_cols without log-likelihoods")
    k = len(vc)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yy is not None and len(yy) != k:
        raise ValueError("loo_quantile: y has %d entries for %d pairs" % (len(yy), k))
    pp = np.ascontiguousarray([float(p) for p in probs], dtype=np.float64)
    q = np.zeros((max(k, 1), max(len(pp), 1)))
    crps, spread, pk = (np.zeros(max(k, 1)) for _ in range(3))
    tn = np.zeros(max(k, 1), dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    ip = lambda a: (a if len(a) else np.zeros(1, dtype=np.int32)).ctypes.data_as(i32p)   # an empty list is a list (refused)
    yp = None if yy is None else _capi.dptr(yy if k else np.zeros(1))
    _capi.check(call(None if plain else ip(lc), ip(vc), k, yp, _capi.dptr(pp if len(pp) else np.zeros(1)), len(pp), _capi.dptr(q),
                     _capi.dptr(crps) if yy is not None else None, _capi.dptr(spread), None if plain else _capi.dptr(pk),
                     None if plain else tn.ctypes.data_as(i32p)), model)
    return LooQuantile(tuple(pp.tolist()), q[:k, :len(pp)], crps[:k] if yy is not None else None, spread[:k], None if plain else pk[:k],
                       None if plain else tn[:k], tuple(lc.tolist()), tuple(vc.tolist()))


def loo_quantile_device(ll_ptr: Optional[int], val_ptr: int, chains: int, iterations: int, nll: int, nval: int, ll_cols: Optional[Sequence[int]],
                        val_cols: Sequence[int], probs: Sequence[float] = (0.05, 0.5, 0.95), y: Optional[Sequence[float]] = None, device: int = 0,
                        first: int = 0, count: Optional[int] = None, thin: int = 1) -> LooQuantile:
    """Leave-one-out predictive quantiles, CRPS and spread over the kept iterations first + j * thin of two buffers on one device,
    log-likelihoods [chains][iterations][nll] and values [chains][iterations][nval] (predictions or replicated observations),
    computed where they are (rh_loo_quantile_device).  Result k pairs log-likelihood column ll_cols[k] with value column val_cols[k];
    y [len(val_cols)]: the observations, for the CRPS.  ll_ptr = None: plain mode, every draw weighs the same."""
    count = int(iterations) - int(first) if count is None else int(count)
    plain = ll_ptr is None
    call = lambda *a: _capi.lib().rh_loo_quantile_device(None if plain else C.c_void_p(ll_ptr), int(nll), C.c_void_p(val_ptr), int(nval), int(device),
                                                         int(chains), int(iterations), int(first), count, int(thin), *a)
    return _loo_quantile_result(call, plain, nll, nval, ll_cols, val_cols, y, probs)


class ppc:
    """Statistic constructors of a Check's table (rh_ppc_stat): what a posterior predictive check evaluates on every segment of every
    replicated data set."""

    @staticmethod
    def _stat(kind, arg=0.0) -> "_capi.PpcStat": return _capi.PpcStat(kind, 0, float(arg))
    @staticmethod
    def mean(): return ppc._stat(_capi.PPC_MEAN)
    @staticmethod
    def sd(): return ppc._stat(_capi.PPC_SD)                  # divisor n - 1
    @staticmethod
    def min(): return ppc._stat(_capi.PPC_MIN)
    @staticmethod
    def max(): return ppc._stat(_capi.PPC_MAX)
    @staticmethod
    def quantile(p): return ppc._stat(_capi.PPC_QUANTILE, p)  # the order statistic sorted[min(n - 1, floor(n p))]: precis' rule
    @staticmethod
    def frac_le(c): return ppc._stat(_capi.PPC_FRAC_LE, c)    # #{v <= c} / n: frac_le(0) is the share of zeros of count data


class Check:
    """rh_ppc: a table of ppc.* statistics over segments of the `nin` columns of a replicated data set (Sampler.ppc, ppc_device).
    cols: the columns selected, duplicates allowed (None: all in order); segments: a list of column lists, each a group of
    observations the statistics are evaluated on (None: one segment, `cols` or everything); give one or the other.  nout = number
    of segments x number of statistics."""

    def __init__(self, stats, nin: int, cols: Optional[Sequence[int]] = None, segments: Optional[Sequence[Sequence[int]]] = None, device: int = -1):
        self._h = C.c_void_p()
        stats = list(stats)
        if segments is not None:
            if cols is not None:
                raise ValueError("Check: give cols or segments, not both")
            segments = [[int(c) for c in seg] for seg in segments]
            cols = [c for seg in segments for c in seg]
            off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(seg) for seg in segments])]), dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        cc = None if cols is None else np.ascontiguousarray([int(c) for c in cols] or [0], dtype=np.int32)
        arr = (_capi.PpcStat * max(1, len(stats)))(*stats)
        _capi.check(_capi.lib().rh_ppc_create(arr, len(stats), None if cc is None else ip(cc), 0 if cols is None else len(cols),
                                              None if segments is None else ip(off), 0 if segments is None else len(segments), int(nin), int(device),
                                              C.byref(self._h)))
        self.nin, self.nstat = int(nin), len(stats)
        self.nout = _capi.lib().rh_ppc_nout(self._h)
        self.nseg = self.nout // self.nstat

    def close(self):
        if self._h:
            _capi.lib().rh_ppc_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class Ppc(NamedTuple):
    """A posterior predictive check: per (segment, statistic) the statistic of the observations t_obs and, over the S draws, how many
    replicated statistics are above it (n_gt), equal to it (n_eq) and NaN (n_bad) -- all None without y; t_rep [chains][kept][nout]
    (output g * nstat + k) on the host or None; dev_ptr: the check's own device buffer of that shape, valid until its next call."""
    t_obs: Optional[np.ndarray]
    n_gt: Optional[np.ndarray]
    n_eq: Optional[np.ndarray]
    n_bad: Optional[np.ndarray]
    t_rep: Optional[np.ndarray]
    dev_ptr: int
    S: int

    def _p(self, weight_eq):
        if self.t_obs is None:
            return np.array(np.nan)
        with np.errstate(all="ignore"):
            den = (self.S - self.n_bad).astype(np.float64)
            return np.where(den > 0, (self.n_gt + weight_eq * self.n_eq) / den, np.nan)

    @property
    def p_ge(self) -> np.ndarray:
        """the Bayesian p-value P(T(y_rep) >= T(y)) over the draws whose statistic is a number; NaN where there is none or no y"""
        return self._p(1.0)

    @property
    def p_gt(self) -> np.ndarray:
        return self._p(0.0)

    @property
    def p_mid(self) -> np.ndarray:
        """(n_gt + n_eq / 2) / (S - n_bad): the mid p-value, for statistics with ties (counts, shares)"""
        return self._p(0.5)


def _ppc_result(call, check, chains, kept, y, to_host, model=None):
    """shared by Sampler.ppc and ppc_device: call(y, t_obs, n_gt, n_eq, n_bad, host_out, byref(dev_out)) -> rc"""
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yy is not None and len(yy) != check.nin:
        raise ValueError("ppc: y has %d entries, the check reads %d columns" % (len(yy), check.nin))
    t_obs = np.zeros(check.nout)
    n_gt, n_eq, n_bad = (np.zeros(check.nout, dtype=np.int64) for _ in range(3))
    out = np.zeros((chains, kept, check.nout)) if to_host else None
    ptr = C.c_void_p()
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    _capi.check(call(None if yy is None else _capi.dptr(yy), _capi.dptr(t_obs), lp(n_gt), lp(n_eq), lp(n_bad), _capi.dptr(out) if to_host else None,
                     C.byref(ptr)), model)
    shape = (check.nseg, check.nstat)
    if yy is None:
        return Ppc(None, None, None, None, out, ptr.value, chains * kept)
    return Ppc(t_obs.reshape(shape), n_gt.reshape(shape), n_eq.reshape(shape), n_bad.reshape(shape), out, ptr.value, chains * kept)


def ppc_device(check: Check, ptr: int, chains: int, iterations: int, nin: int, y: Optional[Sequence[float]] = None, first: int = 0,
               count: Optional[int] = None, thin: int = 1, device: int = 0, to_host: bool = True) -> Ppc:
    """Does the model reproduce the data: the check's statistics of every replicated data set of a device buffer
    [chains][iterations][nin] (a generator's to_host = False result) over the kept iterations first + j * thin, computed where they
    are (rh_ppc_device), and with y [nin] -- the observations -- the same statistics of y and the counts of a Bayesian p-value."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_ppc_device(check._h, C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nin), int(first), count,
                                                int(thin), *a)
    return _ppc_result(call, check, int(chains), _kept(count, thin), y, to_host)


def histogram_device(ptr: int, chains: int, iterations: int, nvars: int, device: int = 0, first: int = 0, count: Optional[int] = None,
                     thin: int = 1, cols: Optional[Sequence[int]] = None, bins: int = 20, range=None) -> Histogram:
    """Histograms of the pooled kept iterations first + j * thin of a device buffer [chains][iterations][nvars] (a sampler's draws, a
    predictor's to_host = False result, Comm.allgather_draws(to_host=False)), binned where the draws are (rh_histogram_device).
    cols: the parameters asked for, in the result's order (None: all).  range: None (every column between its smallest and largest
    finite value, found on the device), one (lo, hi) for all columns, or one per column (None or (nan, nan): automatic).  The
    default of 20 bins is this package's: the reference's comes from a plotting library that is not in its tree."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_histogram_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count,
                                                      int(thin), *a)
    return _histogram_result(call, nvars, cols, bins, range)


def histogram2d_device(ptr: int, chains: int, iterations: int, nvars: int, pairs: Sequence[Tuple[int, int]], device: int = 0, first: int = 0,
                       count: Optional[int] = None, thin: int = 1, bins=(32, 32), range=None) -> Histogram2d:
    """Joint count grids of pairs of parameters over the pooled kept iterations of a device buffer [chains][iterations][nvars]
    (rh_histogram2d_device).  bins: (nbx, nby) or one number, nbx * nby <= 4096.  range: None (automatic per axis), one
    ((xlo, xhi), (ylo, yhi)) for all pairs, or one per pair."""
    count = int(iterations) - int(first) if count is None else int(count)
    call = lambda *a: _capi.lib().rh_histogram2d_device(C.c_void_p(ptr), int(device), int(chains), int(iterations), int(nvars), int(first), count,
                                                        int(thin), *a)
    return _histogram2d_result(call, pairs, bins, range)


def format_precis(names: Sequence[str], summary: Summary) -> str:
    """precis' table (rainier-notebook package.scala:393-417, without the correlations) as a string: Mean, StdDev and the first two
    order statistics of `summary`, %10.2f, one line per parameter."""
    names = [str(k) for k in names]
    if len(names) != len(summary.mean) or summary.quantiles.shape[1] < 2:
        raise ValueError("format_precis: one name per parameter and at least two probabilities")
    width = max(len(k) for k in names)
    heads = ["Mean", "StdDev"] + ["%g%%" % (100.0 * q) for q in summary.probs[:2]]
    lines = ["".ljust(width) + "".join("%10s" % h for h in heads)]
    for k, m, s, q in zip(names, summary.mean, summary.sd, summary.quantiles):
        lines.append(k.ljust(width) + "".join("%10.2f" % v for v in (m, s, q[0], q[1])))
    return "\n".join(lines)


class Sampler:
    """Device-resident chains: split form of Driver.sample used by bench.py (create -> warmup -> run)."""

    def __init__(self, model: "Model", config: SamplerConfig, seeds: Sequence[int] = None, rng_states=None):
        """seeds: chain c runs on ScalaRNG(seeds[c]).  rng_states: instead, continue existing java.util.Random streams --
        one (internal 48-bit state, pending nextNextGaussian or None) per chain (what Driver.sample does with the caller's rng)."""
        self.model = model
        self._nn = None
        if rng_states is not None:
            seeds = [int(st) ^ 0x5DEECE66D for st, _ in rng_states]
            self._nn = np.array([np.nan if g is None else float(g) for _, g in rng_states], dtype=np.float64)
        self.chains = len(seeds)
        self.iterations = int(config.iterations)
        self._cfg, self._keep = to_c_config(config, model.nVars)
        if self._nn is not None:
            self._cfg.rng_next_gaussian = _capi.dptr(self._nn)
        self._seeds = (C.c_int64 * self.chains)(*[int(s) for s in seeds])
        self._h = C.c_void_p()
        _capi.check(_capi.lib().rh_sampler_create(model._h, C.byref(self._cfg), self._seeds, self.chains, C.byref(self._h)), model._h)

    def warmup(self): _capi.check(_capi.lib().rh_sampler_warmup(self._h), self.model._h)
    def run(self, n: int): _capi.check(_capi.lib().rh_sampler_run(self._h, int(n)), self.model._h)

    def draws(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.iterations - first if count is None else count
        out = np.zeros((self.chains, count, self.model.nVars))
        _capi.check(_capi.lib().rh_sampler_draws(self._h, first, count, _capi.dptr(out)), self.model._h)
        return out

    def draws_device_ptr(self) -> int:
        p = C.c_void_p()
        _capi.check(_capi.lib().rh_sampler_draws_device(self._h, C.byref(p)), self.model._h)
        return p.value

    def stats(self):
        st = (_capi.ChainStats * self.chains)()
        mass = np.zeros((self.chains, self.model.nVars))
        _capi.check(_capi.lib().rh_sampler_stats(self._h, st, _capi.dptr(mass)), self.model._h)
        return [Stats(s.leapfrog_steps, s.warmup_leapfrog_steps, s.gradient_evaluations, s.accepted,
                      s.mean_accept_prob, s.step_size, s.bfmi) for s in st], mass

    def progress(self):
        """(warmed, sampling iterations done): what a Progress callback would be told (sampler/Driver.scala:7-11), polled."""
        w, it = C.c_int32(0), C.c_int32(0)
        _capi.check(_capi.lib().rh_sampler_progress(self._h, C.byref(w), C.byref(it)), self.model._h)
        return bool(w.value), int(it.value)

    def diagnostics(self, first: int = 0, count: Optional[int] = None, moments: bool = False):
        """Trace.diagnostics of the draws where they are (rh_sampler_diagnostics): the list of (rHat, effectiveSampleSize) per
        parameter over iterations [first, first + count), count = None: everything completed so far; with moments = True
        (diag, mean [nVars], var [nVars]) -- the pooled mean and Trace's v."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        n = self.model.nVars
        rhat, ess, mean, var = (np.zeros(n) for _ in range(4))
        _capi.check(_capi.lib().rh_sampler_diagnostics(self._h, int(first), count, _capi.dptr(rhat), _capi.dptr(ess), _capi.dptr(mean),
                                                       _capi.dptr(var)), self.model._h)
        return _diag_result(rhat, ess, mean, var, moments)

    def predict(self, predictor: Predictor, first: int = 0, count: Optional[int] = None, thin: int = 1, to_host: bool = True,
                diagnostics: bool = False):
        """Trace.predict over the draws where they are (rh_sampler_predict), with Trace.thin applied to the window: the kept
        iterations are first + j * thin; count = None: everything completed so far.  Returns [chains][kept][nreq] (to_host = False:
        the device pointer of the predictor's buffer); with diagnostics = True (values, diag, mean, var) of the predictions."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda host, dev: _capi.lib().rh_sampler_predict(self._h, predictor._h, int(first), count, int(thin), host, dev)
        # (device -1: the current one, which rh_sampler_predict has just made the sampler's)
        return _predict_result(call, predictor, self.chains, count, thin, -1, to_host, diagnostics, self.model._h)

    def generate(self, predictor: Predictor, generator: Generator, seed: int, first: int = 0, count: Optional[int] = None, thin: int = 1,
                 chain0: int = 0, to_host: bool = True):
        """trace.predict(distribution) over the draws where they are (rh_sampler_generate): the predictor's requirements of the kept
        iterations first + j * thin are the generator's parameter columns.  Returns the samples [chains][kept][nout] (to_host =
        False: the device pointer of the generator's buffer, which summary_device / diagnostics_device take)."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda host, dev, fl: _capi.lib().rh_sampler_generate(self._h, predictor._h, generator._h, int(first), count, int(thin),
                                                                     int(seed), int(chain0), host, dev, fl)
        return _generate_result(call, generator, self.chains, _kept(count, thin), to_host, self.model._h)

    def summary(self, first: int = 0, count: Optional[int] = None, thin: int = 1, probs: Sequence[float] = (0.055, 0.945),
                hdpi: Optional[float] = 0.89) -> Summary:
        """precis' figures and hdpi of the draws where they are (rh_sampler_summary): mean, sd, the order statistics at `probs` and
        the highest-density interval of every parameter over the kept iterations first + j * thin of all chains pooled;
        count = None: everything completed so far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_summary(self._h, int(first), count, int(thin), *a)
        return _summary_result(call, self.model.nVars, probs, hdpi, self.model._h)

    def covariance(self, first: int = 0, count: Optional[int] = None, thin: int = 1, cols: Optional[Sequence[int]] = None,
                   corr: bool = False) -> Covariance:
        """The pooled sample covariance (and, with corr = True, the correlation) of the parameters over the kept iterations
        first + j * thin of all chains, computed where the draws are (rh_sampler_covariance); cols: the parameters asked for, in the
        result's order (None: all); count = None: everything completed so far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_covariance(self._h, int(first), count, int(thin), *a)
        return _covariance_result(call, self.model.nVars, cols, corr, self.model._h)

    def histogram(self, first: int = 0, count: Optional[int] = None, thin: int = 1, cols: Optional[Sequence[int]] = None, bins: int = 20,
                  range=None) -> Histogram:
        """Histograms of the parameters over the kept iterations first + j * thin of all chains pooled, binned where the draws are
        (rh_sampler_histogram): the reference's density(seq, bounds).  cols: the parameters asked for, in the result's order (None:
        all); range: None (every column between its smallest and largest finite value), one (lo, hi) for all columns, or one per
        column (None or (nan, nan): automatic); count = None: everything completed so far.  The default of 20 bins is this
        package's: the reference's comes from a plotting library that is not in its tree.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_histogram(self._h, int(first), count, int(thin), *a)
        return _histogram_result(call, self.model.nVars, cols, bins, range, self.model._h)

    def histogram2d(self, pairs: Sequence[Tuple[int, int]], first: int = 0, count: Optional[int] = None, thin: int = 1, bins=(32, 32),
                    range=None) -> Histogram2d:
        """Joint count grids of pairs of parameters over the same window (rh_sampler_histogram2d): what the reference's scatter /
        contour show.  bins: (nbx, nby) or one number, nbx * nby <= 4096; range: None (automatic per axis), one
        ((xlo, xhi), (ylo, yhi)) for all pairs, or one per pair.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_histogram2d(self._h, int(first), count, int(thin), *a)
        return _histogram2d_result(call, pairs, bins, range, self.model._h)

    def rank_diagnostics(self, first: int = 0, count: Optional[int] = None, cols: Optional[Sequence[int]] = None) -> RankDiagnostics:
        """Can this run be trusted: rank-normalised split R-hat, bulk ESS and tail ESS (Vehtari et al. 2021) of the parameters over
        the window [first, first + count) of every chain, computed where the draws are (rh_sampler_rank_diagnostics).  It sees what
        diagnostics() (the reference's unsplit R-hat on the raw values) cannot: a trend all chains share, a chain of another scale, a
        posterior without a variance.  cols: the parameters asked for, in the result's order (None: all); count = None: everything
        completed so far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_rank_diagnostics(self._h, int(first), count, *a)
        return _rank_result(call, self.model.nVars, cols, self.model._h)

    def mcse(self, first: int = 0, count: Optional[int] = None, cols: Optional[Sequence[int]] = None, probs: Sequence[float] = (0.05, 0.5, 0.95),
             nlags: int = 0) -> Mcse:
        """How many digits of summary()'s figures survive the Monte Carlo error: the standard errors and effective sample sizes of the
        mean, the sd and the quantiles at `probs` (Vehtari et al. 2021, section 4) of the parameters over the window
        [first, first + count) of every chain, with the autocorrelations up to lag `nlags`, computed where the draws are
        (rh_sampler_mcse).  cols: the parameters asked for, in the result's order (None: all); count = None: everything completed so
        far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_mcse(self._h, int(first), count, *a)
        return _mcse_result(call, self.model.nVars, cols, probs, nlags, self.model._h)

    def loo(self, predictor: Predictor, first: int = 0, count: Optional[int] = None, thin: int = 1, cols: Optional[Sequence[int]] = None) -> Loo:
        """Which model predicts better: pointwise WAIC and PSIS-LOO (Vehtari, Gelman, Gabry 2017) of the predictor's requirements --
        the log-likelihood of every observation -- over the kept iterations first + j * thin of every chain.  The chains x kept x
        observations matrix is made and reduced on the device (rh_sampler_loo) and never leaves it.  cols: the observations asked
        for, in the result's order (None: all); count = None: everything completed so far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_loo(self._h, predictor._h, int(first), count, int(thin), *a)
        return _loo_result(call, predictor.nreq, cols, self.model._h)

    def loo_expect(self, ll_predictor: Predictor, predictor: Predictor, ll_cols: Optional[Sequence[int]] = None,
                   val_cols: Optional[Sequence[int]] = None, y: Optional[Sequence[float]] = None, generator: Optional[Generator] = None,
                   seed: int = 0, first: int = 0, count: Optional[int] = None, thin: int = 1) -> LooExpect:
        """Is the model calibrated: the leave-one-out predictive mean and variance of every observation, its LOO-PIT against y and
        the PSIS effective sample size (the `loo` package's E_loo and loo_pit) over the kept iterations first + j * thin of every
        chain.  ll_predictor's requirements are the pointwise log-likelihoods; the values are `predictor`'s requirements or, with a
        generator, the samples it draws from them (with `seed`, the bits of Sampler.generate(predictor, generator, seed)).  Both
        matrices are made and reduced on the device (rh_sampler_loo_expect) and never leave it.  Result k pairs log-likelihood column
        ll_cols[k] with value column val_cols[k]; None: column i with column i up to the narrower width.  count = None: everything
        completed so far.  The chains are not altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_loo_expect(self._h, ll_predictor._h, predictor._h, generator._h if generator is not None else None,
                                                            int(seed), int(first), count, int(thin), *a)
        return _loo_expect_result(call, ll_predictor.nreq, generator.nout if generator is not None else predictor.nreq, ll_cols, val_cols, y,
                                  self.model._h)

    def loo_quantile(self, ll_predictor: Optional[Predictor], predictor: Predictor, probs: Sequence[float] = (0.05, 0.5, 0.95),
                     ll_cols: Optional[Sequence[int]] = None, val_cols: Optional[Sequence[int]] = None, first: int = 0, count: Optional[int] = None,
                     thin: int = 1, y: Optional[Sequence[float]] = None, generator: Optional[Generator] = None, seed: Optional[int] = None) -> LooQuantile:
        """What the leave-one-out predictive distribution of every observation looks like: its quantiles at `probs` (the `loo`
        package's E_loo(type = "quantile"): the 90 % interval by default), its CRPS against y and its spread E|X - X'|, over the kept
        iterations first + j * thin of every chain.  ll_predictor's requirements are the pointwise log-likelihoods (None: plain mode,
        the posterior predictive distribution itself); the values are `predictor`'s requirements or, with a generator, the samples it
        draws from them (with `seed`, the bits of Sampler.generate(predictor, generator, seed); None: 0).  Both matrices are made,
        sorted and scanned on the device (rh_sampler_loo_quantile) and never leave it.  Result k pairs log-likelihood column
        ll_cols[k] with value column val_cols[k]; None: column i with column i up to the narrower width.  The chains are not
        altered."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        plain = ll_predictor is None
        call = lambda *a: _capi.lib().rh_sampler_loo_quantile(self._h, None if plain else ll_predictor._h, predictor._h,
                                                              generator._h if generator is not None else None, int(seed or 0), int(first), count, int(thin), *a)
        return _loo_quantile_result(call, plain, 0 if plain else ll_predictor.nreq, generator.nout if generator is not None else predictor.nreq, ll_cols,
                                    val_cols, y, probs, self.model._h)

    def ppc(self, predictor: Predictor, generator: Generator, check: Check, seed: int, y: Optional[Sequence[float]] = None, first: int = 0,
            count: Optional[int] = None, thin: int = 1, to_host: bool = True) -> Ppc:
        """Does the fitted model reproduce the features of the data: a posterior predictive check over the kept iterations
        first + j * thin of every chain.  The replicated observations are Sampler.generate(predictor, generator, seed)'s, bit for bit;
        they are made and reduced on the device (rh_sampler_ppc) and never leave it.  y [generator.nout]: the observations, for
        t_obs and the p-values' counts; count = None: everything completed so far.  The chains are not altered.  The generator's
        flags are not reported here (generator.flags keeps its last generate call's): a sample outside its domain or from a capped
        loop is NaN, makes its segment's statistics NaN and is counted in n_bad."""
        count = self.progress()[1] - int(first) if count is None else int(count)
        call = lambda *a: _capi.lib().rh_sampler_ppc(self._h, predictor._h, generator._h, check._h, int(seed), 0, int(first), count, int(thin), *a)
        return _ppc_result(call, check, self.chains, _kept(count, thin), y, to_host, self.model._h)

    def mass_dense(self) -> np.ndarray:
        """DenseMassMatrix.elements of every chain: [chains][nVars][nVars] (DenseMassMatrixTuner only)."""
        n = self.model.nVars
        out = np.zeros((self.chains, n, n))
        _capi.check(_capi.lib().rh_sampler_mass_dense(self._h, _capi.dptr(out)), self.model._h)
        return out

    def lane_feed(self):
        """which feed the gradient launches take: None (not the lane walk), "cols" or "rows" (csrc/device/rh_lane.hip.h)"""
        f = _capi.lib().rh_sampler_lane_feed
        f.argtypes, f.restype = [C.c_void_p], C.c_int
        return {0: None, 1: "cols", 2: "rows"}[f(self._h)]

    def timing(self, reset: bool = False):
        t = _capi.Timing()
        _capi.check(_capi.lib().rh_sampler_timing(self._h, C.byref(t), int(reset)), self.model._h)
        return {"kernel_ms": t.kernel_ms, "total_ms": t.total_ms, "launches": t.launches, "density_evals": t.density_evals,
                "row_chain_evals": t.row_chain_evals, "dominant_kernel": t.dominant_kernel.decode(), "chain_slots": t.chain_slots,
                "steady_kernel_ms": t.steady_kernel_ms, "steady_launches": t.steady_launches, "steady_density_evals": t.steady_density_evals}

    def close(self):
        if self._h:
            _capi.lib().rh_sampler_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def sample_multi(models, config: SamplerConfig = None, seeds: Sequence[int] = None) -> "Trace":
    """Model.sample fanned out over several devices behind the C ABI (rh_sample_multi): models[g] is the same program
    compiled for device g; chains are cut into contiguous shards by GLOBAL chain id, so the trace does not depend on
    len(models)."""
    config = config or SamplerConfig()
    nv = models[0].nVars
    chains = len(seeds)
    cfg, _keep = to_c_config(config, nv)
    draws = np.zeros((chains, int(config.iterations), nv))
    mass = np.zeros((chains, nv))
    st = (_capi.ChainStats * chains)()
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    sd = (C.c_int64 * chains)(*[int(x) for x in seeds])
    # a shard's failure is reported through the calling thread's error slot (rh_last_error(NULL)), not through models[0]
    _capi.check(_capi.lib().rh_sample_multi(handles, len(models), C.byref(cfg), sd, chains, _capi.dptr(draws), _capi.dptr(mass), st))
    stats = [Stats(s.leapfrog_steps, s.warmup_leapfrog_steps, s.gradient_evaluations, s.accepted, s.mean_accept_prob, s.step_size, s.bfmi)
             for s in st]
    return Trace(draws, mass, stats)


class Model:
    """A compiled model: Compiler.compileTargets' replacement (compute/Compiler.scala:14-30) + Model.sample."""

    def __init__(self, spec, device: int = -1, math_mode: int = _capi.MATH_FAST, fp_contract: bool = False,
                 rows_unroll: int = 0, grad_chains: int = 0, grad_unroll: int = 0, factor_outputs: bool = False,
                 with_nuts: bool = False):
        L = _capi.lib()
        self.spec = spec
        self.nVars = spec.n_params
        self._cols = [np.ascontiguousarray(c, dtype=np.float64) for c in spec.columns]
        colarr = (C.POINTER(C.c_double) * max(1, len(self._cols)))(*[_capi.dptr(c) for c in self._cols])
        nrows = (C.c_int64 * len(spec.nrows))(*spec.nrows)
        opts = _capi.compile_opts(device, math_mode, fp_contract, rows_unroll, grad_chains, grad_unroll, factor_outputs,
                                   with_nuts)
        blob = C.create_string_buffer(spec.rir, len(spec.rir))
        self._h = C.c_void_p()
        _capi.check(L.rh_model_create(blob, len(spec.rir), colarr, nrows, C.byref(opts), C.byref(self._h)))

    def clone(self, device: int = -1) -> "Model":
        """the same compiled model on another device of this process (rh_model_clone): code object reused, columns copied
        device to device -- one per GPU for sample_multi"""
        other = object.__new__(Model)
        other.spec, other.nVars, other._cols = self.spec, self.nVars, self._cols
        other._h = C.c_void_p()
        _capi.check(_capi.lib().rh_model_clone(self._h, int(device), C.byref(other._h)))
        return other

    @property
    def hip_source(self) -> str: return _capi.lib().rh_model_hip_source(self._h).decode()

    def engines(self) -> dict:
        """rh_model_engines: which engines the engine agrees to run for this model on this toolchain and why not
        ({"chain": bool, "tick": bool, "density": bool, "compile_attempts": int, "why": str})."""
        c, t, d, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        why = C.create_string_buffer(2048)
        _capi.check(_capi.lib().rh_model_engines(self._h, C.byref(c), C.byref(t), C.byref(d), C.byref(a), why, len(why)), self._h)
        return {"chain": bool(c.value), "tick": bool(t.value), "density": bool(d.value), "compile_attempts": a.value,
                "why": why.value.decode(errors="replace")}

    def density(self) -> DensityFunction: return DensityFunction(self)

    def density_batch(self, q: np.ndarray, engine: int = _capi.ENGINE_AUTO, grad_splits: int = 0):
        """Batched DensityFunction.update.  engine = ENGINE_TICK evaluates through the sampler's batched gradient kernels
        (rh_grad_kernel / rh_grad_glm_kernel / rh_grad_gather_kernel + the tick combine) instead of one chain per wavefront."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        chains = q.shape[0]
        lp, g = np.zeros(chains), np.zeros((chains, self.nVars))
        _capi.check(_capi.lib().rh_density_eval_ex(self._h, _capi.dptr(q), chains, int(engine), int(grad_splits),
                                                   _capi.dptr(lp), _capi.dptr(g)), self._h)
        return lp, g

    def sample(self, config: SamplerConfig = None, nChains: int = 4, seeds: Sequence[int] = None, rng_states=None) -> Trace:
        """Model.sample(config, nChains) (core/Model.scala:13-24).  Chain c is the reference run with
        nChains = 1 and ScalaRNG(seeds[c])."""
        config = config or SamplerConfig()
        seeds = list(range(1, nChains + 1)) if seeds is None else list(seeds)
        s = Sampler(self, config, seeds, rng_states)
        try:
            s.warmup(); s.run(config.iterations)
            draws = s.draws() if config.iterations > 0 else np.zeros((s.chains, 0, self.nVars))
            stats, mass = s.stats()
        finally:
            s.close()
        return Trace(draws, mass, stats)

    def optimize(self, starts: np.ndarray = None, max_evals: int = 0):
        """Model.optimize's numeric part = Optimizer.lbfgs(density()) (core/Model.scala:26-30, optimizer/Optimizer.scala:6-24).
        starts None: the reference's single start at 0 -> x [nVars]; starts [k][nVars]: k independent searches sharing
        each batched density launch -> (x [k][nVars], evals [k], status [k])"""
        single = starts is None
        x0 = np.zeros((1, self.nVars)) if single else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, self.nVars)
        k = x0.shape[0]
        x, evals, status = np.zeros((k, self.nVars)), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        _capi.check(_capi.lib().rh_optimize(self._h, _capi.dptr(x0), k, max_evals, _capi.dptr(x), ip(evals), ip(status)), self._h)
        if single:
            if status[0] == _capi.OPT_NOT_DESCENT:
                raise RuntimeError("dginit")       # LBFGS.java:236-237
            return x[0]
        return x, evals, status

    def selftest(self, mode: int, seed: int = 0, x: np.ndarray = None, n: int = None) -> np.ndarray:
        x = np.zeros(1) if x is None else np.ascontiguousarray(x, dtype=np.float64)
        n = (x.size // 2 if mode in (5, 14) else x.size) if n is None else n
        out = np.zeros(n)
        _capi.check(_capi.lib().rh_selftest(self._h, mode, seed, _capi.dptr(x), _capi.dptr(out), n), self._h)
        return out

    def close(self):
        if self._h:
            _capi.lib().rh_model_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
