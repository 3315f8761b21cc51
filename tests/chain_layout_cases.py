"""The cases that pin rh_chain_kernel at every chain-state layout boundary (csrc/device/rh_engine.hip.h, rh_prelude.hip.h), shared by
tests/test_gpu_chain_layouts.py (device against oracle, bit for bit) and tests/test_chain_layout_cases_cpu.py (the oracle alone:
every case here must be a chain that moves -- a stuck chain compares equal whatever the kernel does).

The layout is chosen from the parameter count of a data-free model: packed (RH_PACK_L 8 / 16 / 32, several chains per wavefront)
up to 32 parameters, one register slot up to 64, 2..8 register slots up to 512, big mode beyond (not here).  Every model is
models.funnel(d): an isotropic standard normal in d dimensions, strict math."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import rainier_amd as R
from rainier_amd import models
from tests import oracle_lib as O

SIZES = (1, 2, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 129, 511, 512)
DENSE_SIZES = (1, 2, 8, 9, 16, 17, 32, 33, 63, 64)
RING_SIZES = (1, 63, 64, 65, 128, 255, 256)
RNG_SIZES = (1, 2, 9, 10, 63, 64, 65)
RING_DIM = 10
# Sizes whose register layout this toolchain cannot run, with the reason the engine gives.  Held to the register layout
# (RH_NO_CHUNKS=1), rh_chain_kernel of a funnel of 127 parameters or more spills its vector registers, and the engine's
# code-object inspection takes it out of use.  Left to itself the engine lowers these sizes memory-resident instead (big mode,
# RH_BIGN 1: after the failed attempt, or at once for a generated function of more than 1000 statements), where sums are no longer
# strictly left to right and a bit-exact comparison with the oracle does not apply.  The GPU test expects exactly the refusal:
# where it comes (at 511 rh_density_kernel spills too, which leaves no kernel at all, so creating the model already fails; the
# others fail when a sampler asks for the chain engine) and the reason given there.
REGISTER_LAYOUT_REFUSED = {128: ("sample", "rh_chain_kernel: [0-9]+ spilled vector registers"),
                           129: ("sample", "rh_chain_kernel: [0-9]+ spilled vector registers"),
                           511: ("model", "rh_density_kernel: [0-9]+ spilled vector registers"),
                           512: ("sample", "rh_chain_kernel: [0-9]+ spilled vector registers")}
MANY = 4099            # >= 4096 chains: EHMC / NUTS stay packed (rh_sampler_create), and 4099 leaves the last wavefront ragged


def pack_of(d):
    """RH_PACK_L the emitter chooses for a data-free model of d parameters (csrc/emit.cpp)"""
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def slots_of(d):
    return (d + 63) // 64


def layout_of(source):
    """(RH_PACK_L, RH_SLOTS, RH_BIGN) of a generated translation unit: the emitter's own defines come first"""
    import re
    return tuple(int(re.search(r"#define %s (\d+)\n" % k, source).group(1)) for k in ("RH_PACK_L", "RH_SLOTS", "RH_BIGN"))


def kernel_variants():
    """(d, sampler-kernel variant, environment or None) of every code object tests/test_gpu_chain_layouts.py loads, for build()'s
    kernel cache.  Variant bits (csrc/engine.cpp rh_sampler_create): 1 NUTS, 2 dense mass matrix, 4 one chain per wavefront
    although the model packs (EHMC / NUTS with fewer than 4096 chains)."""
    out = []
    for d in sorted(set(SIZES + RNG_SIZES + (RING_DIM,))):
        out.append((d, 0, None))          # (a refused size: the engine's own, memory-resident lowering, which the test looks at last)
        if d in SIZES and d not in REGISTER_LAYOUT_REFUSED:
            out.append((d, 1, None))
        if d <= 32 and (d in SIZES or d == RING_DIM):
            out.append((d, 4, None))
        if d <= 32 and d in SIZES:
            out += [(d, 5, None), (d, 0, {"RH_PACK": "0"})]
    for d in DENSE_SIZES:
        out += [(d, 2, None), (d, 6, None), (d, 7, None)] if d <= 32 else [(d, 2, None), (d, 3, None)]
    return out


# group: sizes / dense / ring / rng; key: the parameter (d, or the ring size B); d: parameters of the funnel; config: the run;
# seeds: one per chain; compare: the chains that are held against the oracle; rng: None, or per chain (seed, gaussians already
# drawn from it) -- the chain continues that java.util.Random state (an odd count leaves a pending nextNextGaussian)
Case = namedtuple("Case", "group key label d config seeds compare rng")


# first seeds of the two cases whose default seeds gave chains that reject too often on the oracle (fewer than 80 % of the draws
# move: tests/test_chain_layout_cases_cpu.py); every other case derives its seeds from its size
_RESEED = {("sizes", 511, "ehmc3"): 56250, ("rng", 63, "mixed"): 1781}


def _seeds(group, key, label, first, n):
    first = _RESEED.get((group, key, label), first)
    return tuple(range(first, first + n))


def _ends(n):
    return tuple(sorted({0, 1, 2, 3, 5, n // 2, n - 2, n - 1}))


def _diag():
    return R.DiagonalMassMatrixTuner(10, 1.5, 5, 5)


def size_cases(d):
    hmc = R.make_config(20, 40, R.HMCSampler(5), R.DualAvgTuner(0.8), _diag())
    ehmc = lambda: R.make_config(20, 40, R.EHMCSampler(64, 1, 100, 0.1), R.DualAvgTuner(0.8), _diag())
    nuts = lambda: R.make_config(20, 40, R.NUTSSampler(5), R.DualAvgTuner(0.8), _diag())
    s0 = 5000 + 100 * d
    out = [Case("sizes", d, "hmc7", d, hmc, _seeds("sizes", d, "hmc7", s0, 7), tuple(range(7)), None),
           Case("sizes", d, "ehmc3", d, ehmc(), _seeds("sizes", d, "ehmc3", s0 + 10, 3), (0, 1, 2), None),
           Case("sizes", d, "nuts3", d, nuts(), _seeds("sizes", d, "nuts3", s0 + 20, 3), (0, 1, 2), None)]
    if d <= 32:
        out += [Case("sizes", d, "ehmc%d" % MANY, d, ehmc(), tuple(range(s0 + 30, s0 + 30 + MANY)), _ends(MANY), None),
                Case("sizes", d, "nuts%d" % MANY, d, nuts(), tuple(range(s0 + 30, s0 + 30 + MANY)), _ends(MANY), None)]
    return out


def dense_window(d):
    return 3 * d + 20


def dense_cases(d):
    """DenseMassMatrixTuner(W, 1.5, 10, 10) over exactly two windows (W, then int(1.5 W)).  W = 3 d + 20: with W = d + 10 the
    covariance of 63 / 64 parameters comes out indefinite, the Cholesky factor goes NaN and the chain never moves again."""
    W = dense_window(d)
    warm = 10 + W + int(1.5 * W) + 10
    tuner = lambda: R.DenseMassMatrixTuner(W, 1.5, 10, 10)
    return [Case("dense", d, label, d, R.make_config(20, warm, s, R.DualAvgTuner(0.8), tuner()), (7, 8), (0, 1), None)
            for label, s in (("hmc", R.HMCSampler(5)), ("ehmc", R.EHMCSampler(64, 1, 64, 5)), ("nuts", R.NUTSSampler(5)))]


def ring_cases(B):
    """EHMC's step-count ring buffer of B entries, filled and wrapped during B + 40 warm-up iterations"""
    cfg = lambda: R.make_config(10, B + 40, R.EHMCSampler(16, 1, B, 0.3), R.DualAvgTuner(0.8), _diag())
    s0 = 9000 + 10 * B
    return [Case("ring", B, "packed", RING_DIM, cfg(), tuple(range(s0, s0 + MANY)), _ends(MANY), None),
            Case("ring", B, "unpacked", RING_DIM, cfg(), tuple(range(s0, s0 + 3)), (0, 1, 2), None)]


def rng_cases(d):
    """chains that continue a java.util.Random state: one gaussian drawn (a pending nextNextGaussian), two drawn (none pending),
    and both kinds side by side in one launch (chains of one wavefront then pair the elements differently)"""
    cfg = lambda: R.make_config(15, 20, R.HMCSampler(3), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner())
    s0 = 700 + d
    mx = _seeds("rng", d, "mixed", s0, 3)
    return [Case("rng", d, "pending", d, cfg(), (s0,), (0,), ((s0, 1),)),
            Case("rng", d, "fresh", d, cfg(), (s0,), (0,), ((s0, 2),)),
            Case("rng", d, "mixed", d, cfg(), mx, (0, 1, 2), ((mx[0], 1), (mx[1], 2), (mx[2], 3)))]


ALL_CASES = ([c for d in SIZES for c in size_cases(d)] + [c for d in DENSE_SIZES for c in dense_cases(d)] +
             [c for B in RING_SIZES for c in ring_cases(B)] + [c for d in RNG_SIZES for c in rng_cases(d)])


def case_id(c):
    return "%s-%d-%s" % (c.group, c.key, c.label)


def is_dense(c):
    return isinstance(c.config.massMatrixTuner(), R.DenseMassMatrixTuner)


@lru_cache(maxsize=None)
def spec_of(d):
    return models.funnel(d)


def rng_state(seed, drawn):
    """the JRandom of ScalaRNG(seed) after `drawn` gaussians"""
    jr = O.JavaRandom(seed)
    for _ in range(drawn):
        jr.next_gaussian()
    return jr.r


def rng_states_of(c):
    """Model.sample's rng_states of a continued case: (internal state, pending gaussian or None) per chain"""
    out = []
    for seed, drawn in c.rng:
        r = rng_state(seed, drawn)
        out.append((r.seed, r.next_next if r.have_next else None))
    return out


OracleRun = namedtuple("OracleRun", "draws mass stats dense rc")
_cache = {}


def oracle_run(c, chain):
    """chain `chain` of case c on the oracle (deterministic math), computed once: draws [iterations][d], the reported diagonal,
    the statistics, the dense matrix [d][d] (dense cases, else None) and the oracle's status"""
    key = (case_id(c), chain)
    if key not in _cache:
        from tests.test_gpu_parity import _oracle_cfg
        spec = spec_of(c.d)
        ocfg = _oracle_cfg(c.config, O.JM_DET)
        dense = None
        if is_dense(c):
            dense = np.zeros(c.d * c.d); ocfg.dense_out = O._dp(dense)
        dens = O.OracleDensity(spec, O.JM_DET)
        if c.rng is None:
            draws, mass, st, rc = O.sample_chain(dens.fn_ptr, dens.handle, c.d, ocfg, c.seeds[chain])
        else:
            draws, mass, st, rc = O.sample_chain_state(dens.fn_ptr, dens.handle, c.d, ocfg, rng_state(*c.rng[chain]))
        for a in (draws, mass) + (() if dense is None else (dense,)):
            a.setflags(write=False)
        _cache[key] = OracleRun(draws, mass, st, None if dense is None else dense.reshape(c.d, c.d), rc)
    return _cache[key]
