"""The rounds of the tick engine (csrc/engine.cpp advance_to_ticks, csrc/lanes_plan.hpp round_launches): a lock-step run -- static
HMC in the sampling phase -- enqueues its whole remainder as ONE round (up to 4096 launches per lane), launch i of every lane before
launch i + 1 of any, and what a round means for Sampler.timing() is read out of its events later: while the next round runs, or,
when nothing follows, at the next timing(), advance or close (two event pools per lane, used alternately).

RH_ROUND_MAX=n lowers the cap, so that runs of 36 launches cross round boundaries: in mid-trajectory at both parities of the fused
path's partial-sum ping-pong (n = 1, 3, 5, 7 against L = 4), and through both event pools several times.

What must hold:
  * the length of the rounds does not change a bit of any chain -- draws, adapted mass, statistics -- on the lane walk, on the fused
    tile path and under a dynamic sampler, whole runs and piecewise ones, and the chains are the one-lane engine's;
  * the timing figures keep their meaning: launches exact, 0 < kernel_ms <= total_ms, chain slots = density evaluations,
    steady launches <= launches;
  * the deferred read-out is invisible: timing() twice gives the same figures, a reset separates runs, a sampler that is never asked
    closes cleanly."""
import contextlib
import os

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models

pytestmark = pytest.mark.gpu
FAST = dict(fp_contract=True, factor_outputs=True)
L, ITERS, WARMUP = 4, 9, 6
ROUND_MAX = [None, 1, 3, 5, 7]
PIECES = [2, 1, 6]


@contextlib.contextmanager
def _env(**kw):
    """the engine's switches for the samplers created inside (None: unset)"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(model, cfg, seeds, pieces=None):
    s = R.Sampler(model, cfg, seeds)
    s.warmup()
    s.timing(reset=True)
    for n in (pieces or [cfg.iterations]):
        s.run(n)
    tim = s.timing()
    stats, mass = s.stats()
    out = dict(draws=s.draws(), mass=mass, tim=tim,
               stats=[(st.leapfrogSteps, st.warmupLeapfrogSteps, st.stepSize, st.meanAcceptProb, st.gradientEvaluations) for st in stats])
    s.close()
    return out


def _same(a, b, what):
    assert np.array_equal(a["draws"], b["draws"]), what
    assert np.array_equal(a["mass"], b["mass"]) and a["stats"] == b["stats"], what


def _hmc_cfg(steps=L, iters=ITERS, warmup=WARMUP):
    return R.make_config(iters, warmup, R.HMCSampler(steps), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)


def _lock_step_figures(t, lanes, kernel, iters=ITERS, steps=L):
    assert t["dominant_kernel"] == kernel
    assert t["launches"] == lanes * iters * steps
    assert 0 < t["kernel_ms"] <= t["total_ms"]
    assert t["chain_slots"] == t["density_evals"]
    assert 0 <= t["steady_launches"] <= t["launches"] and 0 <= t["steady_kernel_ms"] <= t["kernel_ms"]


# ---- the lane walk, forced at a size a test can afford: 165 chains = two chain groups of 128, the second ragged (lanes cut at 128) ----
@pytest.fixture(scope="module")
def lane_case():
    with _env(RH_GRAD_WALK="lane", RH_LANES="1", RH_ROUND_MAX=None):
        m = R.Model(models.linreg(n=2_051, k=3), device=0, **FAST)
        seeds = [3100 + c for c in range(165)]
        one = _run(m, _hmc_cfg(), seeds)
    assert one["tim"]["dominant_kernel"] == "rh_grad_lane_kernel"
    yield m, seeds, one
    m.close()


@pytest.mark.parametrize("round_max", ROUND_MAX)
def test_round_length_leaves_the_lane_walk_bit_identical(lane_case, round_max):
    m, seeds, one = lane_case
    _lock_step_figures(one["tim"], 1, "rh_grad_lane_kernel")
    with _env(RH_GRAD_WALK="lane", RH_LANES="2", RH_ROUND_MAX=round_max):
        whole = _run(m, _hmc_cfg(), seeds)
        pieces = _run(m, _hmc_cfg(), seeds, pieces=PIECES)
    for got, what in ((whole, "whole"), (pieces, "pieces")):
        _same(got, one, "lane walk, RH_ROUND_MAX=%s, %s" % (round_max, what))
        _lock_step_figures(got["tim"], 2, "rh_grad_lane_kernel")
        assert all(st[0] == ITERS * L for st in got["stats"])


# ---- the fused tile path: 37 chains in groups of 8, lanes of 16 and 21 ----
@pytest.fixture(scope="module")
def fused_case():
    with _env(RH_LANES="1", RH_ROUND_MAX=None):
        m = R.Model(models.linreg(n=70_001, k=3), device=0, grad_chains=8, **FAST)
        seeds = [700 + c for c in range(37)]
        one = _run(m, _hmc_cfg(), seeds)
    assert one["tim"]["dominant_kernel"] == "rh_grad_fused_kernel"
    yield m, seeds, one
    m.close()


@pytest.mark.parametrize("round_max", ROUND_MAX)
def test_round_length_leaves_the_fused_path_bit_identical(fused_case, round_max):
    m, seeds, one = fused_case
    _lock_step_figures(one["tim"], 1, "rh_grad_fused_kernel")
    with _env(RH_LANES="2", RH_ROUND_MAX=round_max):
        whole = _run(m, _hmc_cfg(), seeds)
        pieces = _run(m, _hmc_cfg(), seeds, pieces=PIECES)
    for got, what in ((whole, "whole"), (pieces, "pieces")):
        _same(got, one, "fused, RH_ROUND_MAX=%s, %s" % (round_max, what))
        _lock_step_figures(got["tim"], 2, "rh_grad_fused_kernel")
        assert all(st[0] == ITERS * L for st in got["stats"])


def test_a_dynamic_sampler_keeps_its_rounds_and_its_accounting(fused_case):
    """EHMC is not lock-step: rounds of 32 as before, or of 3 under RH_ROUND_MAX=3; the chains and the compacted accounting do not care"""
    m, _, _ = fused_case
    cfg = R.make_config(6, 25, R.EHMCSampler(64, 2), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK,
                        gradSplits=32)
    seeds = [4100 + c for c in range(37)]
    got = {}
    for round_max in (None, 3):
        with _env(RH_LANES="2", RH_ROUND_MAX=round_max):
            got[round_max] = _run(m, cfg, seeds)
    _same(got[3], got[None], "EHMC, RH_ROUND_MAX=3")
    for g in got.values():
        t = g["tim"]
        assert t["dominant_kernel"] == "rh_grad_kernel"
        assert t["chain_slots"] == t["density_evals"] == got[None]["tim"]["density_evals"] > 0
        assert 0 < t["kernel_ms"] <= t["total_ms"] and 0 <= t["steady_launches"] <= t["launches"]


# ---- the deferred read-out ----
def test_timing_is_the_same_whenever_it_is_asked(fused_case):
    m, seeds, _ = fused_case
    with _env(RH_LANES="2", RH_ROUND_MAX=None):
        s = R.Sampler(m, _hmc_cfg(), seeds)
        s.warmup()
        s.timing(reset=True)
        s.run(2)
        a, b = s.timing(), s.timing()          # the first call resolves the run's one round, the second finds nothing left to do
        assert a == b and a["launches"] == 2 * 2 * L and 0 < a["kernel_ms"] <= a["total_ms"]
        c = s.timing(reset=True)
        assert c == a
        s.run(3)                               # the reset separates the runs: the later one only
        d = s.timing()
        assert d["launches"] == 2 * 3 * L and d["chain_slots"] == d["density_evals"] > 0 and 2 * d["density_evals"] == 3 * a["density_evals"] and 0 < d["kernel_ms"] <= d["total_ms"]
        s.run(4)                               # no reset: this run adds to the last
        e = s.timing()
        assert e["launches"] == 2 * 7 * L and e["kernel_ms"] > d["kernel_ms"] and e["total_ms"] > d["total_ms"]
        s.close()


def test_both_event_pools_are_reused_and_launches_stay_exact(fused_case):
    """2 x RH_ROUND_MAX + 1 launches: rounds of 3, 3 and 1 in pools 0, 1 and 0 again; then once more without a question in between,
    so that the first round of the second run finds a round of the first still unread"""
    m, seeds, _ = fused_case
    with _env(RH_LANES="2", RH_ROUND_MAX=3):
        s = R.Sampler(m, _hmc_cfg(steps=7, iters=2, warmup=3), seeds)
        s.warmup()
        s.timing(reset=True)
        s.run(1)
        s.run(1)
        t = s.timing()
        assert t["launches"] == 2 * 2 * 7 and t["chain_slots"] == t["density_evals"] > 0
        assert 0 < t["kernel_ms"] <= t["total_ms"] and t["steady_launches"] <= t["launches"]
        s.close()


def test_a_sampler_that_is_never_asked_closes_cleanly(fused_case):
    m, seeds, one = fused_case
    for round_max in (None, 3):
        with _env(RH_LANES="2", RH_ROUND_MAX=round_max):
            s = R.Sampler(m, _hmc_cfg(), seeds)
            s.warmup()
            s.run(ITERS)
            draws = s.draws()
            s.close()
        assert np.array_equal(draws, one["draws"])
    # the model and the device are as good as before
    with _env(RH_LANES="2", RH_ROUND_MAX=None):
        _same(_run(m, _hmc_cfg(), seeds), one, "after the unasked samplers")
