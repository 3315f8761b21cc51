"""The tick engine's two lanes (csrc/engine.cpp advance_to_ticks, csrc/lanes_plan.hpp): a sampler's chains cut on a chain-group
boundary into two halves that advance independently on two streams, so that one half's gradient launch has the fp64 pipe while the
other sits between two launches, in a tick or in a prologue.  RH_LANES=2 forces the cut at any chain count, RH_LANES=1 is the
single-stream schedule.

What must hold:
  * lanes do not change a bit of any chain -- draws, adapted mass, statistics -- on each row-streaming kernel, under the dynamic
    samplers (whose lanes drift apart) and on the fused static-HMC path, whole runs and piecewise ones;
  * the two-lane engine agrees with the ORACLE's chains, not only with the one-lane engine;
  * the timing figures keep their meaning under overlap: 0 < kernel_ms <= total_ms, chain slots = density evaluations for the
    compacted schedule, launches = the two lanes' launches;
  * everything that reads the single draws buffer afterwards sees what it saw after a one-lane run."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_live_chains import _cases

pytestmark = pytest.mark.gpu


def _run(model, cfg, seeds, pieces=None, extra=None):
    s = R.Sampler(model, cfg, seeds)
    s.warmup()
    s.timing(reset=True)
    for n in (pieces or [cfg.iterations]):
        s.run(n)
    tim = s.timing()
    stats, mass = s.stats()
    out = dict(draws=s.draws(), mass=mass, tim=tim,
               stats=[(st.leapfrogSteps, st.warmupLeapfrogSteps, st.stepSize, st.meanAcceptProb, st.gradientEvaluations) for st in stats])
    if extra:
        out["extra"] = extra(s)
    s.close()
    return out


def _both(monkeypatch, fn):
    """fn() under RH_LANES=1 and under RH_LANES=2"""
    out = []
    for lanes in ("1", "2"):
        monkeypatch.setenv("RH_LANES", lanes)
        out.append(fn())
    monkeypatch.delenv("RH_LANES")
    return out


def _same(a, b, what):
    assert np.array_equal(a["draws"], b["draws"]), what
    assert np.array_equal(a["mass"], b["mass"]) and a["stats"] == b["stats"], what


@pytest.mark.parametrize("sampler", ["ehmc", "nuts"])
@pytest.mark.parametrize("case", range(4))
def test_lanes_leave_every_chain_bit_identical(case, sampler, monkeypatch):
    name, mk, build, kernel = _cases()[case]
    m = R.Model(mk(), device=0, **build)
    smp = R.EHMCSampler(64, 2) if sampler == "ehmc" else R.NUTSSampler(5)
    cfg = R.make_config(6, 25, smp, R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK)
    seeds = [4100 + c for c in range(37)]         # ragged against every chain-group size (4, 8, 16): one lane ends in a partly filled group
    one, two = _both(monkeypatch, lambda: _run(m, cfg, seeds))
    assert two["tim"]["dominant_kernel"] == kernel, name
    _same(two, one, name)
    monkeypatch.setenv("RH_LANES", "2")
    pieces = _run(m, cfg, seeds, pieces=[1, 3, 2])
    monkeypatch.delenv("RH_LANES")
    _same(pieces, one, name + ", piecewise")
    # the compacted schedule still computes the slots it needs, lane by lane
    for got in (two, pieces):
        assert got["tim"]["chain_slots"] == got["tim"]["density_evals"] == one["tim"]["density_evals"], name
        assert 0 < got["tim"]["kernel_ms"] <= got["tim"]["total_ms"], name
    m.close()


@pytest.mark.parametrize("chains", [37, 64])
def test_lanes_on_the_fused_path(chains, monkeypatch):
    spec = models.linreg(n=70_001, k=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True, grad_chains=8)
    cfg = R.make_config(7, 12, R.HMCSampler(4), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    seeds = [700 + c for c in range(chains)]
    one, two = _both(monkeypatch, lambda: _run(m, cfg, seeds))
    assert one["tim"]["dominant_kernel"] == two["tim"]["dominant_kernel"] == "rh_grad_fused_kernel"
    _same(two, one, "fused, %d chains" % chains)
    # lock step: every launch of the one-lane run is one launch of each lane
    assert two["tim"]["launches"] == 2 * one["tim"]["launches"] == 2 * 7 * 4
    assert 0 < two["tim"]["kernel_ms"] <= two["tim"]["total_ms"]
    assert all(st[0] == 7 * 4 for st in two["stats"])
    # piecewise: a batch ends (and a tick absorbs the records) in the middle of the lanes' record ping-pong, at both parities
    monkeypatch.setenv("RH_LANES", "2")
    for pieces in ([2, 1, 4], [1, 1, 5]):
        _same(_run(m, cfg, seeds, pieces=pieces), one, "fused, %d chains, pieces %s" % (chains, pieces))
    monkeypatch.delenv("RH_LANES")
    m.close()


def test_two_lanes_against_the_oracle(monkeypatch):
    """the scheme and the tolerances of test_gpu_live_chains.py::test_compacted_nuts_and_ehmc_against_the_oracle, under two lanes
    (11 chains in groups of 4: lanes of 8 and 3; chains 0 / 5 in lane 0, chain 10 in lane 1)"""
    from tests import oracle_lib as O
    from tests.test_gpu_parity import _oracle_cfg
    monkeypatch.setenv("RH_LANES", "2")
    spec = models.linreg(n=70_001, k=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT, grad_chains=4)
    seeds = [6300 + c for c in range(11)]
    for smp in (R.NUTSSampler(3), R.EHMCSampler(8, 2)):
        cfg = R.make_config(3, 3, smp, R.StaticStepSize(1e-3), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
        got = _run(m, cfg, seeds)
        for c in (0, 5, 10):
            want, _, _ = O.sample_model(spec, _oracle_cfg(cfg, O.JM_DET), seeds[c])
            np.testing.assert_allclose(got["draws"][c], want, rtol=1e-9, atol=1e-11, err_msg="%s, chain %d" % (type(smp).__name__, c))
    m.close()


def test_timing_under_two_lanes(monkeypatch):
    """EHMC on the plain VALU kernel, K = 8, 37 chains: the lanes are chains 0..15 and 16..36.  Each lane runs the launches it would
    run as a sampler of its own (same row splits), and the timing figures add up over the lanes."""
    spec = models.linreg(n=70_001, k=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True, grad_chains=8)
    cfg = R.make_config(6, 25, R.EHMCSampler(64, 2), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK,
                        gradSplits=32)
    seeds = [4100 + c for c in range(37)]
    one, two = _both(monkeypatch, lambda: _run(m, cfg, seeds))
    monkeypatch.setenv("RH_LANES", "1")
    lane0, lane1 = _run(m, cfg, seeds[:16]), _run(m, cfg, seeds[16:])
    monkeypatch.delenv("RH_LANES")
    _same(two, one, "timing run")
    assert np.array_equal(two["draws"][:16], lane0["draws"]) and np.array_equal(two["draws"][16:], lane1["draws"])
    t = two["tim"]
    assert 0 < t["kernel_ms"] <= t["total_ms"]
    assert t["chain_slots"] == t["density_evals"] == one["tim"]["density_evals"]
    assert t["launches"] == lane0["tim"]["launches"] + lane1["tim"]["launches"]
    assert t["steady_launches"] <= t["launches"] and 0 <= t["steady_kernel_ms"] <= t["kernel_ms"]
    assert [st[0] for st in two["stats"]] == [st[0] for st in one["stats"]]           # leapfrogSteps per chain
    m.close()


def test_readers_of_the_draws_buffer_after_a_two_lane_run(monkeypatch):
    spec = models.linreg(n=70_001, k=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True, grad_chains=8)
    cfg = R.make_config(12, 12, R.HMCSampler(4), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    seeds = [900 + c for c in range(37)]

    def readers(s):
        diag, mean, var = s.diagnostics(first=2, count=9, moments=True)
        summ = s.summary(first=1, count=10, thin=2, probs=(0.25, 0.5), hdpi=None)
        return dict(window=s.draws(3, 5), diag=np.array(diag), mean=mean, var=var, q=summ.quantiles, smean=summ.mean, ssd=summ.sd)
    one, two = _both(monkeypatch, lambda: _run(m, cfg, seeds, pieces=[5, 7], extra=readers))
    _same(two, one, "readers")
    assert np.array_equal(two["extra"]["window"], two["draws"][:, 3:8])
    for k, v in one["extra"].items():
        assert np.array_equal(two["extra"][k], v, equal_nan=True), k
    m.close()
