"""The row feed of the lane walk on the device (csrc/device/rh_lane.hip.h): the walk of rh_grad_lane_kernel
with a target's rows taken from an interleaved copy of its columns, in sets of whole rows requested one compute phase ahead.  Same
rows, same order, same row code: a chain's sums are the column feed's BIT FOR BIT, which is what is tested -- RH_LANE_FEED=cols
against rows, under RH_GRAD_WALK=lane, at row counts whose splits run out, whose pieces are empty, a single set, an odd count of sets
and a ragged tail of single rows (tests/lane_feed_cases.py) -- besides the oracle's bound of tests/test_gpu_lane_walk.py."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi
from tests import lane_feed_cases as FC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
TICK = _capi.ENGINE_TICK


@pytest.fixture(autouse=True)
def lane_walk(monkeypatch):
    monkeypatch.setenv("RH_GRAD_WALK", "lane")


def _run(model, cfg, seeds):
    """tests/test_gpu_fused.py's _run, with the feed the sampler's launches took: -> (draws, mass, stats, kernel, feed)"""
    s = R.Sampler(model, cfg, seeds)
    s.warmup()
    s.timing(reset=True)
    s.run(cfg.iterations)
    tim = s.timing()
    stats, mass = s.stats()
    out = (s.draws(), mass, [(st.leapfrogSteps, st.stepSize, st.meanAcceptProb, st.gradientEvaluations) for st in stats], tim["dominant_kernel"],
           s.lane_feed())
    s.close()
    return out


def _points(spec, n=FC.CHAINS):
    return np.random.default_rng(20).normal(0.0, 0.7, size=(n, spec.n_params))


def _cfg(tuner=None):
    return R.make_config(FC.ITERATIONS, 4, R.HMCSampler(FC.L), R.DualAvgTuner(0.8), tuner or R.IdentityMassMatrixTuner(), engine=TICK,
                         gradSplits=FC.SPLITS)


def _seeds(base):
    return [base + c for c in range(FC.CHAINS)]


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _both_feeds(monkeypatch, case, n):
    """one evaluation at 130 points and a short sampler run of 130 chains under each feed -> {feed: (logp, gradient, run)}"""
    spec = case.make(n)
    m = R.Model(spec, device=0, **case.opts)
    qs = _points(spec)
    out = {}
    for feed in ("cols", "rows"):
        monkeypatch.setenv("RH_LANE_FEED", feed)
        lp, g = m.density_batch(qs, engine=TICK, grad_splits=FC.SPLITS)
        out[feed] = (lp, g, _run(m, _cfg(), _seeds(5100)))
    m.close()
    return out


@pytest.mark.parametrize("n", FC.ROW_COUNTS)
@pytest.mark.parametrize("build", ["fast", "strict"])
def test_the_two_feeds_give_every_chain_the_same_bits(build, n, monkeypatch):
    got = _both_feeds(monkeypatch, FC.BY_NAME["linreg3-%s" % build], n)
    (lp_c, g_c, run_c), (lp_r, g_r, run_r) = got["cols"], got["rows"]
    assert run_c[3:] == (FC.LANE, "cols") and run_r[3:] == (FC.LANE, "rows")      # the kernel of either feed, and which feed it was
    assert np.all(np.isfinite(lp_c)) and np.all(np.isfinite(g_c))
    assert np.all(lp_r == lp_c) and np.all(g_r == g_c)
    _same(run_r, run_c)


@pytest.mark.parametrize("case", FC.OTHER_WIDTHS, ids=repr)
def test_the_two_feeds_give_the_same_bits_at_other_column_counts(case, monkeypatch):
    got = _both_feeds(monkeypatch, case, FC.N_MAIN)
    (lp_c, g_c, run_c), (lp_r, g_r, run_r) = got["cols"], got["rows"]
    assert run_c[3:] == (FC.LANE, "cols") and run_r[3:] == (FC.LANE, "rows")
    assert np.all(lp_r == lp_c) and np.all(g_r == g_c)
    _same(run_r, run_c)


@pytest.mark.parametrize("build", ["fast", "strict"])
def test_density_and_gradient_against_the_oracle_under_the_row_feed(build, monkeypatch):
    monkeypatch.setenv("RH_LANE_FEED", "rows")
    case = FC.BY_NAME["linreg3-%s" % build]
    spec = case.make(FC.N_MAIN)
    qs = _points(spec, 12)
    d = O.OracleDensity(spec)
    ref, sums = np.array([d.update(q) for q in qs]), np.array([d.abs_sums(q) for q in qs])
    m = R.Model(spec, device=0, **case.opts)
    for splits in (FC.SPLITS, 0):
        lp, g = m.density_batch(qs, engine=TICK, grad_splits=splits)
        got = np.concatenate([lp[:, None], g], axis=1)
        bound = 1e-11 * sums + 1e-300         # the bound of tests/test_gpu_lane_walk.py
        assert np.all(np.abs(got - ref) <= bound), np.max(np.abs(got - ref) / bound)
    assert _run(m, _cfg(), [1, 2, 3])[3:] == (FC.LANE, "rows")
    m.close()


@pytest.mark.parametrize("n", FC.ROW_COUNTS)
def test_gradient_only_launches_leave_the_chains_bit_identical_under_the_row_feed(n, monkeypatch):
    """the strict build has a value-only part (HAS_VALUE_ONLY): the mid-trajectory launches of static HMC walk row_g(); same chains,
    bit for bit, as with every launch computing the value (RH_VALUE_FREE=0) -- and as under the column feed"""
    monkeypatch.setenv("RH_LANE_FEED", "rows")
    case = FC.BY_NAME["linreg3-strict"]
    m = R.Model(case.make(n), device=0, **case.opts)
    assert "row_g(" in m.hip_source and "HAS_VALUE_ONLY = true" in m.hip_source
    tuner = R.DiagonalMassMatrixTuner(6, 1.5, 3, 3)
    lean = _run(m, _cfg(tuner), _seeds(7300))
    monkeypatch.setenv("RH_VALUE_FREE", "0")
    full = _run(m, _cfg(tuner), _seeds(7300))
    assert lean[3:] == (FC.LANE, "rows") and full[3:] == (FC.LANE, "rows")
    _same(lean, full)
    monkeypatch.delenv("RH_VALUE_FREE")
    monkeypatch.setenv("RH_LANE_FEED", "cols")
    _same(_run(m, _cfg(tuner), _seeds(7300)), lean)
    m.close()


def test_rh_sample_multi_is_independent_of_the_shard_count_under_the_row_feed(monkeypatch):
    monkeypatch.setenv("RH_LANE_FEED", "rows")
    case = FC.BY_NAME["linreg3-fast"]
    m = R.Model(case.make(FC.N_MAIN), device=0, **case.opts)
    cfg, seeds = _cfg(), _seeds(7000)
    base = R.sample_multi([m], cfg, seeds)
    clone = m.clone(0)                        # (a clone has interleaved copies of its own)
    tr = R.sample_multi([m, clone], cfg, seeds)
    assert np.array_equal(tr.chains, base.chains) and np.array_equal(tr.mass, base.mass)
    assert [s.stepSize for s in tr.stats] == [s.stepSize for s in base.stats]
    assert _run(clone, cfg, seeds[:3])[3:] == (FC.LANE, "rows")
    clone.close()
    m.close()


def test_a_model_without_the_kernel_stays_on_the_column_feed(monkeypatch):
    monkeypatch.setenv("RH_LANE_FEED", "rows")
    for name in ("linreg2-fast", "linreg1-strict"):      # NC 3: not eligible; NC 2 in a strict build: built and dropped
        case = FC.BY_NAME[name]
        spec = case.make(FC.N_MAIN)
        m = R.Model(spec, device=0, **case.opts)
        qs = _points(spec, 5)
        lp, g = m.density_batch(qs, engine=TICK, grad_splits=FC.SPLITS)
        assert _run(m, _cfg(), [1, 2, 3])[3:] == (FC.LANE, "cols")
        monkeypatch.setenv("RH_LANE_FEED", "cols")
        lp_c, g_c = m.density_batch(qs, engine=TICK, grad_splits=FC.SPLITS)
        monkeypatch.setenv("RH_LANE_FEED", "rows")
        assert np.all(lp == lp_c) and np.all(g == g_c)
        m.close()


def test_the_copy_holds_all_rows_of_a_model_whose_self_check_ran_on_a_prefix(monkeypatch):
    """Above 2^22 rows the create-time self-check evaluates a prefix of 2^20 + 37 rows, and under RH_GRAD_WALK=lane it is the first to
    ask for the row feed: the interleaved copy must hold the uploaded rows all the same.  One column of 2^22 + 9 rows; the row feed
    against the column feed bit for bit, and against the closed form of the sums."""
    n = (1 << 22) + 9
    case = FC.BY_NAME["fit_normal-fast"]
    spec = case.make(n)
    m = R.Model(spec, device=0, **case.opts)
    qs = _points(spec, 3)
    out = {}
    for feed in ("rows", "cols"):
        monkeypatch.setenv("RH_LANE_FEED", feed)
        out[feed] = m.density_batch(qs, engine=TICK)
    cfg = R.make_config(1, 1, R.HMCSampler(2), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=TICK)
    monkeypatch.setenv("RH_LANE_FEED", "rows")
    assert _run(m, cfg, [1, 2, 3])[3:] == (FC.LANE, "rows")
    m.close()
    assert np.all(np.isfinite(out["rows"][0])) and np.all(out["rows"][0] == out["cols"][0]) and np.all(out["rows"][1] == out["cols"][1])
    d = O.OracleDensity(spec)
    ref, sums = d.update(qs[0]), d.abs_sums(qs[0])
    got = np.concatenate([out["rows"][0][:1], out["rows"][1][0]])
    assert np.all(np.abs(got - ref) <= 1e-11 * sums + 1e-300)
