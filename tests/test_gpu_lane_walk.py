"""The lane walk of the gradient row loop (rh_grad_lane_kernel, csrc/device/rh_lane.hip.h): chains in the lanes -- two per lane,
128 per chain group --, the row values in scalar registers, eight wavefronts per workgroup that cut the workgroup's row split into
eight pieces and add their sums through LDS in ascending order.  It is the automatic choice for static HMC from 512 chains and 5.12e8 row-chain
evaluations per gradient on (csrc/lanes_plan.hpp walk_is_lane); here RH_GRAD_WALK=lane forces it at sizes a test can afford: linreg with 65 573 rows (just above
the tick engine's threshold, ragged against the 8- and the 4-row block), in the bench build (8 rows per scalar request) and in a
strict build (JVM-faithful arithmetic: 4 rows per request, and a value-only part, so its mid-trajectory launches walk row_g()).
Against the oracle, and bit for bit against itself: a chain's sums may depend on the row split count only."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests import oracle_lib as O
from tests.test_gpu_fused import _run

pytestmark = pytest.mark.gpu
FAST = dict(fp_contract=True, factor_outputs=True)
STRICT = dict(math_mode=_capi.MATH_STRICT)
LANE = "rh_grad_lane_kernel"
NROWS, NPTS = 65_573, 165


@pytest.fixture(autouse=True)
def lane_walk(monkeypatch):
    monkeypatch.setenv("RH_GRAD_WALK", "lane")


@pytest.fixture(scope="module")
def spec():
    return models.linreg(n=NROWS, k=3)


@pytest.fixture(scope="module", params=["bench", "strict"])
def model(spec, request):
    m = R.Model(spec, device=0, **(FAST if request.param == "bench" else STRICT))
    yield m
    m.close()


@pytest.fixture(scope="module")
def points(spec):
    """165 points and the oracle's (logp, gradient, sum |terms|) at each, computed once"""
    rng = np.random.default_rng(20)
    qs = rng.normal(0.0, 0.7, size=(NPTS, spec.n_params))
    d = O.OracleDensity(spec)
    return qs, np.array([d.update(q) for q in qs]), np.array([d.abs_sums(q) for q in qs])


def _within(lp, g, ref, sums, tol=1e-11):
    got = np.concatenate([lp[:, None], g], axis=1)
    bound = tol * sums + 1e-300      # tests/test_gpu_parity.py's bound, its looser class (the row count lies between its two classes)
    assert np.all(np.abs(got - ref) <= bound), np.max(np.abs(got - ref) / bound)


@pytest.mark.parametrize("chains", [1, 63, 64, 65, 127, 128, 129, 165])
def test_density_and_gradient_against_the_oracle(model, points, chains, monkeypatch):
    # a lane's two chains are slots l and 64 + l of a 128-chain group: counts around both boundaries, and a second, ragged group
    qs, ref, sums = points
    lp, g = model.density_batch(qs[:chains], engine=_capi.ENGINE_TICK)
    _within(lp, g, ref[:chains], sums[:chains])
    if chains == 165:   # ... and it IS another walk than the tile kernel's: other bits somewhere, within the same bound
        monkeypatch.setenv("RH_GRAD_WALK", "tile")
        lp_t, g_t = model.density_batch(qs[:chains], engine=_capi.ENGINE_TICK)
        _within(lp_t, g_t, ref[:chains], sums[:chains])
        assert not (np.array_equal(lp, lp_t) and np.array_equal(g, g_t))


@pytest.mark.parametrize("splits", [
    8192,      # 8197 blocks of 8 rows: two blocks per split, so six of a workgroup's eight wavefronts get no row at all
    16384])    # one block per split (two of 4 rows): the last split holds 5 rows, less than a block of 8; nearly half of the splits are empty
def test_edges_of_the_row_cut(model, points, splits):
    qs, ref, sums = points
    lp, g = model.density_batch(qs[:70], engine=_capi.ENGINE_TICK, grad_splits=splits)
    _within(lp, g, ref[:70], sums[:70])


def test_a_chains_sums_do_not_depend_on_its_company(model, points, monkeypatch):
    qs = points[0]
    lp, g = model.density_batch(qs, engine=_capi.ENGINE_TICK, grad_splits=64)
    # chain 100 alone (slot 0 of a group of one) against chain 100 among 165 (the second chain of lane 36)
    lp1, g1 = model.density_batch(qs[100:101], engine=_capi.ENGINE_TICK, grad_splits=64)
    assert lp1[0] == lp[100] and np.array_equal(g1[0], g[100])
    # a compacted list (the sampler's launches: rh_compact_kernel) against the identity list
    sub = [3, 64, 65, 100, 127, 128, 164]
    monkeypatch.setenv("RH_EVAL_LIVE", ",".join(str(c) for c in sub))
    lp2, g2 = model.density_batch(qs, engine=_capi.ENGINE_TICK, grad_splits=64)
    monkeypatch.delenv("RH_EVAL_LIVE")
    assert np.array_equal(lp2[sub], lp[sub]) and np.array_equal(g2[sub], g[sub])


def test_sampler_against_the_oracle_under_tame_dynamics(spec, model):
    # static step, identity mass: rounding does not grow (the scheme and the tolerances of tests/test_gpu_fused.py)
    from tests.test_gpu_parity import _oracle_cfg
    cfg = R.make_config(9, 0, R.HMCSampler(7), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    seeds = [900 + c for c in range(9)]
    got = _run(model, cfg, seeds)
    assert got[3] == LANE
    for c in (0, 8):
        want, _, _ = O.sample_model(spec, _oracle_cfg(cfg, O.JM_DET), seeds[c])
        np.testing.assert_allclose(got[0][c], want, rtol=1e-9, atol=1e-11, err_msg="lane walk differs from the ORACLE (chain %d)" % c)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_chains_are_bit_identical_within_the_lane_walk(model, monkeypatch):
    cfg = R.make_config(6, 10, R.HMCSampler(7), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    seeds = [2100 + c for c in range(165)]         # two chain groups, the second ragged: two lanes cut at chain 128
    monkeypatch.setenv("RH_LANES", "2")
    two = _run(model, cfg, seeds)
    assert two[3] == LANE
    monkeypatch.setenv("RH_LANES", "1")
    one = _run(model, cfg, seeds)
    assert one[3] == LANE
    _same(two, one)
    monkeypatch.delenv("RH_LANES")
    _same(_run(model, cfg, seeds, pieces=[1, 3, 2]), one)     # rh_sampler_run called piecewise
    monkeypatch.setenv("RH_FUSE", "0")                        # (the lane walk has no fused form: the switch changes nothing)
    _same(_run(model, cfg, seeds), one)


def test_rh_sample_multi_is_independent_of_the_shard_count_under_the_lane_walk(model):
    cfg = R.make_config(4, 8, R.HMCSampler(5), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    seeds = [7000 + c for c in range(165)]
    base = R.sample_multi([model], cfg, seeds)
    clone = model.clone(0)
    tr = R.sample_multi([model, clone, model], cfg, seeds)     # shards of 55 chains: walk and row splits come from the total
    assert np.array_equal(tr.chains, base.chains) and np.array_equal(tr.mass, base.mass)
    assert [s.stepSize for s in tr.stats] == [s.stepSize for s in base.stats]
    clone.close()


def test_gradient_only_launches_walk_row_g_and_leave_the_chains_bit_identical(spec, monkeypatch):
    """The strict build has a value-only part (row_g() differs from row()): a wavefront whose chains all asked for the gradient only
    -- every mid-trajectory request of static HMC -- walks row_g().  Same chains, bit for bit, as with every launch computing the
    value (RH_VALUE_FREE=0): the scheme of tests/test_gpu_live_chains.py for the other row-streaming kernels."""
    m = R.Model(spec, device=0, **STRICT)
    assert "row_g(" in m.hip_source and "HAS_VALUE_ONLY = true" in m.hip_source
    cfg = R.make_config(5, 12, R.HMCSampler(6), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(6, 1.5, 3, 3), engine=_capi.ENGINE_TICK)
    seeds = [7300 + c for c in range(165)]
    lean = _run(m, cfg, seeds)
    assert lean[3] == LANE
    monkeypatch.setenv("RH_VALUE_FREE", "0")
    full = _run(m, cfg, seeds)
    assert full[3] == LANE
    _same(lean, full)
    m.close()


def test_an_explicit_chain_group_size_stays_on_the_tile_walk(spec):
    # an explicit K asks for the tile kernel and builds no lane kernel: forcing the lane walk changes nothing
    cfg = R.make_config(3, 4, R.HMCSampler(3), R.DualAvgTuner(0.8), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)
    m = R.Model(spec, device=0, grad_chains=8, **FAST)
    assert _run(m, cfg, [1, 2, 3])[3] == "rh_grad_fused_kernel"
    m.close()
