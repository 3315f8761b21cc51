"""The lane walk of the gradient row loop (rh_grad_lane_kernel, csrc/device/rh_lane.hip.h) on every model shape that gets one
(tests/lane_walk_cases.py) -- tests/test_gpu_lane_walk.py runs linreg with three covariates only.  Reached here and not there: a
second row target (the rh_lane_targets<T + 1> recursion, the TG::ROWT slot of the partial sums, the LDS buffer used again behind the
second barrier, a target's own row count under a split count sized from another), a target with fewer sums than RH_NACC_MAX, eight
sums (64 KB of static LDS), four rows per scalar request in a fast build, row_g() in a fast build, one column, row code of 230+
vector registers, a target shorter than one block of rows, and a chain whose sums are not finite next to finite ones.
RH_GRAD_WALK=lane forces the walk at sizes a test can afford; every case first proves that the walk ran.  The yardstick is the
oracle's interpreter under the project's bound (as in tests/test_gpu_fuzz.py): 1e-12 * sum |term| per output."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi
from tests import oracle_lib as O
from tests.lane_walk_cases import FUZZ_LANE, FUZZ_SLOTS, BUILDS, POSITIVE, fuzz_spec
from tests.test_gpu_fused import _run

pytestmark = pytest.mark.gpu
LANE = "rh_grad_lane_kernel"
TOL = 1e-12
NPTS = 165
SPLITS = (0, 8, 1100)      # the walk's own count (8 at these sizes), 8, and more splits than the shortest -- and any -- target has blocks
BY_NAME = {c.name: c for c in POSITIVE}


@pytest.fixture(autouse=True)
def lane_walk(monkeypatch):
    monkeypatch.setenv("RH_GRAD_WALK", "lane")


_main = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for entry in _main.values():
        entry[1].close()
    _main.clear()


def main(case):
    """the case at its main size: (spec, model, 165 points, the oracle's outputs and sums of |term| at each), made once"""
    if case.name not in _main:
        spec, qs = case.make(case.n_main, NPTS)
        ref, sums = _oracle(spec, qs)
        _main[case.name] = (spec, R.Model(spec, device=0, **case.opts), qs, ref, sums)
    return _main[case.name]


def _oracle(spec, qs):
    d = O.OracleDensity(spec)
    both = [d.update_both(q) for q in qs]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


def _ratio(lp, g, ref, sums):
    """|got - ref| / sum |term| per output; equal values (two infinities) and a NaN on both sides count as no difference"""
    got = np.concatenate([lp[:, None], g], axis=1)
    with np.errstate(invalid="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        return np.where(same, 0.0, np.abs(got - ref) / (sums + 1e-300))


def _within(label, lp, g, ref, sums):
    ratio = _ratio(lp, g, ref, sums)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))
    print("lane-walk-worst %s %.3g" % (label, worst / TOL))      # in units of the bound
    assert worst <= TOL, (label, worst / TOL)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_run(a, b):
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and _same_bits(np.array(a[2]), np.array(b[2]))


def _tame(iterations, steps, eps):
    return R.make_config(iterations, 0, R.HMCSampler(steps), R.StaticStepSize(eps), R.IdentityMassMatrixTuner(), engine=_capi.ENGINE_TICK)


@pytest.mark.parametrize("case", POSITIVE, ids=repr)
def test_the_lane_walk_is_what_runs(case):
    # no tolerance test below means anything if the engine quietly fell back to the tile walk
    spec, m, qs, _, _ = main(case)
    assert _run(m, _tame(3, 3, 1e-3), [11, 12, 13])[3] == LANE


@pytest.mark.parametrize("chains", [1, 64, 65, 128, 129])
@pytest.mark.parametrize("case", POSITIVE, ids=repr)
def test_density_and_gradient_against_the_oracle(case, chains):
    # a lane's two chains are slots l and 64 + l of a 128-chain group: one chain, both boundaries, and a second group of one chain
    spec, m, qs, ref, sums = main(case)
    for splits in SPLITS:
        lp, g = m.density_batch(qs[:chains], engine=_capi.ENGINE_TICK, grad_splits=splits)
        _within("%s chains=%d splits=%d" % (case, chains, splits), lp, g, ref[:chains], sums[:chains])


@pytest.mark.parametrize("case", POSITIVE, ids=repr)
def test_row_counts_around_the_block_and_the_split(case):
    """Every row count is a model of its own (the code object is the same one).  A target shorter than one block of R rows lies in
    the ragged loop of split 0's wavefront 0 and every other (split, wavefront) stores zeros for it: where no target has more rows
    than one block, the outputs are the same bits whatever the split count."""
    for n in case.row_counts:
        spec, qs = case.make(n, 70)                # a ragged chain group: lanes with two chains and lanes with one
        ref, sums = _oracle(spec, qs)
        m = R.Model(spec, device=0, **case.opts)
        got = []
        for splits in SPLITS:
            lp, g = m.density_batch(qs, engine=_capi.ENGINE_TICK, grad_splits=splits)
            _within("%s rows=%s splits=%d" % (case, n, splits), lp, g, ref, sums)
            got.append((lp, g))
        m.close()
        if max(np.atleast_1d(n)) <= case.r:
            for lp, g in got[1:]:
                assert _same_bits(lp, got[0][0]) and _same_bits(g, got[0][1]), (case, n, "a split other than the first added something")


@pytest.mark.parametrize("case", [c for c in POSITIVE if c.value_only], ids=repr)
def test_gradient_only_launches_walk_row_g_and_leave_the_chains_bit_identical(case, monkeypatch):
    """The scheme of tests/test_gpu_lane_walk.py's test of this name, for every build with a value-only part (row_g() differs from
    row()): the strict builds, and the fast builds of fit_normal and of the random models.  129 chains: a full chain group, whose
    lanes all hold two chains, and a group of one."""
    spec, m, _, _, _ = main(case)
    assert "row_g(" in m.hip_source and "HAS_VALUE_ONLY = true" in m.hip_source
    cfg = _tame(4, 5, 1e-3)
    seeds = [7300 + c for c in range(129)]
    lean = _run(m, cfg, seeds)
    assert lean[3] == LANE
    monkeypatch.setenv("RH_VALUE_FREE", "0")
    full = _run(m, cfg, seeds)
    assert full[3] == LANE
    _same_run(lean, full)


@pytest.mark.parametrize("name", ["linreg4-fast", "two_targets-fast", "two_targets-strict"])
def test_a_chains_sums_do_not_depend_on_its_company(name):
    """Chain 100 alone (slot 0 of a group of one) against chain 100 among 165 (the second chain of lane 36); then chain 36 -- the
    first chain of that lane -- gets a scale parameter at which its density is not finite (s = 800: the prior's e^s; s = -800: every
    row's e^(-2s)): its lane partner, its neighbours and every other chain keep their bits."""
    spec, m, qs, _, _ = main(BY_NAME[name])
    lp, g = m.density_batch(qs, engine=_capi.ENGINE_TICK, grad_splits=64)
    lp1, g1 = m.density_batch(qs[100:101], engine=_capi.ENGINE_TICK, grad_splits=64)
    assert _same_bits(lp1[0], lp[100]) and _same_bits(g1[0], g[100])
    others = np.array([c for c in range(NPTS) if c != 36])
    for s in (800.0, -800.0):
        bad = qs.copy()
        bad[36, 0] = s
        lpb, gb = m.density_batch(bad, engine=_capi.ENGINE_TICK, grad_splits=64)
        assert not np.isfinite(lpb[36]), (s, lpb[36])
        for c in (36 + 64, 35, 37):
            assert _same_bits(lpb[c], lp[c]) and _same_bits(gb[c], g[c]), (s, c)
        assert _same_bits(lpb[others], lp[others]) and _same_bits(gb[others], g[others])


@pytest.mark.parametrize("name", ["two_targets-strict", "linreg5-strict"])
def test_sampler_against_the_oracle_under_tame_dynamics(name):
    # static step, identity mass: rounding does not grow (the scheme and the tolerances of tests/test_gpu_lane_walk.py)
    from tests.test_gpu_parity import _oracle_cfg
    spec, m, _, _, _ = main(BY_NAME[name])
    cfg = _tame(9, 7, 2e-3)
    seeds = [900 + c for c in range(9)]
    got = _run(m, cfg, seeds)
    assert got[3] == LANE
    for c in (0, 8):
        want, _, _ = O.sample_model(spec, _oracle_cfg(cfg, O.JM_DET), seeds[c])
        np.testing.assert_allclose(got[0][c], want, rtol=1e-9, atol=1e-11, err_msg="%s: lane walk differs from the ORACLE (chain %d)" % (name, c))


@pytest.mark.parametrize("seed,build", FUZZ_LANE, ids=["slots-%d-%s" % sb for sb in FUZZ_LANE])
def test_random_models_under_the_lane_walk(seed, build):
    """tests/test_gpu_fuzz.py's eight-slot models, at its row counts and points, for every (seed, build) that has a lane kernel"""
    spec, qs, _ = fuzz_spec(seed, dict(FUZZ_SLOTS)[seed], npoints=11)
    assert len(qs) > 0
    qs = np.asarray(qs)
    ref, sums = _oracle(spec, qs)
    m = R.Model(spec, device=0, **BUILDS[build])
    assert _run(m, _tame(3, 3, 1e-3), [4000 + seed, 4100 + seed])[3] == LANE
    for splits in (0, 3):
        lp, g = m.density_batch(qs, engine=_capi.ENGINE_TICK, grad_splits=splits)
        _within("fuzz-slots-%d-%s splits=%d" % (seed, build, splits), lp, g, ref, sums)
    m.close()
