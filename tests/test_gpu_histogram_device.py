"""Posterior histograms and joint count grids on the device (rh_sampler_histogram / rh_histogram_device and the 2-d forms,
csrc/device/rh_hist.hip.h) on an MI355X: the CPU tier's fixtures at its boundary shapes through the kernels -- equality with numpy
(np.histogram over the returned edges, np.histogram2d) and with the host emulation of the device text, a second call, the
sub-list property --, a buffer whose partial counts cross the workspace cap, a sampler's own draws (small model, big mode, a thinned
window), a predictor's device buffer, and the argument errors.  Counts are integers: every comparison is for equality.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_histogram_device_cpu import (CAP, HUGE, KS, NBINS, NS, QUARTERS, SPECIAL, check_1d, check_2d, check_sublist, emulate, emulate2d,
                                             fixture, pairs_for, plan, pooled, same_bits, same_results, shape_for, shuffled_with_duplicate,
                                             window)

pytestmark = pytest.mark.gpu


def on_device(d, first=0, count=None, thin=1, cols=None, bins=20, rng=None):
    m, n, k = d.x.shape
    h = R.histogram_device(d.ptr.value, m, n, k, device=0, first=first, count=count, thin=thin, cols=cols, bins=bins, range=rng)
    assert h.cols == (tuple(range(k)) if cols is None else tuple(cols))
    return h.edges, h.counts, h.under, h.over, h.nan


def on_device2d(d, pairs, first=0, count=None, thin=1, bins=(32, 32), rng=None):
    m, n, k = d.x.shape
    h = R.histogram2d_device(d.ptr.value, m, n, k, pairs, device=0, first=first, count=count, thin=thin, bins=bins, range=rng)
    assert h.pairs == tuple((int(a), int(b)) for a, b in pairs)
    return h.xedges, h.yedges, h.grid, h.outside


def same_results2d(a, b):
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_device_equals_numpy_and_the_host_emulation(n):
    """every K and every bin count at every N (the full cross the CPU tier takes); the thinning alternates over it, so that every
    (N, K), (N, nbins) and (K, nbins) meets both windows somewhere"""
    chains, kept = shape_for(n)
    for ki, k in enumerate(KS):
        for bi, nbins in enumerate(NBINS):
            thin = (1, 3)[(NS.index(n) + ki + bi) % 2]
            first, count, iters = window(kept, thin)
            x = fixture(chains, iters, k, 7 * n + 31 * k + thin)
            cols = shuffled_with_duplicate(k, n + k)
            with DeviceDraws(x) as d:
                got = on_device(d, first, count, thin, bins=nbins)
                again = on_device(d, first, count, thin, bins=nbins)
                sub = on_device(d, first, count, thin, cols=cols, bins=nbins)
            what = (n, k, nbins, thin)
            check_1d(pooled(x, first, count, thin), got, nbins, what)
            assert same_results(got, again), (what, "a second call")
            check_sublist(got, sub, cols, what)
            assert same_results(got, emulate(x, first, count, thin, bins=nbins)), (what, "the host emulation")


@pytest.mark.parametrize("n", NS)
def test_device_pairs_equal_numpy_and_the_host_emulation(n):
    chains, kept = shape_for(n)
    for k, bins, thin in ((7, (32, 32), 1), (14, (64, 64), 3), (6, (7, 300), 1), (5, (4096, 1), 1), (3, (1, 4096), 3), (7, (1, 1), 3)):
        first, count, iters = window(kept, thin)
        x = fixture(chains, iters, k, 13 * n + k + thin)
        pairs = pairs_for(k)
        with DeviceDraws(x) as d:
            got = on_device2d(d, pairs, first, count, thin, bins=bins)
            again = on_device2d(d, pairs, first, count, thin, bins=bins)
        what = (n, k, bins, thin)
        check_2d(pooled(x, first, count, thin), pairs, got, bins[0], bins[1], what)
        assert same_results2d(got, again), (what, "a second call")
        assert same_results2d(got, emulate2d(x, pairs, first, count, thin, bins=bins)), (what, "the host emulation")
        for p, (a, b) in enumerate(pairs):
            if a == b and bins[0] == bins[1]:
                assert got[2][p].sum() == np.trace(got[2][p]), (what, "a pair (a, a) is on the diagonal")


def test_device_given_bounds_and_values_on_edges():
    for n in (65, 4097):
        chains, kept = shape_for(n)
        x = fixture(chains, kept, 14, n)
        rows = pooled(x)
        mixed = [(-1.0, 1.0), (np.nan, np.nan), (-0.5, 0.25), (2.0, 2.0), (1e16, 1e16 + 6.0), None, (0.0, 1.0)] * 2
        as_nan = [(np.nan, np.nan) if r is None else r for r in mixed]
        with DeviceDraws(x) as d:
            quarters = on_device(d, cols=[QUARTERS, QUARTERS + 7], bins=16, rng=(-2.0, 2.0))
            special = on_device(d, cols=[SPECIAL], bins=8, rng=(0.0, 1.5))
            got = on_device(d, bins=20, rng=mixed)
            huge = on_device(d, cols=[HUGE], bins=64)
            pair = on_device2d(d, [(0, SPECIAL), (QUARTERS, 0)], bins=(16, 12), rng=[((-1.0, 1.5), (0.0, 1.0)), ((-2.0, 2.0), None)])
        check_1d(rows[:, [QUARTERS, QUARTERS + 7]], quarters, 16, ("quarters", n), [(-2.0, 2.0)] * 2)
        assert same_bits(quarters[0][0], np.arange(-2.0, 2.25, 0.25)) and quarters[2].sum() == 0 and quarters[3].sum() == 0
        check_1d(rows[:, [SPECIAL]], special, 8, ("special", n), [(0.0, 1.5)])
        assert special[1][0, 0] >= (rows[:, SPECIAL] == 0.0).sum() > 0                 # -0.0 against lo = 0.0 is in the first bin
        check_1d(rows, got, 20, ("mixed", n), as_nan)
        assert same_results(got, emulate(x, bins=20, rng=as_nan))
        check_1d(rows[:, [HUGE]], huge, 64, ("collapsed edges", n))
        assert len(np.unique(huge[0][0])) == 5
        rng2 = [((-1.0, 1.5), (0.0, 1.0)), ((-2.0, 2.0), (np.nan, np.nan))]
        check_2d(rows, [(0, SPECIAL), (QUARTERS, 0)], pair, 16, 12, ("pairs, given", n), rng2)


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_several_chunks_of_column_tiles():
    """4 chains x 16384 x 7 (3.7 MB of draws, N = 65 536, S = 16) with a list of 2100 columns at 1024 bins: 525 tiles of four columns
    with 256.75 KiB of partial counts each cross the 128 MiB cap, so the tiles go in two chunks (510 + 15).  Columns may repeat, so the
    list walks the seven kinds 300 times: every entry must equal its kind's numpy histogram, in both chunks."""
    m, n, k, nbins, ncols = 4, 16384, 7, 1024, 2100
    p = plan(m, n, 1, ncols, nbins)
    assert p["tiles"] == 525 and p["S"] == 16 and p["tiles"] * p["per_tile"] > CAP and p["tc"] == 510
    x = fixture(m, n, k, 2100)
    cols = [c % k for c in range(ncols)]
    with DeviceDraws(x) as d:
        got = on_device(d, cols=cols, bins=nbins)
        base = on_device(d, bins=nbins)
    check_1d(pooled(x), base, nbins, "several chunks, the seven kinds")
    check_sublist(base, got, cols, "several chunks")


# ---- 3. a sampler's own draws ----------------------------------------------------------------------------------------------------------
def test_sampler_histogram_linreg():
    spec = models.linreg(n=1000, k=3, seed=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(200, 200), list(range(300, 364)))
    s.warmup(); s.run(200)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    k = spec.n_params
    h = s.histogram()
    assert h.edges.shape == (k, 21) and h.counts.shape == (k, 20) and h.cols == tuple(range(k))
    got = (h.edges, h.counts, h.under, h.over, h.nan)
    check_1d(pooled(before), got, 20, "linreg")
    assert h.under.sum() == 0 and h.over.sum() == 0 and h.nan.sum() == 0 and np.all(h.counts.sum(axis=1) == 64 * 200)
    assert same_results(got, on_device_ptr(s.draws_device_ptr(), 64, 200, k))
    assert same_results(got, emulate(before))
    dens = h.density
    assert np.allclose((dens * np.diff(h.edges, axis=1)).sum(axis=1), 1.0, rtol=1e-12)
    # a thinned window, a column list on it, given bounds
    win = s.histogram(7, 180, 3, bins=30)
    rows = pooled(before, 7, 180, 3)
    check_1d(rows, (win.edges, win.counts, win.under, win.over, win.nan), 30, "linreg, thinned")
    cols = [k - 1, 0, 0]
    sub = s.histogram(7, 180, 3, cols=cols, bins=30)
    check_sublist((win.edges, win.counts, win.under, win.over, win.nan), (sub.edges, sub.counts, sub.under, sub.over, sub.nan), cols, "linreg, thinned")
    lo, hi = float(np.median(rows[:, 0])), float(rows[:, 0].max())
    cut = s.histogram(7, 180, 3, cols=[0], bins=9, range=(lo, hi))
    check_1d(rows[:, [0]], (cut.edges, cut.counts, cut.under, cut.over, cut.nan), 9, "linreg, given bounds", [(lo, hi)])
    assert cut.under[0] > 0 and cut.over[0] == 0
    # pairs
    pairs = [(0, 1), (k - 1, 0), (1, 1)]
    g = s.histogram2d(pairs, 7, 180, 3)
    check_2d(rows, pairs, (g.xedges, g.yedges, g.grid, g.outside), 32, 32, "linreg, pairs")
    assert g.grid.shape == (3, 32, 32) and np.all(g.outside == 0) and g.grid[2].sum() == np.trace(g.grid[2])
    assert same_results2d((g.xedges, g.yedges, g.grid, g.outside), emulate2d(before, pairs, 7, 180, 3))
    g = s.histogram2d([(0, 1)], bins=(64, 48), range=[((lo, hi), None)])
    check_2d(pooled(before), [(0, 1)], (g.xedges, g.yedges, g.grid, g.outside), 64, 48, "linreg, pairs, given", [((lo, hi), (np.nan, np.nan))])
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        for call in (lambda: s.histogram(first, count, thin), lambda: s.histogram2d([(0, 1)], first, count, thin)):
            with pytest.raises(R.RainierHipError) as e:
                call()
            assert e.value.code == _capi.RH_E_INVALID
    for call in (lambda: s.histogram(cols=[0, k]), lambda: s.histogram(bins=1025), lambda: s.histogram(range=(1.0, 0.0)),
                 lambda: s.histogram2d([(0, k)]), lambda: s.histogram2d([(0, 1)], bins=(65, 64)), lambda: s.histogram2d([])):
        with pytest.raises(R.RainierHipError) as e:
            call()
        assert e.value.code == _capi.RH_E_INVALID
    assert _capi.lib().rh_compile_count() == compiles      # the histogram kernels came from the kernel cache build() filled
    assert "hist" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    s.close(); m.close()


def on_device_ptr(ptr, chains, iters, k, **kw):
    h = R.histogram_device(ptr, chains, iters, k, device=0, **kw)
    return h.edges, h.counts, h.under, h.over, h.nan


def test_sampler_histogram_big_mode_all_parameters():
    """601 parameters (big mode: the chain vectors live in HBM), HMC(4), 8 chains x 6 iterations: 10 column tiles over 48 rows"""
    spec = models.random_walk(600)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    assert "#define RH_BIGN 1\n" in m.hip_source
    cfg = R.make_config(6, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    s = R.Sampler(m, cfg, list(range(70, 78)))
    s.warmup(); s.run(6)
    x = s.draws()
    h = s.histogram()
    assert h.counts.shape == (spec.n_params, 20)
    check_1d(pooled(x), (h.edges, h.counts, h.under, h.over, h.nan), 20, "big mode")
    win = s.histogram(1, 5, 2, bins=128)
    check_1d(pooled(x, 1, 5, 2), (win.edges, win.counts, win.under, win.over, win.nan), 128, "big mode, thinned")
    pairs = [(0, 600), (300, 299)]
    g = s.histogram2d(pairs, bins=(8, 8))
    check_2d(pooled(x), pairs, (g.xedges, g.yedges, g.grid, g.outside), 8, 8, "big mode, pairs")
    assert np.array_equal(s.draws(), x)
    s.close(); m.close()


def test_histogram_of_a_predictors_device_buffer():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values = s.predict(p, first, count, thin)
        ptr = s.predict(p, first, count, thin, to_host=False)
        got = on_device_ptr(ptr, 16, values.shape[1], nreq, bins=25)
        check_1d(pooled(values), got, 25, ("predictions", first, count, thin))
        pairs = [(0, nreq - 1)]
        g = R.histogram2d_device(ptr, 16, values.shape[1], nreq, pairs, device=0, bins=(16, 16))
        check_2d(pooled(values), pairs, (g.xedges, g.yedges, g.grid, g.outside), 16, 16, ("predictions, pairs", first, count, thin))
    p.close(); s.close(); m.close()


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusal():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=49, count=2), dict(first=-1, count=5), dict(count=0), dict(thin=0), dict(first=50, count=1),
                   dict(cols=[]), dict(cols=[5]), dict(cols=[0, -1]), dict(bins=0), dict(bins=1025), dict(rng=(1.0, 0.0)), dict(rng=(0.0, np.inf)),
                   dict(rng=(np.nan, 1.0)), dict(rng=(-1e308, 1e308))):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        for kw in (dict(pairs=[(0, 5)]), dict(pairs=[(-1, 0)]), dict(pairs=[]), dict(bins=(0, 4)), dict(bins=(65, 64)), dict(first=49, count=2),
                   dict(thin=0), dict(rng=((0.0, 1.0), (1.0, 0.0)))):
            with pytest.raises(R.RainierHipError) as e:
                on_device2d(d, **dict(dict(pairs=[(0, 1)]), **kw))
            assert e.value.code == _capi.RH_E_INVALID, kw
        # one tile's partial counts beyond the workspace cap are refused from the shape alone, before any launch: the buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.histogram_device(d.ptr.value, 8169, 4096, 2, device=0, bins=1024)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        assert on_device(d)[1].shape == (5, 20) and on_device2d(d, [(0, 1)])[2].shape == (1, 32, 32)
