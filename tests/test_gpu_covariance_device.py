"""Posterior covariance and correlation on the device (rh_sampler_covariance / rh_covariance_device, csrc/device/rh_cov.hip.h) on
an MI355X: the CPU tier's fixtures at its boundary shapes through the kernels -- the derived bounds against the independent
reference, the very bits of the host emulation of the device text, a second call, symmetry and the sub-matrix property --, a buffer whose partial
sums cross the workspace cap, a sampler's own draws (small model, big mode, a thinned window), a predictor's device buffer, and the
argument errors.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_covariance_device_cpu import (CAP, KS, NS, check_bounds, check_constant_columns, check_properties, check_submatrix,
                                              emulate, fixture, plan, pooled, same_bits, same_results, shape_for, shuffled_with_duplicate,
                                              window)

pytestmark = pytest.mark.gpu


def on_device(d, first=0, count=None, thin=1, cols=None, corr=True):
    m, n, k = d.x.shape
    return R.covariance_device(d.ptr.value, m, n, k, device=0, first=first, count=count, thin=thin, cols=cols, corr=corr)


def check_against_emulation(got, emu, what):
    """The host emulation takes v_mfma_f64_16x16x4_f64 for a chain of fma over k = 0, 1, 2, 3 at the documented lane maps.  The first
    device run of every fixture here gave the emulation's bits, so that is what is asked: the same bits, mean, cov and corr."""
    assert same_bits(got[0], emu[0]), (what, "mean")
    assert same_bits(got[1], emu[1]), (what, "cov", float(np.nanmax(np.abs(np.asarray(got[1]) - np.asarray(emu[1])))))
    assert same_bits(got[2], emu[2]), (what, "corr")


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_device_within_the_derived_bounds_and_against_the_host_emulation(n, k):
    chains, kept = shape_for(n)
    for thin in (1, 3):
        first, count, iters = window(kept, thin)
        x = fixture(chains, iters, k, 7 * n + 31 * k + thin)
        with DeviceDraws(x) as d:
            got = on_device(d, first, count, thin)
            again = on_device(d, first, count, thin)
            cols = shuffled_with_duplicate(k, n + k)
            sub = on_device(d, first, count, thin, cols=cols)
            plain = on_device(d, first, count, thin, corr=False)
        what = (n, k, thin)
        rows = pooled(x, first, count, thin)
        check_bounds(rows, got.mean, got.cov, what)
        check_properties(got.mean, got.cov, got.corr, what)
        check_constant_columns(rows, got.mean, got.cov, got.corr, what)
        assert same_results(got, again), (what, "a second call")
        assert plain.corr is None and same_bits(plain.cov, got.cov) and same_bits(plain.mean, got.mean)
        check_submatrix(got, sub, cols, what)
        check_properties(sub.mean, sub.cov, sub.corr, what, cols)
        assert sub.cols == tuple(cols) and got.cols == tuple(range(k))
        check_against_emulation(got, emulate(x, first, count, thin), what)


def test_device_nan_column_touches_nothing_else():
    for n, k, nan_col in ((4097, 17, 5), (4096, 65, 64), (9, 5, 0)):
        chains, kept = shape_for(n)
        x = fixture(chains, kept, k, n + k, nan_col=nan_col)
        others = [c for c in range(k) if c != nan_col]
        with DeviceDraws(x) as d:
            got = on_device(d)
            without = on_device(d, cols=others)
        rows = pooled(x)
        check_bounds(rows, got.mean, got.cov, ("nan", n, k))
        check_properties(got.mean, got.cov, got.corr, ("nan", n, k))
        check_submatrix(got, without, others, ("nan", n, k))
        assert not np.any(np.isnan(without.cov)) and np.isnan(got.mean[nan_col])
        assert np.all(np.isnan(got.cov[nan_col, :])) and np.all(np.isnan(got.cov[:, nan_col]))
        assert np.all(np.isnan(got.corr[nan_col, :])) and np.all(np.isnan(got.corr[:, nan_col]))
        check_against_emulation(got, emulate(x), ("nan", n, k))


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_several_chunks_of_tile_pairs():
    """4 chains x 5000 x 2600 (416 MB of draws, N = 20 000, S = 5): 861 tile pairs of 160 KiB of partial sums cross the 128 MiB cap,
    so the pairs go in two chunks (819 + 42).  The bounds on every diagonal entry and 200 sampled off-diagonal ones; the sub-matrix
    property for a list whose columns' tile pairs lie in both chunks."""
    m, n, k = 4, 5000, 2600
    p = plan(m, n, 1, k)
    assert p["pairs"] == 861 and p["S"] == 5 and p["pairs"] * p["per_pair"] > CAP and p["pc"] == 819
    rng = np.random.default_rng(2600)
    x = rng.standard_normal((m, n, k))
    x[:, :, 1::4] += 1e6                                      # moved by 1e6 standard deviations
    x[:, :, 2::4] = 0.9 * x[:, :, 0:k - 2:4] + 0.3 * x[:, :, 2::4]   # the pair of the column two to the left
    x[:, :, 3::4] = 2.0                                       # no variance
    cols = [5, 2599, 70, 2300, 1000, 2590, 5, 2562, 2498, 63, 64]    # tiles 0, 1, 15, 35, 39, 40: pairs before and after 819
    with DeviceDraws(x) as d:
        got = on_device(d)
        sub = on_device(d, cols=cols)
    rows = x.reshape(-1, k)
    entries = [(a, a) for a in range(k)] + [(int(a), int(b)) for a, b in rng.integers(0, k, size=(200, 2))] + [(0, 2), (2562, 2560), (2597, 2599)]
    check_bounds(rows, got.mean, got.cov, "several chunks", entries)
    check_properties(got.mean, got.cov, got.corr, "several chunks")
    check_submatrix(got, sub, cols, "several chunks")
    assert np.all(got.cov[3::4, :] == 0.0) and np.all(np.isnan(got.corr[3::4, :]))
    assert 0.9 < got.corr[0, 2] < 0.99 and 0.9 < got.corr[2560, 2562] < 0.99 and abs(got.corr[0, 4]) < 0.05


# ---- 3. a sampler's own draws ----------------------------------------------------------------------------------------------------------
def test_sampler_covariance_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    got = s.covariance(corr=True)
    k = spec.n_params
    assert got.mean.shape == (k,) and got.cov.shape == (k, k) and got.corr.shape == (k, k) and got.cols == tuple(range(k))
    check_bounds(pooled(before), got.mean, got.cov, "eight schools")
    check_properties(got.mean, got.cov, got.corr, "eight schools")
    assert same_results(got, R.covariance_device(s.draws_device_ptr(), 64, 200, k, device=0, corr=True))
    check_against_emulation(got, emulate(before), "eight schools")
    assert np.all(np.diag(got.cov) > 0) and np.all(np.diag(got.corr) == 1.0) and np.all(np.abs(got.corr) <= 1.0 + 1e-12)
    # a thinned window, and a column list on it
    win = s.covariance(7, 180, 3, corr=True)
    rows = pooled(before, 7, 180, 3)
    check_bounds(rows, win.mean, win.cov, "eight schools, thinned")
    check_properties(win.mean, win.cov, win.corr, "eight schools, thinned")
    cols = [k - 1, 0, 3, 0]
    check_submatrix(win, s.covariance(7, 180, 3, cols=cols, corr=True), cols, "eight schools, thinned")
    with DeviceDraws(np.ascontiguousarray(before[:, 7:187:3, :])) as d:       # a window equals its copy, bit for bit
        assert same_results(win, on_device(d))
    assert s.covariance().corr is None
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.covariance(first, count, thin)
        assert e.value.code == _capi.RH_E_INVALID
    with pytest.raises(R.RainierHipError) as e:
        s.covariance(cols=[0, k])
    assert e.value.code == _capi.RH_E_INVALID
    assert _capi.lib().rh_compile_count() == compiles      # the covariance kernels came from the kernel cache build() filled
    assert "cov" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    s.close(); m.close()


def test_sampler_covariance_big_mode_all_parameters():
    """601 parameters (big mode: the chain vectors live in HBM), HMC(4), 8 chains x 6 iterations: 55 tile pairs over 48 rows"""
    spec = models.random_walk(600)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    assert "#define RH_BIGN 1\n" in m.hip_source
    cfg = R.make_config(6, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    s = R.Sampler(m, cfg, list(range(70, 78)))
    s.warmup(); s.run(6)
    x = s.draws()
    got = s.covariance(corr=True)
    assert got.cov.shape == (spec.n_params, spec.n_params)
    check_bounds(pooled(x), got.mean, got.cov, "big mode")
    check_properties(got.mean, got.cov, got.corr, "big mode")
    win = s.covariance(1, 5, 2)
    check_bounds(pooled(x, 1, 5, 2), win.mean, win.cov, "big mode, thinned")
    assert np.array_equal(s.draws(), x)
    s.close(); m.close()


def test_covariance_of_a_predictors_device_buffer():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values = s.predict(p, first, count, thin)
        ptr = s.predict(p, first, count, thin, to_host=False)
        got = R.covariance_device(ptr, 16, values.shape[1], nreq, device=0, corr=True)
        check_bounds(pooled(values), got.mean, got.cov, ("predictions", first, count, thin))
        check_properties(got.mean, got.cov, got.corr, ("predictions", first, count, thin))
    p.close(); s.close(); m.close()


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusal():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=49, count=2), dict(first=-1, count=5), dict(count=0), dict(thin=0), dict(first=50, count=1),
                   dict(cols=[]), dict(cols=[5]), dict(cols=[0, -1])):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        with pytest.raises(R.RainierHipError) as e:            # N < 2
            R.covariance_device(d.ptr.value, 1, 50, 5, device=0, count=3, thin=3)
        assert e.value.code == _capi.RH_E_INVALID and "at least 2" in str(e.value)
        # one tile pair's partial sums beyond the workspace cap (more than 4096 splits) are refused from the shape alone, before any
        # launch: the buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.covariance_device(d.ptr.value, 4097, 4096, 2, device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        assert on_device(d).cov.shape == (5, 5)
