"""Pointwise WAIC and PSIS-LOO on the device (rh_loo_device / rh_sampler_loo, csrc/device/rh_loo.hip.h) on an MI355X: the CPU tier's
shapes through the kernels -- the very bits of the host emulation of the device text, a second call, a column list with a duplicate,
NaN / -inf / constant columns --, a buffer whose workspace crosses the cap, a sampler's predictions (small model, big mode), and what
is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import math

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_loo_device_cpu import (CAP, FIELDS, LOO_MEASURED, NKINDS, SHAPES, case, emulate, emulated_case, fixture, plan, rel, restate, same_bits, same_results,
                                       shuffled_with_duplicate, tail_len, waic_bounds)

pytestmark = pytest.mark.gpu


def fields(r):
    return {f: getattr(r, f) for f in FIELDS}


def on_device(d, first=0, count=None, thin=1, cols=None):
    m, n, k = d.x.shape
    return R.loo_device(d.ptr.value, m, n, k, device=0, first=first, count=count, thin=thin, cols=cols)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off, its sums run in the emulation's order, and exp, log, log1p and expm1 are
    written out in the header instead of taken from either side's library: the same bits are asked for, in all five outputs."""
    for f in FIELDS:
        a, b = np.asarray(getattr(got, f), dtype=np.float64), np.asarray(emu[f], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]) and same_bits(a, b), (what, f, a, b)
    assert same_bits(got.elpd_waic, got.lpd - got.p_waic) and same_bits(got.p_loo, got.lpd - got.elpd_loo)


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_gives_the_bits_of_the_host_emulation(i):
    x, first, count, thin, emu = emulated_case(i)
    nv = x.shape[2]
    cols = shuffled_with_duplicate(nv, i)
    with DeviceDraws(x) as d:
        got = on_device(d, first, count, thin)
        again = on_device(d, first, count, thin)
        sub = on_device(d, first, count, thin, cols=cols)
    check_against_emulation(got, emu, SHAPES[i])
    assert same_results(fields(again), fields(got)), (SHAPES[i], "a second call")
    assert same_results(fields(sub), fields(got), cols) and sub.cols == tuple(cols) and got.cols == tuple(range(nv))
    for k in range(nv):
        if k % NKINDS == 5:                                   # one NaN in the window
            assert all(np.isnan(getattr(got, f)[k]) for f in FIELDS[:4]) and got.tail_n[k] == 0
        elif k % NKINDS == 4:                                 # the constant column
            assert got.lpd[k] == -2.0 and got.p_waic[k] == 0.0 and got.elpd_loo[k] == -2.0 and got.pareto_k[k] == math.inf and got.tail_n[k] == 0
        elif k % NKINDS != 2:                                 # (a column rounded to quarters may be constant at the smallest S)
            assert np.isfinite(got.lpd[k]) and np.isfinite(got.elpd_loo[k]) and got.p_waic[k] > 0.0 and 1 <= got.tail_n[k] <= tail_len(emu["sorted"].shape[1])


def test_device_nan_and_inf_columns_are_nan_and_touch_nothing_else():
    x, first, count, thin, emu = emulated_case(5, -np.inf)    # 5 chains, count 819, 13 columns; columns 5 and 11 hold a -inf
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[0, first - 1, 1] = np.nan                             # outside the window
    with DeviceDraws(x) as d:
        clean = on_device(d, first, count, thin)
    with DeviceDraws(bad) as d:
        got = on_device(d, first, count, thin)
    check_against_emulation(clean, emu, "a -inf")
    for k in range(x.shape[2]):
        if k in (0, 6, 9, 5, 11):
            assert all(np.isnan(getattr(got, f)[k]) for f in FIELDS[:4]) and got.tail_n[k] == 0, k
        else:
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in FIELDS) and np.isfinite(got.elpd_loo[k]), k
    check_against_emulation(got, emulate(bad, first, count, thin), "nan and inf")


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_several_chunks_of_columns():
    """64 chains x 2000 x 70: S = 128 000 and 2 MB of workspace per column, so the 70 columns cross the 128 MiB cap and go in two
    chunks (65 + 5).  Every column asked for alone, and a list that straddles the chunks' seam backwards, has the bits of the full call."""
    m, n, k = 64, 2000, 70
    p = plan(m, n, 1, k)
    assert p["S"] == 128000 and k * p["per_col"] > CAP and p["pc"] == 65 and -(-k // p["pc"]) == 2
    x = fixture(m, n, k, 4000, bad_at=5)
    with DeviceDraws(x) as d:
        got = on_device(d)
        for c in (0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68, 69):
            assert same_results(fields(on_device(d, cols=[c])), fields(got), [c]), c
        back = list(range(k - 1, -1, -1))
        assert same_results(fields(on_device(d, cols=back)), fields(got), back)
    some = [0, 1, 2, 3, 4, 5, 63, 64, 65, 66]
    emu = emulate(x, cols=some)
    for f in FIELDS:
        assert same_bits(np.asarray(getattr(got, f), dtype=np.float64)[some], emu[f]), f
    for c in range(k):
        if c % NKINDS == 5:
            assert np.isnan(got.elpd_loo[c])
        elif c % NKINDS == 4:
            assert got.pareto_k[c] == math.inf and got.tail_n[c] == 0
        elif c % NKINDS == 1:
            assert got.pareto_k[c] > 0.7 and got.tail_n[c] == tail_len(128000)
        elif c % NKINDS == 0:
            assert 0.0 < got.pareto_k[c] < 0.5 and got.tail_n[c] == tail_len(128000)


# ---- 3. a sampler's predictions ---------------------------------------------------------------------------------------------------------
def test_sampler_loo_eight_schools():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_loglik()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    before = s.draws()
    s.predict(p)                                           # the predictor's buffer is allocated
    compiles = _capi.lib().rh_compile_count()
    got = s.loo(p)                                         # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    assert all(getattr(got, f).shape == (nreq,) for f in FIELDS) and got.cols == tuple(range(nreq)) and nreq == 8
    # the same figures over the predictions left on the device, bit for bit
    values = s.predict(p)
    ptr = s.predict(p, to_host=False)
    assert values.shape == (64, 200, 8)
    assert same_results(fields(got), fields(R.loo_device(ptr, 64, 200, nreq, device=0)))
    check_against_emulation(got, emulate(values), "eight schools")
    # ... and the numpy restatement applied to the host copy of the same predictions, within the CPU test's bound
    ref = restate(values)
    assert np.array_equal(got.tail_n, ref["tail_n"]) and np.all(got.tail_n <= tail_len(64 * 200)) and np.all(got.tail_n >= tail_len(64 * 200) - 8)   # (a tie at the cutoff shortens a tail)
    for k in range(nreq):
        lpd, b_lpd, pw, b_pw = waic_bounds(values[:, :, k].reshape(-1))
        assert abs(got.lpd[k] - lpd) <= b_lpd and abs(got.p_waic[k] - pw) <= b_pw and rel(lpd, ref["lpd"][k]) <= 1e-15 and rel(pw, ref["p_waic"][k]) <= 1e-15, k
        assert rel(got.elpd_loo[k], ref["elpd_loo"][k]) <= 4 * LOO_MEASURED and rel(got.pareto_k[k], ref["pareto_k"][k], 1.0) <= 4 * LOO_MEASURED, k
    # what the figures say: eight observations, a hierarchical model that shrinks -- every school is predicted, none is a surprise
    assert np.all(got.pareto_k < 1.0) and np.all(got.elpd_loo < got.lpd) and np.all(got.p_waic > 0.0)
    total, se = got.loo()
    assert -35.0 < total < -28.0 and 0.0 < se < 3.0 and abs(got.waic()[0] - total) < 1.0 and 0.0 < got.p_loo_total()[0] < 4.0
    assert R.loo_compare(got, got) == (0.0, 0.0)
    # a window with thinning, and a column list on it
    win = s.loo(p, 7, 181, 3)
    pv = s.predict(p, 7, 181, 3)
    check_against_emulation(win, emulate(pv), "eight schools, a thinned window")
    cols = [7, 0, 3, 0]
    assert same_results(fields(s.loo(p, 7, 181, 3, cols=cols)), fields(win), cols)
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.loo(p, first, count, thin)
        assert e.value.code == _capi.RH_E_INVALID
    for cols in ([0, 8], [], [-1]):
        with pytest.raises(R.RainierHipError) as e:
            s.loo(p, cols=cols)
        assert e.value.code == _capi.RH_E_INVALID
    assert "loo" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    p.close(); s.close(); m.close()


def test_the_loo_kernels_come_from_the_kernel_cache():
    """build() left the code object in the kernel cache: loading it compiles nothing"""
    compiles = _capi.lib().rh_compile_count()
    with DeviceDraws(fixture(2, 12, 2, 3)) as d:
        on_device(d)
    assert _capi.lib().rh_compile_count() == compiles


def test_loo_device_big_mode():
    """601 parameters (big mode: the chain vectors live in HBM), HMC(4), 8 chains x 6 iterations: the draws themselves as a buffer of
    601 columns, a few of them asked for (S = 48, and 16 with a thinned window)"""
    spec = models.random_walk(600)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    assert "#define RH_BIGN 1\n" in m.hip_source
    cfg = R.make_config(6, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    s = R.Sampler(m, cfg, list(range(70, 78)))
    s.warmup(); s.run(6)
    x = s.draws()
    cols = [600, 0, 299, 17, 0]
    got = R.loo_device(s.draws_device_ptr(), 8, 6, 601, device=0, cols=cols)
    check_against_emulation(got, emulate(x, cols=cols), "big mode")
    check_against_emulation(R.loo_device(s.draws_device_ptr(), 8, 6, 601, device=0, first=1, count=4, thin=3, cols=cols), emulate(x, 1, 4, 3, cols=cols),
                            "big mode, a thinned window")
    # ... and the sampler's own call through a predictor that reads 4 of the 601 parameters
    rir, nreq = models.sparse_predict(601)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    check_against_emulation(s.loo(p), emulate(s.predict(p)), "big mode, a predictor")
    check_against_emulation(s.loo(p, 1, 5, 2, cols=[3, 1]), emulate(s.predict(p, 1, 5, 2), cols=[3, 1]), "big mode, a predictor, a thinned window")
    assert np.array_equal(s.draws(), x)
    p.close(); s.close(); m.close()


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusal():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=47, count=4), dict(first=-1, count=5), dict(count=0), dict(first=50, count=1), dict(thin=0),
                   dict(cols=[]), dict(cols=[5]), dict(cols=[0, -1])):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        with pytest.raises(R.RainierHipError) as e:          # S < 2
            R.loo_device(d.ptr.value, 1, 50, 5, device=0, count=1)
        assert e.value.code == _capi.RH_E_INVALID and "at least 2" in str(e.value)
        # one column's workspace beyond the cap, and a tail beyond the LDS, are refused from the shape alone, before any launch: the
        # buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.loo_device(d.ptr.value, 4097, 2048, 2, device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        with pytest.raises(R.RainierHipError) as e:
            R.loo_device(d.ptr.value, 3600, 2048, 2, device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "LDS" in str(e.value)
        assert on_device(d).lpd.shape == (5,)
