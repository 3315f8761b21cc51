"""Rank-normalised split R-hat, bulk ESS and tail ESS on the device (rh_sampler_rank_diagnostics / rh_rank_diagnostics_device,
csrc/device/rh_rank.hip.h) on an MI355X: the CPU tier's shapes through the kernels -- the very bits of the host emulation of the
device text, a second call, a column list with a duplicate, NaN / inf / constant columns --, a buffer whose workspace crosses the cap,
a sampler's own draws (small model, big mode), a predictor's device buffer, and what is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_rank_diagnostics_device_cpu import (CAP, FIELDS, NKINDS, SHAPES, case, emulate, emulated_case, fixture, plan, same_bits, same_results,
                                                    shuffled_with_duplicate)

pytestmark = pytest.mark.gpu


def fields(r):
    return {f: getattr(r, f) for f in FIELDS}


def on_device(d, first=0, count=None, cols=None):
    m, n, k = d.x.shape
    return R.rank_diagnostics_device(d.ptr.value, m, n, k, device=0, first=first, count=count, cols=cols)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off, its sums run in the emulation's order, and log and the normal quantile are
    written out in the header instead of taken from either side's library: the same bits are asked for, in all five outputs."""
    for f in FIELDS:
        assert same_bits(np.asarray(getattr(got, f), dtype=np.float64), np.asarray(emu[f], dtype=np.float64)), (what, f, getattr(got, f), emu[f])
    with np.errstate(invalid="ignore"):
        assert same_bits(got.rhat, np.where(np.isnan(got.rhat_bulk) | np.isnan(got.rhat_folded), np.nan, np.maximum(got.rhat_bulk, got.rhat_folded)))


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_gives_the_bits_of_the_host_emulation(i):
    x, first, count, emu = emulated_case(i)
    chains, _ = SHAPES[i]
    nv = x.shape[2]
    cols = shuffled_with_duplicate(nv, i)
    with DeviceDraws(x) as d:
        got = on_device(d, first, count)
        again = on_device(d, first, count)
        sub = on_device(d, first, count, cols=cols)
    check_against_emulation(got, emu, SHAPES[i])
    assert same_results(fields(again), fields(got)), (SHAPES[i], "a second call")
    assert same_results(fields(sub), fields(got), cols) and sub.cols == tuple(cols) and got.cols == tuple(range(nv))
    for k in range(nv):
        if k % NKINDS == 4:                                   # the constant column
            assert all(np.isnan(getattr(got, f)[k]) for f in FIELDS[:4]) and np.isnan(got.rhat[k]) and got.truncated[k] == 0
        else:
            assert np.isfinite(got.rhat[k]) and np.isfinite(got.ess_bulk[k])
            assert np.isfinite(got.ess_tail[k]) == (2 * chains * (count // 2) >= 20)


def test_device_nan_and_inf_columns_are_nan_and_touch_nothing_else():
    x, first, count = case(5)                                 # 5 chains, count 819, 17 columns
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[1, first + count // 2, 3] = np.nan                    # count is odd: the middle draw is left out, the column stays clean
    bad[0, first - 1, 1] = np.nan                             # outside the window
    with DeviceDraws(x) as d:
        clean = on_device(d, first, count)
    with DeviceDraws(bad) as d:
        got = on_device(d, first, count)
    for k in range(x.shape[2]):
        if k in (0, 6, 9):
            assert all(np.isnan(getattr(got, f)[k]) for f in FIELDS[:4]) and np.isnan(got.rhat[k]) and got.truncated[k] == 0, k
        else:
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in FIELDS), k
    check_against_emulation(got, emulate(bad, first, count), "nan and inf")


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_several_chunks_of_columns():
    """64 chains x 2000 x 40: S = 128 000 and about 4.4 MB of workspace per column, so the 40 columns cross the 128 MiB cap and go in
    two chunks (30 + 10).  Every column has the bits of the call that asks for it alone."""
    m, n, k = 64, 2000, 40
    p = plan(m, n, k)
    assert p["S"] == 128000 and k * p["per_col"] > CAP and p["pc"] == 30 and -(-k // p["pc"]) == 2
    x = fixture(m, n, k, 4000)
    with DeviceDraws(x) as d:
        got = on_device(d)
        for c in range(k):
            one = on_device(d, cols=[c])
            assert same_results(fields(one), fields(got), [c]), c
    for c in range(k):
        if c % NKINDS == 4:
            assert np.isnan(got.rhat[c])
        elif c % NKINDS == 2:
            # one chain of 64 at three times the scale: the folded R-hat sees it, and its draws hold most of either tail, so the
            # tails' indicators do not mix and their lags run out
            assert got.rhat_bulk[c] < 1.01 < got.rhat_folded[c] and got.truncated[c] == 6 and got.ess_tail[c] > 1000
        else:
            assert got.rhat[c] < 1.02 and got.ess_tail[c] > 1000 and got.truncated[c] == 0
    assert np.all(got.ess_bulk[0::NKINDS] > 100000) and np.all(got.ess_bulk[1::NKINDS] < 12000)


# ---- 3. a sampler's own draws ----------------------------------------------------------------------------------------------------------
def test_sampler_rank_diagnostics_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    got = s.rank_diagnostics()                             # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    k = spec.n_params
    assert all(getattr(got, f).shape == (k,) for f in FIELDS) and got.rhat.shape == (k,) and got.cols == tuple(range(k))
    assert same_results(fields(got), fields(R.rank_diagnostics_device(s.draws_device_ptr(), 64, 200, k, device=0)))
    check_against_emulation(got, emulate(before), "eight schools")
    assert np.all(got.rhat < 1.05) and np.all(got.truncated == 0) and np.all(got.ess_bulk > 400) and np.all(got.ess_tail > 400)
    # a window, and a column list on it
    win = s.rank_diagnostics(7, 181)
    check_against_emulation(win, emulate(before, 7, 181), "eight schools, a window")
    cols = [k - 1, 0, 3, 0]
    assert same_results(fields(s.rank_diagnostics(7, 181, cols=cols)), fields(win), cols)
    for first, count in ((0, 201), (150, 51), (0, 3), (-1, 10), (198, 3)):
        with pytest.raises(R.RainierHipError) as e:
            s.rank_diagnostics(first, count)
        assert e.value.code == _capi.RH_E_INVALID
    for cols in ([0, k], [], [-1]):
        with pytest.raises(R.RainierHipError) as e:
            s.rank_diagnostics(cols=cols)
        assert e.value.code == _capi.RH_E_INVALID
    assert "rank" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    s.close(); m.close()


def test_the_rank_kernels_come_from_the_kernel_cache():
    """build() left the code object in the kernel cache: loading it compiles nothing"""
    compiles = _capi.lib().rh_compile_count()
    with DeviceDraws(fixture(2, 12, 2, 3)) as d:
        on_device(d)
    assert _capi.lib().rh_compile_count() == compiles


def test_sampler_rank_diagnostics_big_mode():
    """601 parameters (big mode: the chain vectors live in HBM), HMC(4), 8 chains x 6 iterations: h = 3, a few columns"""
    spec = models.random_walk(600)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    assert "#define RH_BIGN 1\n" in m.hip_source
    cfg = R.make_config(6, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    s = R.Sampler(m, cfg, list(range(70, 78)))
    s.warmup(); s.run(6)
    x = s.draws()
    cols = [600, 0, 299, 17, 0]
    got = s.rank_diagnostics(cols=cols)
    check_against_emulation(got, emulate(x, cols=cols), "big mode")
    check_against_emulation(s.rank_diagnostics(1, 5, cols=cols), emulate(x, 1, 5, cols=cols), "big mode, a window")
    assert np.array_equal(s.draws(), x)
    s.close(); m.close()


def test_rank_diagnostics_of_a_predictors_device_buffer():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values = s.predict(p, first, count, thin)
        ptr = s.predict(p, first, count, thin, to_host=False)
        got = R.rank_diagnostics_device(ptr, 16, values.shape[1], nreq, device=0)
        check_against_emulation(got, emulate(values), ("predictions", first, count, thin))
    p.close(); s.close(); m.close()


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusal():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=47, count=4), dict(first=-1, count=5), dict(count=3), dict(count=0), dict(first=50, count=4),
                   dict(cols=[]), dict(cols=[5]), dict(cols=[0, -1])):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        # one column's workspace beyond the cap is refused from the shape alone, before any launch: the buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.rank_diagnostics_device(d.ptr.value, 2049, 2048, 2, device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        assert on_device(d).rhat.shape == (5,)
