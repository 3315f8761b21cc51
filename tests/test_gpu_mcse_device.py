"""Monte Carlo standard errors and ESS of the reported figures on the device (rh_sampler_mcse / rh_mcse_device,
csrc/device/rh_mcse.hip.h) on an MI355X: the CPU tier's shapes through the kernels -- the very bits of the host emulation of the
device text in every output, a second call, a column list with a duplicate, NaN / inf / constant columns --, the pin to the rank
diagnostics on the same buffer, a buffer whose workspace crosses the cap, a sampler's own draws, a predictor's device buffer, and
what is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_mcse_device_cpu import CAP, DOUBLES, FIELDS, PROBS, emulate, emulated_case, params, plan, same_results
from tests.test_rank_diagnostics_device_cpu import NKINDS, SHAPES, case, fixture, same_bits, shuffled_with_duplicate

pytestmark = pytest.mark.gpu


def fields(r):
    return {f: getattr(r, f) for f in FIELDS}


def on_device(d, first=0, count=None, cols=None, probs=PROBS, nlags=0):
    m, n, k = d.x.shape
    return R.mcse_device(d.ptr.value, m, n, k, device=0, first=first, count=count, cols=cols, probs=probs, nlags=nlags)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off, its sums run in the emulation's order and the host's part (qbeta, the
    brackets) is the same code on either side: the same bits are asked for, in all eleven outputs."""
    for f in FIELDS:
        assert same_bits(np.asarray(getattr(got, f), dtype=np.float64), np.asarray(emu[f], dtype=np.float64)), (what, f, getattr(got, f), emu[f])


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_gives_the_bits_of_the_host_emulation(i):
    x, first, count, emu = emulated_case(i)
    probs, nlags = params(i)
    nv = x.shape[2]
    cols = shuffled_with_duplicate(nv, i)
    with DeviceDraws(x) as d:
        got = on_device(d, first, count, probs=probs, nlags=nlags)
        again = on_device(d, first, count, probs=probs, nlags=nlags)
        sub = on_device(d, first, count, cols=cols, probs=probs, nlags=nlags)
        rank = R.rank_diagnostics_device(d.ptr.value, *x.shape, device=0, first=first, count=count)
    check_against_emulation(got, emu, SHAPES[i])
    assert got.quantile.shape == (nv, len(probs)) and got.acf.shape == (nv, nlags + 1) and got.probs == tuple(probs)
    assert same_results(fields(again), fields(got)), (SHAPES[i], "a second call")
    assert same_results(fields(sub), fields(got), cols) and sub.cols == tuple(cols) and got.cols == tuple(range(nv))
    # the pin to merged code: the tails' indicator series are the rank diagnostics', through the same arithmetic
    lo, hi = got.ess_quantile[:, 0], got.ess_quantile[:, 2]
    with np.errstate(invalid="ignore"):
        tail = np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.minimum(lo, hi))
    assert same_bits(tail, rank.ess_tail), SHAPES[i]
    assert np.array_equal((got.truncated >> 3) & 1, (rank.truncated >> 1) & 1) and np.array_equal((got.truncated >> 5) & 1, (rank.truncated >> 2) & 1)
    for k in range(nv):
        if k % NKINDS == 4:                                   # the constant column
            assert got.mean[k] == 2.0 and got.sd[k] == 0.0 and np.isnan(got.ess_mean[k]) and np.isnan(got.mcse_mean[k]) and got.truncated[k] == 0
        else:
            assert all(np.isfinite(getattr(got, f)[k]) for f in DOUBLES[:6])


def test_device_nan_and_inf_columns_no_probabilities_and_sixteen():
    x, first, count = case(5)                                 # 5 chains, count 819, 17 columns
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[1, first + count // 2, 3] = np.nan                    # count is odd: the middle draw is left out, the column stays clean
    bad[0, first - 1, 1] = np.nan                             # outside the window
    many = tuple(np.linspace(0.03, 0.97, 16))
    with DeviceDraws(x) as d:
        clean = on_device(d, first, count, nlags=5)
    with DeviceDraws(bad) as d:
        got = on_device(d, first, count, nlags=5)
        none = on_device(d, first, count, probs=(), nlags=255)
        full = on_device(d, first, count, probs=many)
    for k in range(x.shape[2]):
        if k in (0, 6, 9):
            assert all(np.all(np.isnan(getattr(got, f)[k])) for f in DOUBLES) and got.truncated[k] == 0, k
        else:
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in FIELDS), k
    check_against_emulation(got, emulate(bad, first, count, nlags=5), "nan and inf")
    check_against_emulation(none, emulate(bad, first, count, probs=(), nlags=255), "no probabilities, every lag")
    check_against_emulation(full, emulate(bad, first, count, probs=many), "sixteen probabilities")


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_several_chunks_of_columns():
    """64 chains x 2000: S = 128 000 and about 4.65 MB of workspace per column with three probabilities, so 28 columns fill the 128 MiB
    cap and the 29th -- the smallest buffer that does -- makes a second chunk.  The host's part runs once per chunk.  Columns have the
    bits of the call that asks for them alone."""
    m, n = 64, 2000
    p = plan(m, n, 40)
    k = CAP // p["per_col"] + 1
    assert p["S"] == 128000 and k == 29 and (k - 1) * p["per_col"] <= CAP < k * p["per_col"] and plan(m, n, k)["pc"] == k - 1
    x = fixture(m, n, k, 4000)
    with DeviceDraws(x) as d:
        got = on_device(d, nlags=3)
        for c in (0, 1, 2, 27, 28):                           # of the first chunk, its last column, the second chunk's only one
            one = on_device(d, cols=[c], nlags=3)
            assert same_results(fields(one), fields(got), [c]), c
    for c in range(k):
        if c % NKINDS == 4:
            assert np.isnan(got.ess_mean[c]) and got.sd[c] == 0.0
        elif c % NKINDS == 0:
            assert 64000 < got.ess_mean[c] < 256000 and abs(got.mcse_mean[c] - 1.0 / np.sqrt(128000.0)) < 1e-3
        elif c % NKINDS == 1:
            assert got.ess_mean[c] < 12000 and 0.85 < got.acf[c, 1] < 0.95


# ---- 3. other buffers ------------------------------------------------------------------------------------------------------------------
def test_sampler_mcse_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    got = s.mcse(nlags=10)                                 # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    k = spec.n_params
    assert got.mean.shape == (k,) and got.quantile.shape == (k, 3) and got.acf.shape == (k, 11) and got.cols == tuple(range(k)) and got.probs == PROBS
    assert same_results(fields(got), fields(R.mcse_device(s.draws_device_ptr(), 64, 200, k, device=0, nlags=10)))
    check_against_emulation(got, emulate(before, nlags=10), "eight schools")
    summ = s.summary()
    assert np.allclose(got.mean, summ.mean, rtol=1e-12, atol=1e-12) and np.all(got.ess_mean > 400) and np.all(got.mcse_mean < 0.1 * got.sd)
    # a window, and a column list on it
    win = s.mcse(7, 181, probs=(0.5,))
    check_against_emulation(win, emulate(before, 7, 181, probs=(0.5,)), "eight schools, a window")
    cols = [k - 1, 0, 3, 0]
    assert same_results(fields(s.mcse(7, 181, cols=cols, probs=(0.5,))), fields(win), cols)
    for first, count in ((0, 201), (150, 51), (0, 3), (-1, 10), (198, 3)):
        with pytest.raises(R.RainierHipError) as e:
            s.mcse(first, count)
        assert e.value.code == _capi.RH_E_INVALID
    for kw in (dict(cols=[0, k]), dict(cols=[]), dict(cols=[-1]), dict(probs=(0.0,)), dict(probs=(0.5, 1.0)), dict(probs=tuple(np.linspace(0.1, 0.9, 17))),
               dict(nlags=-1), dict(nlags=256)):
        with pytest.raises(R.RainierHipError) as e:
            s.mcse(**kw)
        assert e.value.code == _capi.RH_E_INVALID, kw
    assert "mcse" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    s.close(); m.close()


def test_mcse_of_a_predictors_device_buffer():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values = s.predict(p, first, count, thin)
        ptr = s.predict(p, first, count, thin, to_host=False)
        got = R.mcse_device(ptr, 16, values.shape[1], nreq, device=0, nlags=4)
        check_against_emulation(got, emulate(values, nlags=4), ("predictions", first, count, thin))
    p.close(); s.close(); m.close()


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusal():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=47, count=4), dict(first=-1, count=5), dict(count=3), dict(count=0), dict(first=50, count=4),
                   dict(cols=[]), dict(cols=[5]), dict(cols=[0, -1]), dict(probs=(0.5, 0.0)), dict(probs=(1.0,)), dict(probs=(float("nan"),)),
                   dict(probs=tuple(np.linspace(0.1, 0.9, 17))), dict(nlags=-1), dict(nlags=256)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        # one column's workspace beyond the cap is refused from the shape alone, before any launch: the buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.mcse_device(d.ptr.value, 2183, 2048, 2, device=0, probs=())
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        assert on_device(d).mean.shape == (5,)
