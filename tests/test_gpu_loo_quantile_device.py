"""Leave-one-out predictive quantiles, CRPS and spread on the device (rh_loo_quantile_device / rh_sampler_loo_quantile,
csrc/device/rh_loo_quantile.hip.h) on an MI355X: the CPU tier's shapes through the kernels in both modes -- the very bits of the host
emulation of the device text, a second call, a pair list with a duplicate, the tail fit of rh_loo_device --, a buffer whose workspace
crosses the cap, NaN and infinity in either window, a sampler's predictions and replicated observations, plain mode without a
log-likelihood predictor, and what is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import math

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_loo_device_cpu import NKINDS, SHAPES, fixture, same_bits, tail_len
from tests.test_loo_expect_device_cpu import case_x, shuffled_with_duplicate
from tests.test_loo_quantile_device_cpu import CAP, FIELDS, PROBS, emulate, emulated_case, plan, same_results

pytestmark = pytest.mark.gpu


def fields(r):
    return {f: getattr(r, f) for f in FIELDS}


def on_device(dl, dv, lc, vc, y=None, probs=PROBS, first=0, count=None, thin=1):
    """dl None: plain mode"""
    m, n, nval = dv.x.shape
    return R.loo_quantile_device(None if dl is None else dl.ptr.value, dv.ptr.value, m, n, 0 if dl is None else dl.x.shape[2], nval, None if dl is None else lc, vc,
                                 probs=probs, y=y, device=0, first=first, count=count, thin=thin)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off, the sorted pairs are a function of the multiset, the scan's sums run in the
    emulation's order, and exp and log are written out in the header instead of taken from either side's library: the same bits are
    asked for, in every output."""
    for f in FIELDS:
        a, b = getattr(got, f), emu[f]
        assert (a is None) == (b is None), (what, f)
        if a is not None:
            assert same_bits(a, b), (what, f, a, b)


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_gives_the_bits_of_the_host_emulation(i, plain):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, plain)
    pick = shuffled_with_duplicate(len(lc), i)
    with DeviceDraws(x) as dl, DeviceDraws(v) as dv:
        d = None if plain else dl
        got = on_device(d, dv, lc, vc, y, PROBS, first, count, thin)
        again = on_device(d, dv, lc, vc, y, PROBS, first, count, thin)
        sub = on_device(d, dv, [lc[j] for j in pick], [vc[j] for j in pick], y[pick], PROBS, first, count, thin)
        none = on_device(d, dv, lc, vc, None, PROBS, first, count, thin)
        loo = None if plain else R.loo_device(dl.ptr.value, *x.shape, device=0, first=first, count=count, thin=thin)
    check_against_emulation(got, emu, (SHAPES[i], plain))
    assert same_results(fields(again), fields(got)), (SHAPES[i], "a second call")
    assert same_results(fields(sub), fields(got), pick) and sub.val_cols == tuple(vc[j] for j in pick)
    assert none.crps is None and same_results(fields(none), fields(got))
    assert got.val_cols == tuple(vc) and got.probs == PROBS and got.quantiles.shape == (len(vc), len(PROBS))
    if plain:
        assert got.pareto_k is None and got.tail_n is None and got.ll_cols == ()
    else:
        # the tail fit is rh_loo_device's, bit for bit
        assert got.ll_cols == tuple(lc) and same_bits(got.pareto_k, loo.pareto_k[lc]) and np.array_equal(got.tail_n, loo.tail_n[lc]), SHAPES[i]
    for k in range(len(lc)):
        if np.isnan(emu["spread"][k]):
            assert np.all(np.isnan(got.quantiles[k])) and np.isnan(got.crps[k]) and np.isnan(got.spread[k])
        else:
            assert np.all(np.diff(got.quantiles[k]) >= 0.0) and got.crps[k] >= 0.0 and got.spread[k] >= 0.0, (SHAPES[i], k)
        if not plain and lc[k] % NKINDS == 4:                 # the constant log-likelihood: every weight is 1
            assert got.pareto_k[k] == math.inf and got.tail_n[k] == 0


def test_device_nan_and_inf_in_either_window_touch_their_own_pairs_only():
    x, v, first, count, thin, lc, vc, y = case_x(5, -np.inf)   # 5 chains, count 819, 13 log-likelihood columns; 5 and 11 hold a -inf
    bx, bv, yy = x.copy(), v.copy(), y.copy()
    bx[2, first + 100, 0] = np.nan
    bx[4, first + 7, 6] = np.inf
    bx[0, first + count - 1, 9] = -np.inf
    bx[0, first - 1, 1] = np.nan                              # outside the window
    bv[3, first + 5, 4 * 3 + 0] = np.nan
    bv[0, first, 4 * 4 + 3] = np.inf
    bv[1, first + count - 1, 4 * 7 + 2] = -np.inf
    bv[2, first + count, 4 * 8 + 3] = np.inf                  # outside the window
    yy[4 * 10 + 3] = np.nan
    with DeviceDraws(x) as dl, DeviceDraws(v) as dv:
        clean = on_device(dl, dv, lc, vc, y, PROBS, first, count, thin)
    with DeviceDraws(bx) as dl, DeviceDraws(bv) as dv:
        got = on_device(dl, dv, lc, vc, yy, PROBS, first, count, thin)
        pgot = on_device(None, dv, lc, vc, yy, PROBS, first, count, thin)
    check_against_emulation(clean, emulated_case(5, False, -np.inf)[8], "a -inf")
    canonical = lambda a: np.all(np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64) == np.uint64(0x7ff8000000000000))
    for k in range(len(lc)):
        if lc[k] in (0, 6, 9, 5, 11):
            assert all(canonical(getattr(got, f)[k]) for f in ("quantiles", "crps", "spread", "pareto_k")) and got.tail_n[k] == 0, k
        elif vc[k] in (4 * 3, 4 * 4 + 3, 4 * 7 + 2):
            assert all(canonical(getattr(got, f)[k]) for f in ("quantiles", "crps", "spread")), k
            assert same_bits(got.pareto_k[k], clean.pareto_k[k]) and got.tail_n[k] == clean.tail_n[k], k
        elif k == 4 * 10 + 3:
            assert canonical(got.crps[k]) and all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in ("quantiles", "spread", "pareto_k", "tail_n")), k
        else:
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in FIELDS) and np.all(np.isfinite(got.quantiles[k])), k
    check_against_emulation(got, emulate(bx, bv, lc, vc, yy, PROBS, first, count, thin), "nan and inf")
    check_against_emulation(pgot, emulate(None, bv, lc, vc, yy, PROBS, first, count, thin), "nan and inf, plain mode")


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_one_buffer_for_both_roles_in_several_chunks():
    """64 chains x 2000 x K, one buffer as log-likelihoods and as values: S = 128 000 and 4 MB of workspace per pair, K two more than
    the cap holds, so the pairs go in two chunks (and the sort takes five merge passes: the log-likelihood side ends in the array it
    began in, the pairs in the other buffer).  Single pairs on both sides of the seam, and the list backwards across it, have the bits
    of the full call."""
    m, n = 64, 2000
    pc = plan(m, n, 1, 1000)["pc"]
    k = pc + 2
    p = plan(m, n, 1, k)
    assert p["S"] == 128000 and p["M"] == tail_len(128000) and k * p["per_pair"] > CAP and p["pc"] == pc == 32 and -(-k // pc) == 2 and p["passes"] == 5
    x = fixture(m, n, k, 4000, bad_at=5)
    lc = list(range(k))
    vc = [(c + 1) % k for c in lc]
    y = np.linspace(-3.0, 0.0, k)
    probs = (0.05, 0.5, 0.95)
    with DeviceDraws(x) as d:
        got = on_device(d, d, lc, vc, y, probs)
        for c in (0, 1, 31, 32, 33):
            assert same_results(fields(on_device(d, d, [lc[c]], [vc[c]], y[[c]], probs)), fields(got), [c]), c
        back = lc[::-1]
        assert same_results(fields(on_device(d, d, back, [vc[c] for c in back], y[back], probs)), fields(got), back)
    some = [0, 1, 2, 3, 31, 32, 33]
    emu = emulate(x, x, [lc[c] for c in some], [vc[c] for c in some], y[some], probs)
    for f in FIELDS:
        assert same_bits(np.asarray(getattr(got, f), dtype=np.float64)[some], emu[f]), f
    for c in range(k):
        if c % NKINDS == 5 or vc[c] % NKINDS == 5:            # either column holds the NaN
            assert np.all(np.isnan(got.quantiles[c])) and np.isnan(got.spread[c])
        elif c % NKINDS == 0:
            assert 0.0 < got.pareto_k[c] < 0.5 and got.tail_n[c] == tail_len(128000) and got.quantiles[c][0] < got.quantiles[c][1] < got.quantiles[c][2]


# ---- 3. a sampler's predictions ---------------------------------------------------------------------------------------------------------
def test_sampler_loo_quantile_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    p_ll = R.Predictor(models.eight_schools_loglik()[0], device=0, math_mode=_capi.MATH_STRICT)
    p_val = R.Predictor(models.eight_schools_predict()[0], device=0, math_mode=_capi.MATH_STRICT)
    g = R.Generator([R.gen.Normal(R.gen.col(j), sg) for j, sg in enumerate(models.EIGHT_SCHOOLS_SIGMA)], 8, device=0)
    yobs = np.array(models.EIGHT_SCHOOLS_Y)
    before = s.draws()
    ll, theta = s.predict(p_ll), s.predict(p_val)          # the predictors' buffers are allocated
    yrep = s.generate(p_val, g, 11)
    compiles = _capi.lib().rh_compile_count()
    got = s.loo_quantile(p_ll, p_val, y=yobs)              # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    eight = list(range(8))
    probs = (0.05, 0.5, 0.95)
    assert got.probs == probs and got.ll_cols == got.val_cols == tuple(eight) and got.quantiles.shape == (8, 3)
    # the same figures over the two predictors' device buffers, and from the emulation of their host copies, bit for bit
    ptr_ll, ptr_val = s.predict(p_ll, to_host=False), s.predict(p_val, to_host=False)
    assert same_results(fields(got), fields(R.loo_quantile_device(ptr_ll, ptr_val, 64, 200, 8, 8, eight, eight, y=yobs, device=0)))
    check_against_emulation(got, emulate(ll, theta, eight, eight, yobs, probs), "eight schools")
    loo = s.loo(p_ll)
    assert same_bits(got.pareto_k, loo.pareto_k) and np.array_equal(got.tail_n, loo.tail_n)
    assert np.all(got.quantiles[:, 0] < got.quantiles[:, 1]) and np.all(got.quantiles[:, 1] < got.quantiles[:, 2]) and np.all(got.spread > 0.0)
    assert np.allclose(got.abs_err, got.crps + 0.5 * got.spread) and np.all(np.isfinite(got.scrps))
    # replicated observations from the generator: the values are Sampler.generate's with the same seed
    rep = s.loo_quantile(p_ll, p_val, y=yobs, generator=g, seed=11)
    check_against_emulation(rep, emulate(ll, yrep, eight, eight, yobs, probs), "eight schools, y_rep")
    assert np.all(rep.spread > got.spread) and same_bits(rep.pareto_k, got.pareto_k)       # the observation noise widens every predictive distribution
    assert not same_bits(s.loo_quantile(p_ll, p_val, y=yobs, generator=g, seed=12).quantiles, rep.quantiles)
    # plain mode: the posterior predictive distribution itself
    pl = s.loo_quantile(None, p_val, y=yobs, generator=g, seed=11)
    check_against_emulation(pl, emulate(None, yrep, eight, eight, yobs, probs), "eight schools, y_rep, plain mode")
    assert pl.pareto_k is None and pl.tail_n is None and pl.ll_cols == ()
    # a window with thinning, and a pair list on it
    win = s.loo_quantile(p_ll, p_val, (0.25, 0.75), y=yobs, first=7, count=181, thin=3)
    check_against_emulation(win, emulate(s.predict(p_ll, 7, 181, 3), s.predict(p_val, 7, 181, 3), eight, eight, yobs, (0.25, 0.75)), "eight schools, a thinned window")
    cols = [7, 0, 3, 0]
    assert same_results(fields(s.loo_quantile(p_ll, p_val, (0.25, 0.75), cols, cols, 7, 181, 3, yobs[cols])), fields(win), cols)
    wrep = s.loo_quantile(p_ll, p_val, (0.5,), cols, [0, 7, 3, 3], y=yobs[cols], generator=g, seed=5, first=7, count=181, thin=3)
    check_against_emulation(wrep, emulate(s.predict(p_ll, 7, 181, 3), s.generate(p_val, g, 5, 7, 181, 3), cols, [0, 7, 3, 3], yobs[cols], (0.5,)), "y_rep, a thinned window")
    assert compiles == _capi.lib().rh_compile_count()
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.loo_quantile(p_ll, p_val, first=first, count=count, thin=thin)
        assert e.value.code == _capi.RH_E_INVALID
    for bad in ((), (1.5,), (-0.1, 0.5), tuple([0.5] * 17)):
        with pytest.raises(R.RainierHipError) as e:
            s.loo_quantile(p_ll, p_val, bad)
        assert e.value.code == _capi.RH_E_INVALID
    for cols in ([0, 8], [], [-1]):
        for kw in (dict(ll_cols=cols, val_cols=[0] * len(cols)), dict(ll_cols=[0] * len(cols), val_cols=cols)):
            with pytest.raises(R.RainierHipError) as e:
                s.loo_quantile(p_ll, p_val, **kw)
            assert e.value.code == _capi.RH_E_INVALID
    assert "loo" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    g.close(); p_ll.close(); p_val.close(); s.close(); m.close()


def test_plain_mode_over_linreg_without_a_log_likelihood_predictor():
    spec = models.linreg(n=8, k=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(100, 60), list(range(40, 56)))
    s.warmup(); s.run(60)
    p = R.Predictor(models.linreg_predict(k=3, x=[0.5, -1.0, 2.0]), device=0, math_mode=_capi.MATH_STRICT)
    yhat = s.predict(p)
    nreq = yhat.shape[2]
    cols = list(range(nreq))
    got = s.loo_quantile(None, p, (0.05, 0.5, 0.95), y=np.zeros(nreq))
    check_against_emulation(got, emulate(None, yhat, cols, cols, np.zeros(nreq), (0.05, 0.5, 0.95)), "linreg, plain mode")
    assert got.pareto_k is None and got.val_cols == tuple(cols) and np.all(got.quantiles[:, 0] <= got.quantiles[:, 2])
    # plain quantiles bracket the pooled order statistics next to them
    flat = np.sort(yhat.reshape(-1, nreq), axis=0)
    S = flat.shape[0]
    for c in cols:
        j = int(math.ceil(0.5 * S))
        assert flat[j - 2, c] <= got.quantiles[c, 1] <= flat[j - 1, c]
    p.close(); s.close(); m.close()


def test_the_loo_quantile_kernels_come_from_the_kernel_cache():
    """build() left the code object in the kernel cache: loading it compiles nothing"""
    compiles = _capi.lib().rh_compile_count()
    with DeviceDraws(fixture(2, 12, 2, 3)) as d:
        on_device(d, d, [0, 1], [1, 0])
    assert _capi.lib().rh_compile_count() == compiles


# ---- 4. what is refused ------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments_and_the_shape_only_refusals():
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=47, count=4), dict(first=-1, count=5), dict(count=0), dict(first=50, count=1), dict(thin=0)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, d, [0], [1], **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        for lc, vc in (([], []), ([5], [0]), ([0], [5]), ([0, -1], [0, 0]), ([0, 1], [0, -1])):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, d, lc, vc)
            assert e.value.code == _capi.RH_E_INVALID, (lc, vc)
        for probs in ((), (2.0,), (0.5, math.nan)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, d, [0], [1], probs=probs)
            assert e.value.code == _capi.RH_E_INVALID, probs
        with pytest.raises(R.RainierHipError) as e:          # S < 2
            R.loo_quantile_device(d.ptr.value, d.ptr.value, 1, 50, 5, 5, [0], [1], device=0, count=1)
        assert e.value.code == _capi.RH_E_INVALID and "at least 2" in str(e.value)
        # one pair's workspace beyond the cap is refused from the shape alone, before any launch: the buffer is never read
        for ll in (d.ptr.value, None):
            with pytest.raises(R.RainierHipError) as e:
                R.loo_quantile_device(ll, d.ptr.value, 2049, 2048, 2, 2, None if ll is None else [0], [1], device=0)
            assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        assert on_device(d, d, [0, 4], [1, 1]).quantiles.shape == (2, len(PROBS))
