"""PSIS leave-one-out expectations and LOO-PIT on the device (rh_loo_expect_device / rh_sampler_loo_expect,
csrc/device/rh_loo_expect.hip.h) on an MI355X: the CPU tier's shapes through the kernels -- the very bits of the host emulation of the
device text, a second call, a pair list with a duplicate, the tail fit of rh_loo_device --, one buffer for both roles whose workspace
crosses the cap, NaN and infinity in either window, a sampler's predictions and replicated observations (small model, big mode), and
what is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws, hip
from tests.test_loo_device_cpu import NKINDS, SHAPES, fixture, tail_len
from tests.test_loo_expect_device_cpu import (CAP, DOUBLES, FIELDS, VKINDS, case_x, emulate, emulated_case, plan, same_bits, same_results, shuffled_with_duplicate)

pytestmark = pytest.mark.gpu


def fields(r):
    return {f: getattr(r, f) for f in FIELDS}


def on_device(dl, dv, lc, vc, y=None, first=0, count=None, thin=1):
    m, n, nll = dl.x.shape
    return R.loo_expect_device(dl.ptr.value, dv.ptr.value, m, n, nll, dv.x.shape[2], lc, vc, y=y, device=0, first=first, count=count, thin=thin)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off, its sums run in the emulation's order, and exp, log, log1p and expm1 are
    written out in the header instead of taken from either side's library: the same bits are asked for, in all seven outputs."""
    for f in FIELDS:
        a, b = getattr(got, f), emu[f]
        assert (a is None) == (b is None), (what, f)
        if a is not None:
            assert same_bits(a, b), (what, f, a, b)


# ---- 1. synthetic draws at the boundary shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_gives_the_bits_of_the_host_emulation(i):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i)
    pick = shuffled_with_duplicate(len(lc), i)
    with DeviceDraws(x) as dl, DeviceDraws(v) as dv:
        got = on_device(dl, dv, lc, vc, y, first, count, thin)
        again = on_device(dl, dv, lc, vc, y, first, count, thin)
        sub = on_device(dl, dv, [lc[j] for j in pick], [vc[j] for j in pick], y[pick], first, count, thin)
        loo = R.loo_device(dl.ptr.value, *x.shape, device=0, first=first, count=count, thin=thin)
    check_against_emulation(got, emu, SHAPES[i])
    assert same_results(fields(again), fields(got)), (SHAPES[i], "a second call")
    assert same_results(fields(sub), fields(got), pick) and sub.ll_cols == tuple(lc[j] for j in pick) and sub.val_cols == tuple(vc[j] for j in pick)
    assert got.ll_cols == tuple(lc) and got.val_cols == tuple(vc)
    # the tail fit is rh_loo_device's, bit for bit
    assert same_bits(got.pareto_k, loo.pareto_k[lc]) and np.array_equal(got.tail_n, loo.tail_n[lc]), SHAPES[i]
    S = emu["w"].shape[1]
    for k in range(len(lc)):
        if lc[k] % NKINDS == 5:                               # one NaN in the log-likelihood window
            assert all(np.isnan(getattr(got, f)[k]) for f in DOUBLES) and got.tail_n[k] == 0
        else:
            assert np.isfinite(got.mean[k]) and got.var[k] >= 0.0 and 0.0 <= got.pit_lt[k] <= got.pit[k] <= 1.0 and 1.0 <= got.ess[k] <= S, (SHAPES[i], k)
        if lc[k] % NKINDS == 4:                               # the constant log-likelihood: every weight is 1
            assert got.pareto_k[k] == math.inf and got.tail_n[k] == 0 and got.ess[k] == float(S)


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
    yy[4 * 10 + 1] = np.nan
    with DeviceDraws(x) as dl, DeviceDraws(v) as dv:
        clean = on_device(dl, dv, lc, vc, y, first, count, thin)
    with DeviceDraws(bx) as dl, DeviceDraws(bv) as dv:
        got = on_device(dl, dv, lc, vc, yy, first, count, thin)
        none = on_device(dl, dv, lc, vc, None, first, count, thin)
    check_against_emulation(clean, emulated_case(5, -np.inf)[8], "a -inf")
    for k in range(len(lc)):
        if lc[k] in (0, 6, 9, 5, 11):
            assert all(np.isnan(getattr(got, f)[k]) for f in DOUBLES) and got.tail_n[k] == 0, k
        elif vc[k] in (4 * 3, 4 * 4 + 3, 4 * 7 + 2):
            assert all(np.isnan(getattr(got, f)[k]) for f in ("mean", "var", "pit", "pit_lt")), k
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in ("ess", "pareto_k", "tail_n")) and np.isfinite(got.ess[k]), k
        elif k == 4 * 10 + 1:
            assert np.isnan(got.pit[k]) and np.isnan(got.pit_lt[k]) and same_bits(got.mean[k], clean.mean[k]) and same_bits(got.var[k], clean.var[k]), k
        else:
            assert all(same_bits(getattr(got, f)[k], getattr(clean, f)[k]) for f in FIELDS) and np.isfinite(got.mean[k]), k
    check_against_emulation(got, emulate(bx, bv, lc, vc, yy, first, count, thin), "nan and inf")
    assert none.pit is None and none.pit_lt is None and same_results(fields(none), fields(got))


# ---- 2. the workspace cap ----------------------------------------------------------------------------------------------------------------
def test_device_one_buffer_for_both_roles_in_several_chunks():
    """64 chains x 2000 x K, one buffer as log-likelihoods and as values: S = 128 000 and 2 MB of workspace per pair, K two more than
    the cap holds, so the pairs go in two chunks.  Single pairs on both sides of the seam, and the list backwards across it, have the
    bits of the full call."""
    m, n = 64, 2000
    pc = plan(m, n, 1, 1000)["pc"]
    k = pc + 2
    p = plan(m, n, 1, k)
    assert p["S"] == 128000 and p["M"] == tail_len(128000) and k * p["per_pair"] > CAP and p["pc"] == pc == 65 and -(-k // pc) == 2
    x = fixture(m, n, k, 4000, bad_at=5)
    lc = list(range(k))
    vc = [(c + 1) % k for c in lc]
    y = np.linspace(-3.0, 0.0, k)
    with DeviceDraws(x) as d:
        got = on_device(d, d, lc, vc, y)
        for c in (0, 1, 2, 63, 64, 65, 66):
            assert same_results(fields(on_device(d, d, [lc[c]], [vc[c]], y[[c]])), fields(got), [c]), c
        back = lc[::-1]
        assert same_results(fields(on_device(d, d, back, [vc[c] for c in back], y[back])), fields(got), back)
    some = [0, 1, 2, 3, 64, 65, 66]
    emu = emulate(x, x, [lc[c] for c in some], [vc[c] for c in some], y[some])
    for f in FIELDS:
        assert same_bits(np.asarray(getattr(got, f), dtype=np.float64)[some], emu[f]), f
    for c in range(k):
        if c % NKINDS == 5:
            assert np.isnan(got.mean[c]) and np.isnan(got.ess[c])
        elif vc[c] % NKINDS == 5:                             # the value column holds the NaN
            assert np.isnan(got.mean[c]) and np.isfinite(got.ess[c])
        elif c % NKINDS == 0:
            assert 0.0 < got.pareto_k[c] < 0.5 and got.tail_n[c] == tail_len(128000) and got.ess[c] > 64000.0


# ---- 3. a sampler's predictions ---------------------------------------------------------------------------------------------------------
def test_sampler_loo_expect_eight_schools():
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
    got = s.loo_expect(p_ll, p_val, y=yobs)                # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    eight = list(range(8))
    assert got.ll_cols == got.val_cols == tuple(eight) and all(getattr(got, f).shape == (8,) for f in FIELDS)
    # the same figures over the two predictors' device buffers, and from the emulation of their host copies, bit for bit
    ptr_ll, ptr_val = s.predict(p_ll, to_host=False), s.predict(p_val, to_host=False)
    assert same_results(fields(got), fields(R.loo_expect_device(ptr_ll, ptr_val, 64, 200, 8, 8, eight, eight, y=yobs, device=0)))
    check_against_emulation(got, emulate(ll, theta, eight, eight, yobs), "eight schools")
    loo = s.loo(p_ll)
    assert same_bits(got.pareto_k, loo.pareto_k) and np.array_equal(got.tail_n, loo.tail_n)
    # leaving a school out pulls its effect towards the others: the school with the largest observation has the largest shift down
    plain = theta.reshape(-1, 8).mean(axis=0)
    assert got.mean[0] < plain[0] and np.all(got.ess > 100.0) and np.all(got.var > 0.0)
    # replicated observations from the generator: the values are Sampler.generate's with the same seed
    rep = s.loo_expect(p_ll, p_val, y=yobs, generator=g, seed=11)
    check_against_emulation(rep, emulate(ll, yrep, eight, eight, yobs), "eight schools, y_rep")
    assert np.all(rep.pit > 0.0) and np.all(rep.pit < 1.0) and np.all(rep.pit_lt <= rep.pit) and same_bits(rep.ess, got.ess)
    assert not same_bits(s.loo_expect(p_ll, p_val, y=yobs, generator=g, seed=12).mean, rep.mean)
    # a window with thinning, and a pair list on it
    win = s.loo_expect(p_ll, p_val, y=yobs, first=7, count=181, thin=3)
    check_against_emulation(win, emulate(s.predict(p_ll, 7, 181, 3), s.predict(p_val, 7, 181, 3), eight, eight, yobs), "eight schools, a thinned window")
    cols = [7, 0, 3, 0]
    assert same_results(fields(s.loo_expect(p_ll, p_val, cols, cols, yobs[cols], first=7, count=181, thin=3)), fields(win), cols)
    wrep = s.loo_expect(p_ll, p_val, cols, [0, 7, 3, 3], yobs[cols], generator=g, seed=5, first=7, count=181, thin=3)
    check_against_emulation(wrep, emulate(s.predict(p_ll, 7, 181, 3), s.generate(p_val, g, 5, 7, 181, 3), cols, [0, 7, 3, 3], yobs[cols]), "y_rep, a thinned window")
    assert compiles == _capi.lib().rh_compile_count()
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.loo_expect(p_ll, p_val, first=first, count=count, thin=thin)
        assert e.value.code == _capi.RH_E_INVALID
    for cols in ([0, 8], [], [-1]):
        for kw in (dict(ll_cols=cols, val_cols=[0] * len(cols)), dict(ll_cols=[0] * len(cols), val_cols=cols)):
            with pytest.raises(R.RainierHipError) as e:
                s.loo_expect(p_ll, p_val, **kw)
            assert e.value.code == _capi.RH_E_INVALID
    g3 = R.Generator([R.gen.Normal(R.gen.col(0), 1.0)], 3, device=0)     # reads 3 columns: not p_val's width
    with pytest.raises(R.RainierHipError) as e:
        s.loo_expect(p_ll, p_val, [0], [0], generator=g3)
    assert e.value.code == _capi.RH_E_INVALID
    assert "loo" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    g3.close(); g.close(); p_ll.close(); p_val.close(); s.close(); m.close()


def test_the_loo_expect_kernels_come_from_the_kernel_cache():
    """build() left the code object in the kernel cache: loading it compiles nothing"""
    compiles = _capi.lib().rh_compile_count()
    with DeviceDraws(fixture(2, 12, 2, 3)) as d:
        on_device(d, d, [0, 1], [1, 0])
    assert _capi.lib().rh_compile_count() == compiles


def test_loo_expect_device_big_mode():
    """601 parameters (big mode: the chain vectors live in HBM), HMC(4), 8 chains x 6 iterations: the draws themselves as both buffers
    of 601 columns, a few of them paired (S = 48, and 16 with a thinned window)"""
    spec = models.random_walk(600)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    assert "#define RH_BIGN 1\n" in m.hip_source
    cfg = R.make_config(6, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    s = R.Sampler(m, cfg, list(range(70, 78)))
    s.warmup(); s.run(6)
    x = s.draws()
    lc, vc = [600, 0, 299, 17, 0], [0, 600, 17, 17, 1]
    y = np.array([x[0, 2, c] for c in vc])
    ptr = s.draws_device_ptr()
    check_against_emulation(R.loo_expect_device(ptr, ptr, 8, 6, 601, 601, lc, vc, y=y, device=0), emulate(x, x, lc, vc, y), "big mode")
    check_against_emulation(R.loo_expect_device(ptr, ptr, 8, 6, 601, 601, lc, vc, device=0, first=1, count=4, thin=3), emulate(x, x, lc, vc, None, 1, 4, 3),
                            "big mode, a thinned window")
    assert np.array_equal(s.draws(), x)
    s.close(); m.close()


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
        with pytest.raises(R.RainierHipError) as e:          # S < 2
            R.loo_expect_device(d.ptr.value, d.ptr.value, 1, 50, 5, 5, [0], [1], device=0, count=1)
        assert e.value.code == _capi.RH_E_INVALID and "at least 2" in str(e.value)
        # one pair's workspace beyond the cap, and a tail beyond the LDS, are refused from the shape alone, before any launch: the
        # buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.loo_expect_device(d.ptr.value, d.ptr.value, 4097, 2048, 2, 2, [0], [1], device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)
        with pytest.raises(R.RainierHipError) as e:
            R.loo_expect_device(d.ptr.value, d.ptr.value, 3600, 2048, 2, 2, [0], [1], device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "LDS" in str(e.value)
        assert on_device(d, d, [0, 4], [1, 1]).mean.shape == (2,)


def test_the_values_on_another_device_are_refused():
    if _capi.lib().rh_device_count() < 2:
        pytest.skip("one device visible")
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        other = C.c_void_p()
        assert hip().hipSetDevice(1) == 0 and hip().hipMalloc(C.byref(other), x.nbytes) == 0
        try:
            assert hip().hipMemcpy(other, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
            assert hip().hipSetDevice(0) == 0
            with pytest.raises(R.RainierHipError) as e:
                R.loo_expect_device(d.ptr.value, other.value, 3, 50, 5, 5, [0], [1], device=0)
            assert e.value.code == _capi.RH_E_INVALID and "different devices" in str(e.value)
        finally:
            hip().hipSetDevice(1); hip().hipFree(other); hip().hipSetDevice(0)
