"""Posterior predictive checks on the device (rh_ppc_device / rh_sampler_ppc, csrc/device/rh_ppc.hip.h) on an MI355X: the CPU tier's
shapes through the kernels -- the very bits of the host emulation of the device text in t_rep, t_obs and the counts, a second call --,
duplicated and reordered selections, NaN and infinity, the layout summary_device reads, a sampler's replicated observations, and what
is refused.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws, hip
from tests.test_ppc_device_cpu import (CASES, FRAC_LE, MAX, MEAN, MIN, QUANTILE, SD, SIX, base_buffer, emulate, emulated_case, five_segments, same_bits, selection)

pytestmark = pytest.mark.gpu
MAKE = {MEAN: lambda a: R.ppc.mean(), SD: lambda a: R.ppc.sd(), MIN: lambda a: R.ppc.min(), MAX: lambda a: R.ppc.max(), QUANTILE: R.ppc.quantile, FRAC_LE: R.ppc.frac_le}


def check_of(stats, nin, cols=None, segments=None):
    return R.Check([MAKE[k](a) for k, a in stats], nin, cols=cols, segments=segments, device=0)


def on_device(chk, d, y=None, first=0, count=None, thin=1, to_host=True):
    m, n, nin = d.x.shape
    return R.ppc_device(chk, d.ptr.value, m, n, nin, y=y, first=first, count=count, thin=thin, device=0, to_host=to_host)


def check_against_emulation(got, emu, what):
    """The device text is compiled with contraction off and its sums run in the emulation's order, which the shape alone fixes: the
    same bits are asked for, in every statistic of every draw, in t_obs, and the same counts."""
    S, nout = emu["t_rep"].shape
    assert got.S == S and same_bits(got.t_rep.reshape(S, nout), emu["t_rep"]), what
    if "t_obs" in emu:
        assert same_bits(got.t_obs.reshape(-1), emu["t_obs"]), what
        for f in ("n_gt", "n_eq", "n_bad"):
            assert np.array_equal(getattr(got, f).reshape(-1), emu[f]), (what, f)
    else:
        assert got.t_obs is None and got.n_gt is None and got.n_eq is None and got.n_bad is None


def same_ppc(a, b):
    return same_bits(a.t_rep, b.t_rep) and same_bits(a.t_obs, b.t_obs) and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("n_gt", "n_eq", "n_bad"))


# ---- 1. synthetic replicated draws at the boundary shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_device_gives_the_bits_of_the_host_emulation(i):
    nin, cols, segments = CASES[i][:3]
    x, base, touched, cc, off, stats, first, count, thin, y, emu = emulated_case(i)
    chk = check_of(stats, nin, cols, segments)
    assert (chk.nseg, chk.nstat) == (len(off) - 1, len(stats))
    with DeviceDraws(x) as d:
        got = on_device(chk, d, y, first, count, thin)
        again = on_device(chk, d, y, first, count, thin)
        none = on_device(chk, d, None, first, count, thin)
    check_against_emulation(got, emu, CASES[i][:3])
    assert same_ppc(again, got), "a second call"
    assert same_bits(none.t_rep, got.t_rep) and none.t_obs is None and np.isnan(none.p_ge)
    assert got.t_obs.shape == got.n_gt.shape == got.p_ge.shape == (chk.nseg, chk.nstat)
    chk.close()


def test_device_duplicates_and_reordered_segments_give_the_corresponding_outputs():
    x = base_buffer(40, 2, 25, 9)
    segs = five_segments()
    order = [3, 0, 4, 2, 1, 3]
    a, b = check_of(SIX, 40, segments=segs), check_of(SIX, 40, segments=[segs[g] for g in order])
    one, two = check_of([(MIN, 0.0), (MAX, 0.0), (FRAC_LE, 0.0)], 40, cols=[18]), check_of([(MIN, 0.0), (MAX, 0.0), (FRAC_LE, 0.0), (SD, 0.0), (MEAN, 0.0)], 40, cols=[18, 18])
    with DeviceDraws(x) as d:
        ta, tb = on_device(a, d).t_rep.reshape(50, 30), on_device(b, d).t_rep.reshape(50, 36)
        t1, t2 = on_device(one, d).t_rep.reshape(50, 3), on_device(two, d).t_rep.reshape(50, 5)
    for at, g in enumerate(order):
        assert same_bits(tb[:, at * 6:(at + 1) * 6], ta[:, g * 6:(g + 1) * 6])
    assert same_bits(t2[:, :3], t1) and np.all(t2[:, 3] == 0.0) and same_bits(t2[:, 4], x.reshape(-1, 40)[:, 18])
    for c in (a, b, one, two):
        c.close()


def test_device_nan_and_inf_touch_their_own_draw_and_segment_only():
    x = base_buffer(40, 3, 30, 21)
    segs = five_segments()
    cc, off = selection(40, None, segs)
    bad = x.copy()
    bad[1, 7, 20] = np.nan                                      # segment 3
    bad[2, 29, 17] = np.inf                                     # segment 1, of one column
    bad[0, 0, 5] = np.inf                                       # column 5 is in segments 0 and 4
    chk = check_of(SIX, 40, segments=segs)
    with DeviceDraws(x) as d:
        clean = on_device(chk, d).t_rep
    with DeviceDraws(bad) as d:
        got = on_device(chk, d).t_rep
    touched = np.zeros(clean.shape, dtype=bool)
    touched[1, 7, 3 * 6:4 * 6] = touched[2, 29, 6:12] = touched[0, 0, 0:6] = touched[0, 0, 24:30] = True
    assert np.array_equal(got.view(np.uint64)[~touched], clean.view(np.uint64)[~touched])
    assert np.all(np.isnan(got[1, 7, 18:24]))
    assert got[2, 29, 6] == got[2, 29, 8] == got[2, 29, 9] == got[2, 29, 10] == np.inf and np.isnan(got[2, 29, 7]) and got[2, 29, 11] == 0.0
    assert got[0, 0, 0] == np.inf and np.isnan(got[0, 0, 1]) and np.isfinite(got[0, 0, 2]) and got[0, 0, 3] == np.inf and got[0, 0, 24 + 3] == np.inf
    assert same_bits(got.reshape(90, 30), emulate(bad, cc, off, SIX)["t_rep"])
    chk.close()


def test_summary_device_reads_the_checks_own_buffer():
    """dev_ptr is [chains][kept][nout], the layout every other device call reads: the summary over it is numpy's over t_rep"""
    x = np.random.default_rng(77).standard_normal((4, 60, 24))
    chk = check_of([(MEAN, 0.0), (MAX, 0.0), (QUANTILE, 0.25)], 24, segments=[list(range(10)), list(range(10, 24))])
    with DeviceDraws(x) as d:
        got = on_device(chk, d, first=3, count=55, thin=2)
        dev = on_device(chk, d, first=3, count=55, thin=2, to_host=False)
        assert dev.t_rep is None and dev.dev_ptr == got.dev_ptr and got.t_rep.shape == (4, 28, 6)
        s = R.summary_device(dev.dev_ptr, 4, 28, 6, device=0, probs=(0.0, 0.5, 1.0), hdpi=None)
    flat = got.t_rep.reshape(-1, 6)
    srt = np.sort(flat, axis=0)
    assert np.array_equal(s.quantiles, srt[[0, 56, 111]].T) and np.allclose(s.mean, flat.mean(axis=0), rtol=1e-13, atol=0)
    chk.close()


# ---- 2. a sampler's replicated observations -----------------------------------------------------------------------------------------------
def test_sampler_ppc_is_generate_then_the_check():
    n, k, rows = 300, 3, 20
    cols = models.linreg_data(n, k)
    spec = models.linreg(n=n, k=k)
    m = R.Model(spec, device=0)
    cfg = R.make_config(50, 20, R.HMCSampler(3))
    s = R.Sampler(m, cfg, list(range(500, 564)))
    s.warmup(); s.run(50)
    xs = np.stack([c[:rows] for c in cols[1:]], axis=1)
    p = R.Predictor(models.linreg_fitted(k, xs)[0], device=0)
    g = R.Generator([R.gen.Normal(R.gen.col(j), R.gen.col(rows)) for j in range(rows)], rows + 1, device=0)
    chk = R.Check([R.ppc.mean(), R.ppc.sd(), R.ppc.min(), R.ppc.max(), R.ppc.quantile(0.5), R.ppc.frac_le(0.0)], rows, segments=[list(range(12)), list(range(12, 20))],
                  device=0)
    y = cols[0][:rows]
    before = s.draws()
    seed = 1996
    got = s.ppc(p, g, chk, seed, y=y)
    yrep = s.generate(p, g, seed)                                # the host copy of that call's replicated observations
    ptr = s.generate(p, g, seed, to_host=False)
    over = R.ppc_device(chk, ptr, 64, 50, rows, y=y, device=0)
    assert same_ppc(got, over) and got.S == 3200 and got.t_rep.shape == (64, 50, 12)
    cc, off = selection(rows, None, [list(range(12)), list(range(12, 20))])
    check_against_emulation(got, emulate(yrep, cc, off, SIX, y), "linreg, y_rep")
    assert np.all(got.n_bad == 0) and np.all((0.0 <= got.p_gt) & (got.p_gt <= got.p_mid) & (got.p_mid <= got.p_ge) & (got.p_ge <= 1.0))
    assert not same_bits(s.ppc(p, g, chk, seed + 1, y=y).t_rep, got.t_rep)
    win = s.ppc(p, g, chk, seed, y=y, first=5, count=41, thin=3)
    check_against_emulation(win, emulate(s.generate(p, g, seed, 5, 41, 3), cc, off, SIX, y), "a thinned window")
    dev = s.ppc(p, g, chk, seed, to_host=False)
    assert dev.t_rep is None and dev.t_obs is None and dev.dev_ptr
    # refused: a generator of another width, a broken window
    wide = R.Check([R.ppc.mean()], rows + 1, device=0)
    with pytest.raises(R.RainierHipError) as e:
        s.ppc(p, g, wide, seed)
    assert e.value.code == _capi.RH_E_INVALID and "the check reads 21 columns" in str(e.value)
    for first, count, thin in ((0, 51, 1), (0, 0, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.ppc(p, g, chk, seed, first=first, count=count, thin=thin)
        assert e.value.code == _capi.RH_E_INVALID
    assert "ppc" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)                     # the chains are unaltered
    wide.close(); chk.close(); g.close(); p.close(); s.close(); m.close()


def test_the_ppc_kernels_come_from_the_kernel_cache():
    """build() left the code object in the kernel cache: loading it compiles nothing"""
    compiles = _capi.lib().rh_compile_count()
    chk = check_of(SIX, 8)
    with DeviceDraws(base_buffer(8, 2, 12, 3)) as d:
        on_device(chk, d)
    assert _capi.lib().rh_compile_count() == compiles
    chk.close()


# ---- 3. what is refused -------------------------------------------------------------------------------------------------------------------
def test_device_invalid_arguments():
    x = base_buffer(8, 3, 50, 1)
    chk = check_of(SIX, 8)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=47, count=4), dict(first=-1, count=5), dict(count=0), dict(thin=0)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(chk, d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        with pytest.raises(R.RainierHipError) as e:
            R.ppc_device(chk, d.ptr.value, 3, 50, 7, device=0)
        assert e.value.code == _capi.RH_E_INVALID and "the check reads 8" in str(e.value)
        assert on_device(chk, d, first=49, count=1).t_rep.shape == (3, 1, 6)
    chk.close()


def test_a_check_on_another_device_is_refused():
    if _capi.lib().rh_device_count() < 2:
        pytest.skip("one device visible")
    x = base_buffer(8, 3, 50, 1)
    chk = R.Check([R.ppc.mean()], 8, device=1)
    with DeviceDraws(x) as d:
        with pytest.raises(R.RainierHipError) as e:
            R.ppc_device(chk, d.ptr.value, 3, 50, 8, device=0)
        assert e.value.code == _capi.RH_E_INVALID and "different devices" in str(e.value)
        other = C.c_void_p()
        assert hip().hipSetDevice(1) == 0 and hip().hipMalloc(C.byref(other), x.nbytes) == 0
        try:
            assert hip().hipSetDevice(0) == 0
            here = R.Check([R.ppc.mean()], 8, device=0)
            with pytest.raises(R.RainierHipError) as e:
                R.ppc_device(here, other.value, 3, 50, 8, device=0)
            assert e.value.code == _capi.RH_E_INVALID and "different devices" in str(e.value)
            here.close()
        finally:
            hip().hipSetDevice(1); hip().hipFree(other); hip().hipSetDevice(0)
    chk.close()
