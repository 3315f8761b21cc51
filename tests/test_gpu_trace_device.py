"""Trace.diagnostics on the device (rh_sampler_diagnostics / rh_diagnostics_device, csrc/device/rh_trace.hip.h) on an MI355X:
the CPU tier's fixtures through the kernels -- the oracle's figures at the oracle-vs-numpy bars, and the very bits of the host
emulation of the device text --, a sampler's own draws (small model, big mode, a half-finished run), windows, repeatability, and
the gathered buffer of a communicator.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from rainier_amd import distributed as D
from tests import oracle_lib as O
from tests.test_trace_device_cpu import (NVARS, SHAPES, ar1_fixture, check_against_oracle, close, emulate, fixture_seed, special_cases,
                                         RHAT_REL, ESS_REL)

pytestmark = pytest.mark.gpu

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


class DeviceDraws:
    """a host array [chains][iterations][nvars] copied to device 0"""

    def __init__(self, x):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.ptr = C.c_void_p()
        assert hip().hipSetDevice(0) == 0
        assert hip().hipMalloc(C.byref(self.ptr), self.x.nbytes) == 0
        assert hip().hipMemcpy(self.ptr, self.x.ctypes.data_as(C.c_void_p), self.x.nbytes, 1) == 0     # hipMemcpyHostToDevice

    def diagnostics(self, first=0, count=None):
        m, n, k = self.x.shape
        diag, mean, var = R.diagnostics_device(self.ptr.value, m, n, k, device=0, first=first, count=count, moments=True)
        return np.array([r for r, _ in diag]), np.array([e for _, e in diag]), mean, var

    def free(self):
        if self.ptr:
            hip().hipFree(self.ptr); self.ptr = C.c_void_p()

    def __enter__(self): return self
    def __exit__(self, *a): self.free()


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. synthetic draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SHAPES)
def test_device_matches_the_oracle_and_the_host_emulation_bit_for_bit(m, n):
    for k in NVARS:
        x = ar1_fixture(m, n, k, fixture_seed(m, n, k))
        with DeviceDraws(x) as d:
            got = d.diagnostics()
        check_against_oracle(x, got[0], got[1], (m, n, k))
        assert same_bits(got, emulate(x)), (m, n, k)


def test_device_special_cases_and_windows():
    for name, x in special_cases():
        with DeviceDraws(x) as d:
            got = d.diagnostics()
        check_against_oracle(x, got[0], got[1], name)
        assert same_bits(got, emulate(x)), name
    x = ar1_fixture(4, 700, 20, 5)
    with DeviceDraws(x) as d:
        for first, count in ((1, 699), (37, 2), (100, 101), (250, 450), (0, 600)):
            got = d.diagnostics(first, count)
            rows = x[:, first:first + count, :].copy()
            check_against_oracle(rows, got[0], got[1], ("window", first, count))
            with DeviceDraws(rows) as own:                    # a window equals its copy, bit for bit
                assert same_bits(got, own.diagnostics()), (first, count)
            assert same_bits(got, d.diagnostics(first, count))   # and a second call gives the same bits
        for first, count in ((0, 701), (699, 2), (5, 1)):
            with pytest.raises(R.RainierHipError) as e:
                d.diagnostics(first, count)
            assert e.value.code == _capi.RH_E_INVALID
    with DeviceDraws(x[:1]) as d:
        with pytest.raises(R.RainierHipError, match="requirement failed: diagnostics requires multiple chains"):
            d.diagnostics()


def test_device_large_shape_against_the_host_on_sampled_columns():
    """1024 chains x 400 iterations x 2048 parameters (6.7 GB: 13 chunks of the bounded workspace, full tiles, lanes along p)
    against the host entry point on 64 sampled columns"""
    m, n, k = 1024, 400, 2048
    rng = np.random.default_rng(11)
    x = np.empty((m, n, k))
    x[:, 0, :] = rng.standard_normal((m, k))
    phi = np.linspace(0.0, 0.95, k)
    for i in range(1, n):
        x[:, i, :] = phi * x[:, i - 1, :] + rng.standard_normal((m, k))
    with DeviceDraws(x) as d:
        rhat, ess, mean, var = d.diagnostics()
    cols = np.sort(rng.choice(k, 64, replace=False))
    want = R.diagnostics(x[:, :, cols])
    for j, p in enumerate(cols):
        assert close(rhat[p], want[j][0], RHAT_REL) and close(ess[p], want[j][1], ESS_REL), (p, rhat[p], ess[p], want[j])
    np.testing.assert_allclose(mean[cols], x[:, :, cols].mean(axis=(0, 1)), rtol=0, atol=1e-12)
    assert np.all(np.isfinite(rhat)) and np.all(np.isfinite(ess)) and np.all(ess > 0)


# ---- 2. a sampler's own draws -------------------------------------------------------------------------------------------------------------
def _against_host(s, diag, mean, var, first, count):
    x = s.draws(first, count)
    want = R.diagnostics(x)
    for p, ((r, e), (wr, we)) in enumerate(zip(diag, want)):
        assert close(r, wr, RHAT_REL) and close(e, we, ESS_REL), (p, r, e, wr, we)
    m, n, _ = x.shape
    np.testing.assert_allclose(mean, x.mean(axis=(0, 1)), rtol=1e-12, atol=1e-13)
    w = x.var(axis=1, ddof=1).mean(axis=0)
    v = (n - 1) / n * w + x.mean(axis=1).var(axis=0, ddof=1)          # Trace.scala:85
    np.testing.assert_allclose(var, v, rtol=1e-10)


def test_sampler_diagnostics_eight_schools_and_a_half_finished_run():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 100)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    seeds = list(range(300, 364))
    s = R.Sampler(m, cfg, seeds)
    s.warmup(); s.run(100)
    compiles = _capi.lib().rh_compile_count()
    diag, mean, var = s.diagnostics(moments=True)          # the default window: the completed half
    _against_host(s, diag, mean, var, 0, 100)
    assert s.diagnostics() == diag and s.diagnostics(0, 100) == diag
    for first, count in ((0, 101), (50, 51), (0, 200), (0, 1), (-1, 10)):
        with pytest.raises(R.RainierHipError) as e:
            s.diagnostics(first, count)
        assert e.value.code == _capi.RH_E_INVALID
    half = s.draws(0, 100)
    s.run(100)
    assert np.array_equal(s.draws(0, 100), half)
    diag, mean, var = s.diagnostics(moments=True)
    _against_host(s, diag, mean, var, 0, 200)
    for (r, e) in diag:                                    # per-chain oracle on the way: the figures are Trace.diagnostics'
        assert np.isfinite(r) and e > 0
    x = s.draws()
    check_against_oracle(x, [r for r, _ in diag], [e for _, e in diag], "eight schools")
    w = s.diagnostics(37, 120, moments=True)
    _against_host(s, *w, 37, 120)
    assert _capi.lib().rh_compile_count() == compiles      # the trace kernels came from the kernel cache build() filled
    # the chains are the uninterrupted run's: a diagnostics call in between changes nothing
    s2 = R.Sampler(m, cfg, seeds)
    s2.warmup(); s2.run(200)
    assert np.array_equal(s2.draws(), x)
    s.close(); s2.close(); m.close()


def test_sampler_diagnostics_big_mode_all_parameters():
    """704 parameters (big mode: the chain vectors live in HBM), tick engine, HMC(8), 256 chains: every parameter against the host"""
    spec = models.hier_negbin(700, 100, seed=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True)
    assert "#define RH_BIGN 1" in m.hip_source and spec.n_params > 512
    cfg = R.make_config(40, 20, R.HMCSampler(8), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK)
    s = R.Sampler(m, cfg, [5000 + c for c in range(256)])
    s.warmup(); s.run(40)
    diag, mean, var = s.diagnostics(moments=True)
    assert len(diag) == spec.n_params
    _against_host(s, diag, mean, var, 0, 40)
    t = s.timing()
    assert "trace" not in t["dominant_kernel"]
    s.close(); m.close()


# ---- 3. next to the other calls over device-resident draws --------------------------------------------------------------------------------
def test_diagnostics_summary_and_predict_interleaved_on_one_device():
    """The trace and the summary kernels come out of one per-device module cache (csrc/draws.cpp), first use and repeat use
    interleaved: diagnostics, summary and predict (thin 3) of a sampler's draws, diagnostics and summary of the predictor's device
    buffer, diagnostics again -- each the host emulation's bits, the last the first's.  Funnel(10), strict math, 2 chains,
    HMC 50 + 20, L = 5."""
    from tests import test_predict_device_cpu as P
    from tests import test_summary_device_cpu as S

    def bits(got):
        diag, mean, var = got
        return np.array([r for r, _ in diag]), np.array([e for _, e in diag]), mean, var

    def same_summary(a, b):
        return all(S.same_bits(u, v) for u, v in zip(tuple(a)[:4], tuple(b)[:4]))
    rir, nreq = models.funnel_predict(10)
    m = R.Model(models.funnel(10), device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.HMC(50, 20, 5)
    cfg.massMatrixTuner = lambda: R.IdentityMassMatrixTuner()
    s = R.Sampler(m, cfg, [123, 124])
    s.warmup(); s.run(20)
    x = s.draws()
    d_first = bits(s.diagnostics(moments=True))
    assert same_bits(d_first, emulate(x))
    assert same_summary(s.summary(), S.emulate(x))
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    values = s.predict(p, thin=3)
    assert values.shape == (2, 7, nreq) and np.array_equal(values, P.emulate("funnel", x, thin=3))
    ptr = s.predict(p, thin=3, to_host=False)
    assert same_bits(bits(R.diagnostics_device(ptr, 2, 7, nreq, device=0, moments=True)), emulate(values))
    assert same_summary(R.summary_device(ptr, 2, 7, nreq, device=0), S.emulate(values))
    d_last = bits(s.diagnostics(moments=True))
    assert same_bits(d_last, emulate(x)) and same_bits(d_last, d_first)
    p.close(); s.close(); m.close()


# ---- 4. the gathered buffer ---------------------------------------------------------------------------------------------------------------
def test_comm_diagnostics_world_size_one_equals_the_samplers():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(60, 60), D.shard_seeds(900, 8, 0))
    s.warmup(); s.run(60)
    comm = D.Comm(D.Comm.unique_id(), 1, 0, 0)
    own = s.diagnostics(moments=True)
    got = comm.diagnostics(s, moments=True)
    assert got[0] == own[0] and np.array_equal(got[1], own[1]) and np.array_equal(got[2], own[2])
    assert comm.diagnostics(s, first=10, count=30) == s.diagnostics(10, 30)
    comm.close(); s.close(); m.close()
