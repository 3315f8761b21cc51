"""Trace.predict / Trace.thin over device-resident draws (rh_predict_*, rh_sampler_predict, csrc/device/rh_predict.hip.h) on an
MI355X: the CPU tier's shapes, windows and three programs through the kernels -- the oracle's bits and the host emulation's in
strict math, rh_requirements_eval's bits in fast math --, a sampler's own draws (a half-finished run, big mode), the diagnostics of
a prediction, a Lookup that leaves its table, and the gathered buffer of a communicator.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from rainier_amd import distributed as D
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_predict_device_cpu import SHAPES, emulate, kept_rows, oracle_rows, programs, synthetic_draws, windows
from tests.test_trace_device_cpu import ESS_REL, RHAT_REL, close

pytestmark = pytest.mark.gpu

_predictors = {}


def predictor(name, mode, fp_contract=False):
    """one handle per (program, options) for the whole module: compiled once, as a caller would keep it"""
    key = (name, mode, fp_contract)
    if key not in _predictors:
        _predictors[key] = R.Predictor(programs()[name][0], device=0, math_mode=mode, fp_contract=fp_contract)
    return _predictors[key]


def on_device(p, d, first=0, count=None, thin=1, **kw):
    m, n, k = d.x.shape
    return R.predict_device(p, d.ptr.value, m, n, k, device=0, first=first, count=count, thin=thin, **kw)


# ---- 1. synthetic draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,n", SHAPES)
@pytest.mark.parametrize("name", ["funnel", "sparse", "dense"])
def test_device_matches_the_oracle_the_emulation_and_requirements_eval(name, chains, n):
    rir, nreq, nvars = programs()[name][:3]
    strict, fast = predictor(name, _capi.MATH_STRICT), predictor(name, _capi.MATH_FAST)
    assert (strict.nreq, strict.nvars) == (nreq, nvars)
    x = synthetic_draws(chains, n, nvars)
    with DeviceDraws(x) as d:
        for first, count, thin in windows(n):
            rows = np.ascontiguousarray(kept_rows(x, first, count, thin))
            want = oracle_rows(name, rows)
            got = on_device(strict, d, first, count, thin)
            assert got.shape == want.shape and np.array_equal(got, want), (name, chains, n, first, count, thin)
            assert np.array_equal(got, emulate(name, x, first, count, thin))
            got = on_device(fast, d, first, count, thin)
            assert np.array_equal(got, R.predict(rir, rows, nreq, device=0)), (name, chains, n, first, count, thin)
            np.testing.assert_allclose(got, want, rtol=4e-16)


def test_device_fp_contract_and_invalid_windows():
    rir, nreq, nvars = programs()["funnel"][:3]
    x = synthetic_draws(3, 300, nvars)
    with DeviceDraws(x) as d:
        p = predictor("funnel", _capi.MATH_FAST, True)          # contraction allowed: no bit claim, the 1e-15 bar
        for first, count, thin in ((0, 300, 1), (3, 290, 4)):
            np.testing.assert_allclose(on_device(p, d, first, count, thin), oracle_rows("funnel", kept_rows(x, first, count, thin)), rtol=1e-15)
        p = predictor("funnel", _capi.MATH_STRICT)
        for first, count, thin in ((0, 301, 1), (299, 2, 1), (-1, 5, 1), (0, 0, 1), (0, 10, 0), (0, 10, -2), (300, 1, 1)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(p, d, first, count, thin)
            assert e.value.code == _capi.RH_E_INVALID, (first, count, thin)
        with pytest.raises(R.RainierHipError) as e:             # another nvars than the program's
            R.predict_device(p, d.ptr.value, 3, 300, nvars - 1, device=0)
        assert e.value.code == _capi.RH_E_INVALID
        # the device pointer is the handle's own buffer, reused while it is large enough
        a = on_device(p, d, 0, 300, 1, to_host=False)
        assert on_device(p, d, 0, 100, 2, to_host=False) == a
    with pytest.raises(R.RainierHipError) as e:
        R.Predictor(models.funnel(10).rir, device=0)
    assert e.value.code == _capi.RH_E_INVALID and "header kind" in str(e.value)


# ---- 2. a sampler's own draws -------------------------------------------------------------------------------------------------------------
def test_sampler_predict_eight_schools_and_a_half_finished_run():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 100)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    seeds = list(range(300, 364))
    s = R.Sampler(m, cfg, seeds)
    s.warmup(); s.run(100)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    want = R.predict(rir, s.draws(0, 100), nreq, device=0, math_mode=_capi.MATH_STRICT)
    compiles = _capi.lib().rh_compile_count()              # (both programs are built by now; nothing below may compile)
    got = s.predict(p)                                     # the default window: the completed half
    assert got.shape == (64, 100, nreq) and np.array_equal(got, want)
    for first, count, thin in ((0, 100, 1), (0, 100, 3), (7, 90, 4), (99, 1, 1), (0, 100, 101)):
        got = s.predict(p, first, count, thin)
        want = R.predict(rir, s.draws(first, count)[:, ::thin], nreq, device=0, math_mode=_capi.MATH_STRICT)
        assert got.shape == want.shape and np.array_equal(got, want), (first, count, thin)
        assert np.array_equal(s.predict(p, first, count, thin), got)          # a second call gives the same bits
    assert _capi.lib().rh_compile_count() == compiles                          # repeated calls compile nothing
    for first, count, thin in ((0, 101, 1), (50, 51, 1), (0, 200, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.predict(p, first, count, thin)
        assert e.value.code == _capi.RH_E_INVALID
    other = R.Predictor(programs()["sparse"][0], device=0)                     # another model's nVars
    with pytest.raises(R.RainierHipError) as e:
        s.predict(other)
    assert e.value.code == _capi.RH_E_INVALID
    other.close()
    assert "predict" not in s.timing()["dominant_kernel"]
    # the chains are the uninterrupted run's: predicting in between changes nothing
    half = s.draws(0, 100)
    s.run(100)
    x = s.draws()
    assert np.array_equal(x[:, :100], half)
    s2 = R.Sampler(m, cfg, seeds)
    s2.warmup(); s2.run(200)
    assert np.array_equal(s2.draws(), x)
    assert np.array_equal(s.predict(p, thin=2), R.predict(rir, x[:, ::2], nreq, device=0, math_mode=_capi.MATH_STRICT))
    assert "predict" not in s.timing()["dominant_kernel"]
    p.close(); s.close(); s2.close(); m.close()


# ---- 3. big mode ----------------------------------------------------------------------------------------------------------------------------
def test_sampler_predict_big_mode_sparse_and_dense():
    """704 parameters (big mode: the chain vectors live in HBM), tick engine, HMC(8), 256 chains: 4 of the parameters through the
    gathered staging, all of them through the direct kernel, against rh_requirements_eval on the host copy"""
    spec = models.hier_negbin(700, 100, seed=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True)
    assert spec.n_params == 704
    cfg = R.make_config(40, 20, R.HMCSampler(8), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK)
    s = R.Sampler(m, cfg, [5000 + c for c in range(256)])
    s.warmup(); s.run(40)
    x = s.draws()
    for name in ("sparse", "dense"):
        rir, nreq = programs()[name][:2]
        p = predictor(name, _capi.MATH_FAST)
        for first, count, thin in ((0, 40, 1), (3, 30, 4)):
            got = s.predict(p, first, count, thin)
            assert np.array_equal(got, R.predict(rir, x[:, first:first + count:thin], nreq, device=0)), (name, first, count, thin)
    assert "predict" not in s.timing()["dominant_kernel"]
    s.close(); m.close()


# ---- 4. the diagnostics of a prediction ----------------------------------------------------------------------------------------------------
def test_diagnostics_of_predictions():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values, diag, mean, var = s.predict(p, first, count, thin, diagnostics=True)
        kept = values.shape[1]
        ptr = s.predict(p, first, count, thin, to_host=False)
        d2, m2, v2 = R.diagnostics_device(ptr, 16, kept, nreq, device=0, moments=True)
        assert d2 == diag and np.array_equal(m2, mean) and np.array_equal(v2, var)
        for (r, e), (wr, we) in zip(diag, R.diagnostics(values)):
            assert close(r, wr, RHAT_REL) and close(e, we, ESS_REL), (r, e, wr, we)
        np.testing.assert_allclose(mean, values.mean(axis=(0, 1)), rtol=1e-12, atol=1e-13)
    p.close(); s.close(); m.close()


# ---- 5. a Lookup that leaves its table -------------------------------------------------------------------------------------------------------
def test_lookup_out_of_range_is_reported():
    rir, nreq = models.lookup_predict(4)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    x = np.zeros((2, 70, 4))
    x[..., 1:] = np.arange(1.0, 4.0)
    x[..., 0] = 0.6                                       # index (int)(1.2) = 1 -> the second entry, parameter 2
    with DeviceDraws(x) as d:
        assert np.array_equal(on_device(p, d), np.full((2, 70, 1), 2.0))
        assert np.array_equal(on_device(p, d), R.predict(rir, x, nreq, device=0, math_mode=_capi.MATH_STRICT))
    x[1, 69, 0] = 1.7                                     # one draw of the last wavefront's ragged tail: index 3 of a table of 3
    with DeviceDraws(x) as d:
        with pytest.raises(R.RainierHipError) as e:
            on_device(p, d)
        assert e.value.code == _capi.RH_E_LOOKUP
        assert np.array_equal(on_device(p, d, 0, 69, 1), np.full((2, 69, 1), 2.0))          # the window without it is fine again
    p.close()


# ---- 6. the gathered buffer ------------------------------------------------------------------------------------------------------------------
def test_comm_predict_world_size_one_equals_the_samplers():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(60, 60), D.shard_seeds(900, 8, 0))
    s.warmup(); s.run(60)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    comm = D.Comm(D.Comm.unique_id(), 1, 0, 0)
    assert np.array_equal(comm.predict(s, p), s.predict(p))
    assert np.array_equal(comm.predict(s, p, first=10, count=30, thin=4), s.predict(p, 10, 30, 4))
    ptr = comm.allgather_draws(s, to_host=False)
    assert np.array_equal(comm.predict(ptr, p, chains=8, iterations=60, nvars=10, thin=2), s.predict(p, thin=2))
    comm.close(); p.close(); s.close(); m.close()
