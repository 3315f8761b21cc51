"""Posterior summaries on the device (rh_sampler_summary / rh_summary_device, csrc/device/rh_summary.hip.h) on an MI355X: the CPU
tier's fixtures through the kernels -- numpy's order statistics and hdpi bit for bit, the host emulation's bits for mean and sd --,
a buffer that crosses the workspace cap, a sampler's own draws (small model, big mode, a thinned window), a predictor's device
buffer, and the gathered buffer of a communicator.

Synthetic draws are uploaded with a ctypes handle on the HIP runtime (no torch in a test process: it would swap the compiler
under hiprtc, tests/test_capi_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from rainier_amd import distributed as D
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_summary_device_cpu import (HDPI, NCASES, NKINDS, PROBS, Reference, check_against_reference, emulate, fixture, n_cases,
                                           same_bits, tile, window)

pytestmark = pytest.mark.gpu


def on_device(d, first=0, count=None, thin=1, probs=PROBS, hdpi=HDPI):
    m, n, k = d.x.shape
    return R.summary_device(d.ptr.value, m, n, k, device=0, first=first, count=count, thin=thin, probs=probs, hdpi=hdpi)


def same_summary(a, b):
    return all((u is None and v is None) or same_bits(u, v) for u, v in zip(tuple(a)[:4], tuple(b)[:4]))


# ---- 1. synthetic draws --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(NCASES))
@pytest.mark.parametrize("thin", [1, 3])
def test_device_matches_numpy_and_the_host_emulation_bit_for_bit(case, thin):
    chains, kept = n_cases()[case]
    first, count, iters = window(kept, thin)
    for nvars, off in [(1, off) for off in range(NKINDS)] + [(5, 0), (5, 5), (65, 0)]:
        x = fixture(chains, iters, nvars, 100 * case + 10 * nvars + off + thin, off)
        with DeviceDraws(x) as d:
            got = on_device(d, first, count, thin)
        check_against_reference(got, Reference(x, first, count, thin), (case, thin, nvars, off))
        assert same_summary(got, emulate(x, first, count, thin)), (case, thin, nvars, off)


def test_device_probability_edges_and_invalid_arguments():
    T = tile()
    probs16 = tuple(np.linspace(0.0, 1.0, 16))
    n = 64
    near_one = float(np.nextafter((n - 1) / n, 1.0))
    for chains, iters, probs, hdpis in ((1, 1, (0.0, 1.0, 0.055), (0.89, 1.0, 1e-300)), (3, 21, probs16, (1.0, None)), (1, T + 1, probs16, (1.0,)),
                                        (1, n, PROBS, (near_one, (n - 1) / n)), (1, 100, PROBS, (0.55,))):
        x = fixture(chains, iters, NKINDS, 17)
        with DeviceDraws(x) as d:
            for hd in hdpis:
                got = on_device(d, probs=probs, hdpi=hd)
                check_against_reference(got, Reference(x, probs=probs, hdpi=hd), (chains, iters, hd))
                assert same_summary(got, emulate(x, probs=probs, hdpi=hd)) and (got.hdpi is None) == (hd is None)
    x = fixture(3, 50, 5, 1)
    with DeviceDraws(x) as d:
        for kw in (dict(first=0, count=51), dict(first=49, count=2), dict(first=-1, count=5), dict(count=0), dict(thin=0), dict(first=50, count=1),
                   dict(probs=()), dict(probs=tuple([0.5] * 17)), dict(probs=(0.5, 1.5)), dict(probs=(-0.1,)), dict(hdpi=1.5)):
            with pytest.raises(R.RainierHipError) as e:
                on_device(d, **kw)
            assert e.value.code == _capi.RH_E_INVALID, kw
        # one pooled column beyond the workspace cap (2 * N * 8 bytes > 128 MiB) is refused from its shape alone, before any launch:
        # the buffer is never read
        with pytest.raises(R.RainierHipError) as e:
            R.summary_device(d.ptr.value, 1024, 8193, 1, device=0)
        assert e.value.code == _capi.RH_E_UNSUPPORTED and "workspace" in str(e.value)


def test_device_two_chunks_all_columns_and_a_second_call():
    """4 chains x 5000 x 700 (112 MB of draws, N = 20 000): 320 KB of workspace per parameter, so the 128 MiB cap makes two chunks"""
    x = fixture(4, 5000, 700, 77)
    assert 2 * 20000 * 8 * 700 > (128 << 20)
    with DeviceDraws(x) as d:
        got = on_device(d)
        again = on_device(d)
        win = on_device(d, 11, 4000, 3)
    check_against_reference(got, Reference(x), "two chunks")
    assert same_summary(got, again)
    check_against_reference(win, Reference(x, 11, 4000, 3), "two chunks, a thinned window")


# ---- 2. a sampler's own draws --------------------------------------------------------------------------------------------------------
def test_sampler_summary_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    cfg = R.make_config(200, 200)                          # DefaultConfig's EHMC, dual averaging, windowed diagonal mass
    s = R.Sampler(m, cfg, list(range(300, 364)))
    s.warmup(); s.run(200)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    got = s.summary()
    assert got.quantiles.shape == (spec.n_params, 2) and got.hdpi.shape == (spec.n_params, 2)
    assert same_summary(got, R.summary_device(s.draws_device_ptr(), 64, 200, spec.n_params, device=0))
    check_against_reference(got, Reference(before), "eight schools")
    assert same_summary(got, emulate(before))
    assert np.all(got.quantiles[:, 0] < got.quantiles[:, 1]) and np.all(got.hdpi[:, 0] < got.hdpi[:, 1]) and np.all(got.sd > 0)
    # a thinned window equals the summary of a host copy of those rows, uploaded
    win = s.summary(7, 180, 3, probs=(0.25, 0.5, 0.75), hdpi=0.5)
    rows = np.ascontiguousarray(before[:, 7:187:3, :])
    with DeviceDraws(rows) as d:
        assert same_summary(win, R.summary_device(d.ptr.value, 64, rows.shape[1], spec.n_params, device=0, probs=(0.25, 0.5, 0.75), hdpi=0.5))
    check_against_reference(win, Reference(before, 7, 180, 3, (0.25, 0.5, 0.75), 0.5), "eight schools, thinned")
    # windows at thin = 1 that start late and end early, against numpy and against the device form on the same buffer
    for first, count in ((5, 150), (199, 1), (1, 199)):
        w1 = s.summary(first, count)
        check_against_reference(w1, Reference(before, first, count), ("eight schools, window", first, count))
        assert same_summary(w1, R.summary_device(s.draws_device_ptr(), 64, 200, spec.n_params, device=0, first=first, count=count))
    for first, count, thin in ((0, 201, 1), (150, 51, 1), (0, 0, 1), (-1, 10, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.summary(first, count, thin)
        assert e.value.code == _capi.RH_E_INVALID
    assert _capi.lib().rh_compile_count() == compiles      # the summary kernels came from the kernel cache build() filled
    assert "summary" not in s.timing()["dominant_kernel"]
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    print(R.format_precis(["p%d" % i for i in range(spec.n_params)], got))
    s.close(); m.close()


def test_sampler_summary_half_finished_run_uses_the_completed_iterations():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(100, 60), list(range(40, 48)))
    s.warmup(); s.run(40)
    half = s.draws(0, 40)
    check_against_reference(s.summary(), Reference(half), "the completed part")
    with pytest.raises(R.RainierHipError) as e:
        s.summary(0, 41)
    assert e.value.code == _capi.RH_E_INVALID
    s.run(60)
    assert np.array_equal(s.draws(0, 40), half)
    check_against_reference(s.summary(), Reference(s.draws()), "the whole run")
    s.close(); m.close()


def test_sampler_summary_big_mode_all_parameters():
    """704 parameters (big mode: the chain vectors live in HBM), tick engine, HMC(8), 256 chains: every parameter against numpy"""
    spec = models.hier_negbin(700, 100, seed=3)
    m = R.Model(spec, device=0, fp_contract=True, factor_outputs=True)
    assert "#define RH_BIGN 1" in m.hip_source and spec.n_params > 512
    cfg = R.make_config(40, 20, R.HMCSampler(8), R.DualAvgTuner(0.8), R.DiagonalMassMatrixTuner(8, 1.5, 4, 4), engine=_capi.ENGINE_TICK)
    s = R.Sampler(m, cfg, [5000 + c for c in range(256)])
    s.warmup(); s.run(40)
    x = s.draws()
    got = s.summary()
    assert len(got.mean) == spec.n_params
    check_against_reference(got, Reference(x), "big mode")
    check_against_reference(s.summary(3, 30, 4), Reference(x, 3, 30, 4), "big mode, thinned")
    check_against_reference(s.summary(2, 31), Reference(x, 2, 31), "big mode, a window at thin 1")
    assert "summary" not in s.timing()["dominant_kernel"] and np.array_equal(s.draws(), x)
    s.close(); m.close()


# ---- 3. a posterior-predictive interval without a copy -------------------------------------------------------------------------------
def test_summary_of_a_predictors_device_buffer():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(120, 100), list(range(700, 716)))
    s.warmup(); s.run(120)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    for first, count, thin in ((0, 120, 1), (10, 100, 3)):
        values = s.predict(p, first, count, thin)
        ptr = s.predict(p, first, count, thin, to_host=False)
        got = R.summary_device(ptr, 16, values.shape[1], nreq, device=0)
        check_against_reference(got, Reference(values), ("predictions", first, count, thin))
        assert same_summary(got, emulate(values))
    p.close(); s.close(); m.close()


# ---- 4. the gathered buffer ----------------------------------------------------------------------------------------------------------
def test_comm_summary_world_size_one_equals_the_samplers():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(60, 60), D.shard_seeds(900, 8, 0))
    s.warmup(); s.run(60)
    comm = D.Comm(D.Comm.unique_id(), 1, 0, 0)
    assert same_summary(comm.summary(s), s.summary())
    assert same_summary(comm.summary(s, first=10, count=30, thin=4, probs=(0.1, 0.9), hdpi=None), s.summary(10, 30, 4, (0.1, 0.9), None))
    comm.close(); s.close(); m.close()
