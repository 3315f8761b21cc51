"""A linear map of the draws (csrc/device/rh_linear.hip.h) on an MI355X: the CPU tier's shapes and properties through the kernel, the
host emulation's bits, the map's device buffers handed to another *_device call, a sampler's draws, Sampler.mahalanobis."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_covariance_device_cpu import pooled, same_bits
from tests.test_linear_device_cpu import KS, MS, NS, case, check_bounds, check_properties, emulate

pytestmark = pytest.mark.gpu


def on_device(x, W, center=None, offset=None, cols=None, y=True, sqnorm=True, **at):
    """the CPU tier's run() on the device: (y or None, sqnorm or None) on the host"""
    with DeviceDraws(x) as d:
        lmap = R.LinearMap(W, center, offset, cols, device=0)
        r = R.linear_device(lmap, d.ptr.value, *d.x.shape, device=0, sqnorm=sqnorm if y else "only", **at)
        lmap.close()
    return r if y and sqnorm else (r, None) if y else (None, r)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_device_within_the_derived_bounds_invariant_and_the_host_emulation(n, k, m):
    for thin in (1, 3):
        x, lmap, at = case(n, k, m, thin)
        y, sq = check_properties(on_device, x, lmap, at, (n, k, m, thin))
        ey, esq = emulate(x, **lmap, **at)
        assert same_bits(y, ey) and same_bits(sq, esq), (n, k, m, thin, "the host emulation's bits")
        h = R.LinearMap(device=0, **lmap)                                   # to_host = False: the map's buffers as another call's draw set
        with DeviceDraws(x) as d, DeviceDraws(y) as uy, DeviceDraws(sq[:, :, None]) as us:
            py, psq = R.linear_device(h, d.ptr.value, *x.shape, device=0, to_host=False, sqnorm=True, **at)
            for got, want in ((R.covariance_device(py, *y.shape, device=0), R.covariance_device(uy.ptr.value, *y.shape, device=0)),
                              (R.covariance_device(psq, *sq.shape, 1, device=0), R.covariance_device(us.ptr.value, *sq.shape, 1, device=0))):
                assert same_bits(got.mean, want.mean) and same_bits(got.cov, want.cov), (n, k, m, thin, "the device buffers")
        h.close()


def test_sampler_linear_and_mahalanobis_eight_schools():
    spec = models.eight_schools()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(200, 200), list(range(300, 364)))
    s.warmup(); s.run(200)
    before, k = s.draws(), spec.n_params
    rng = np.random.default_rng(5)
    lmap = dict(W=rng.standard_normal((k, 70)), center=before.mean(axis=(0, 1)), offset=rng.standard_normal(70), cols=list(range(k)))
    h = R.LinearMap(device=0, **lmap)
    compiles = _capi.lib().rh_compile_count()
    for first, count, thin in ((0, 200, 1), (7, 180, 3)):
        y, sq = s.linear(h, first, count, thin, sqnorm=True)
        check_bounds(pooled(before, first, count, thin), lmap, y.reshape(-1, 70), sq.reshape(-1), ("eight schools", thin))
        assert same_bits(s.linear(h, first, count, thin), y)
        cov = s.covariance(first, count, thin)                              # the documented recipe, built here
        white = R.LinearMap(np.linalg.solve(np.linalg.cholesky(cov.cov), np.eye(k)).T, center=cov.mean, cols=cov.cols, device=0)
        got = s.mahalanobis(first, count, thin)
        assert same_bits(got.d2, s.linear(white, first, count, thin, sqnorm=True)[1]) and same_bits(got.cov, cov.cov) and got.cols == cov.cols
        white.close()
    assert _capi.lib().rh_compile_count() == compiles                       # the kernel cache that build() filled served them
    assert np.array_equal(s.draws(), before)                                # the chains are unaltered
    h.close(); s.close(); m.close()
