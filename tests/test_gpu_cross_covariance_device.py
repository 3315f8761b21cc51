"""Cross-covariance of two draw sets (csrc/device/rh_xcov.hip.h) on an MI355X: the CPU tier's shapes through the kernels, the square
covariance kernel's bits when both sides are one buffer, a sampler's draws against a predictor's requirements, Sampler.influence.
(The chunk loop of the tile pairs is reached on the device only at shapes of several GB: the emulation covers it.)"""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_covariance_device_cpu import pooled, same_bits, shuffled_with_duplicate
from tests.test_cross_covariance_device_cpu import KAS, KBS, LD, NS, check_bounds, emulate, same_results, two_fixtures

pytestmark = pytest.mark.gpu
FIGURES = lambda r: (r.mean_a, r.mean_b, r.var_a, r.var_b, r.cross, r.corr)


def on_device(da, db, **kw):
    m, n, na = da.x.shape
    return R.cross_covariance_device(da.ptr.value, db.ptr.value, m, n, na, db.x.shape[2], device=0, corr=True, **kw)


@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("ka", KAS)
@pytest.mark.parametrize("n", NS)
def test_device_within_the_derived_bound_and_against_the_host_emulation(n, ka, kb):
    for thin in (1, 3):
        a, b, first, count = two_fixtures(n, ka, kb, thin)
        at = dict(first=first, count=count, thin=thin)
        with DeviceDraws(a) as da, DeviceDraws(b) as db:
            got, again = on_device(da, db, **at), on_device(da, db, **at)
            ca, cb = shuffled_with_duplicate(ka, n + ka), shuffled_with_duplicate(ka, n + kb)
            own = on_device(da, da, cols_a=ca, cols_b=cb, **at)
            square = R.covariance_device(da.ptr.value, *a.shape, device=0, **at)
        check_bounds(pooled(a, first, count, thin), pooled(b, first, count, thin), FIGURES(got), (n, ka, kb, thin))
        assert same_results(FIGURES(got), emulate(a, b, **at)[0]), (n, ka, kb, thin, "the host emulation's bits")
        assert same_results(FIGURES(got), FIGURES(again)), (n, ka, kb, thin, "a second call")
        assert same_bits(own.cross, square.cov[np.ix_(ca, cb)]) and same_bits(own.var_a, np.diag(square.cov)[ca]) and same_bits(own.mean_b, square.mean[cb])


def test_sampler_cross_covariance_eight_schools():
    spec = models.eight_schools()
    rir, nreq = models.eight_schools_predict()
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(200, 200), list(range(300, 364)))
    s.warmup(); s.run(200)
    p = R.Predictor(rir, device=0, math_mode=_capi.MATH_STRICT)
    before = s.draws()
    compiles = _capi.lib().rh_compile_count()
    for first, count, thin in ((0, 200, 1), (7, 180, 3)):
        values = s.predict(p, first, count, thin)
        got = s.cross_covariance(p, first, count, thin, corr=True)
        assert got.cross.shape == (spec.n_params, nreq) and got.cols_b == tuple(range(nreq)) and got.cols_a == tuple(range(spec.n_params))
        check_bounds(pooled(before, first, count, thin), pooled(values), FIGURES(got), ("eight schools", thin))
        win = np.ascontiguousarray(before[:, first:first + count:thin, :])           # the device form on the two pointers: the same bits
        with DeviceDraws(win) as da:
            ptr = s.predict(p, first, count, thin, to_host=False)
            dev = R.cross_covariance_device(da.ptr.value, ptr, 64, win.shape[1], spec.n_params, nreq, device=0, corr=True)
        assert same_results(FIGURES(got), FIGURES(dev)), thin
        sub = s.cross_covariance(p, first, count, thin, cols=[3, 0], pred_cols=[7, 7, 1])
        assert sub.corr is None and same_bits(sub.cross, got.cross[np.ix_([3, 0], [7, 7, 1])])
    assert np.all(np.abs(got.corr) <= 1.0 + 1e-12) and _capi.lib().rh_compile_count() == compiles   # the kernel cache that build() filled served it
    assert np.array_equal(s.draws(), before)                                        # the chains are unaltered
    p.close(); s.close(); m.close()


def test_sampler_influence_linreg():
    n, k, rows = 300, 3, 20
    cols = models.linreg_data(n, k)
    m = R.Model(models.linreg(n=n, k=k), device=0)
    s = R.Sampler(m, R.make_config(50, 20, R.HMCSampler(3)), list(range(500, 564)))
    s.warmup(); s.run(50)
    p = R.Predictor(models.linreg_loglik(k, np.stack([c[:rows] for c in cols[1:]], axis=1), cols[0][:rows])[0], device=0)
    got, full = s.influence(p), s.cross_covariance(p, corr=True)
    check_bounds(pooled(s.draws()), pooled(s.predict(p)), FIGURES(full), "linreg")                # influence against np.longdouble
    assert same_bits(got.influence, full.cross) and same_bits(got.post_sd, np.sqrt(full.var_a)) and got.influence.shape == (2 + k, rows)
    assert got.cols == full.cols_a == tuple(range(2 + k)) and got.ll_cols == tuple(range(rows))
    # ij_cov by the same formula in longdouble from that influence: the row means enter in second order, as in the CPU tier's bound
    i = got.influence.astype(LD)
    d, e = i - i.mean(axis=1, keepdims=True), LD((rows + 2) * 2.0 ** -53) * np.abs(i).mean(axis=1)
    bound = LD((rows + 4) * 2.0 ** -53) * (np.abs(d) @ np.abs(d).T) + LD(rows) * e[:, None] * e[None, :]
    assert np.all(np.abs(got.ij_cov.astype(LD) - d @ d.T) <= bound) and same_bits(got.ij_se, np.sqrt(np.diag(got.ij_cov)))
    p.close(); s.close(); m.close()
