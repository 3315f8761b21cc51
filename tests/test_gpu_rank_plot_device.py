"""Rank plots on the device (rh_sampler_rank_plot / rh_rank_plot_device, csrc/device/rh_rank_plot.hip.h) on an MI355X: the CPU tier's
cases through the kernels against the same numpy reference -- counts and nan equal, the derived figures against np.longdouble at
1e-13 relative --, a second call, a window against its copy, and a sampler's own draws.  (No torch in a test process:
tests/test_gpu_trace_device.py.)"""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_rank_plot_device_cpu import CASES, case, derived, plan

pytestmark = pytest.mark.gpu


def on_device(d, first, n, cols, bins):
    return R.rank_plot_device(d.ptr.value, *d.x.shape, device=0, first=first, count=n, cols=cols, bins=bins)


def close(got, want):
    """1e-13 relative to the figure (a figure that is 0 is 0); NaN matches NaN"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool(np.all(np.nan_to_num(np.abs(got - want)) <= 1e-13 * np.nan_to_num(np.abs(want))))


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_numpy_reference(name):
    c = case(name)
    x, first, n, cols, bins = c["x"], c["first"], c["n"], c["cols"], c["bins"]
    with DeviceDraws(x) as d:
        got, again = on_device(d, first, n, cols, bins), on_device(d, first, n, cols, bins)
    with DeviceDraws(x[:, first:first + n, :]) as d:
        copy = on_device(d, 0, n, cols, bins)
    assert np.array_equal(got.counts, c["ref"][0]) and np.array_equal(got.nan, c["ref"][1]), name
    assert np.array_equal(again.counts, got.counts) and np.array_equal(copy.counts, got.counts) and np.array_equal(copy.nan, got.nan)
    assert got.cols == tuple(cols if cols else range(x.shape[2])) and got.bins == bins and got.counts.dtype == np.int64
    gap, ks, chi2 = derived(c["ref"][0], c["ref"][1], n, np.longdouble)
    assert close(got.ecdf_gap, gap) and close(got.ks, ks) and close(got.chi2, chi2), name
    if name == "segments":
        assert plan(x.shape[0], n, x.shape[2], bins)["segs"] > 1
    if name == "values":
        assert got.ks[5, 0] == np.nanmax(got.ks) and np.all(np.isnan(got.chi2[4]))               # the shifted chain; the column with a NaN


def test_sampler_rank_plot_equals_the_call_on_its_draws_pointer():
    spec = models.linreg(n=8, k=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(60, 50), list(range(40, 48)))
    s.warmup(); s.run(60)
    before, k, compiles = s.draws(), spec.n_params, _capi.lib().rh_compile_count()
    got = s.rank_plot(3, 50, cols=[k - 1, 0], bins=10)                                            # the code object comes from the kernel cache build() filled
    assert _capi.lib().rh_compile_count() == compiles
    want = R.rank_plot_device(s.draws_device_ptr(), 8, 60, k, device=0, first=3, count=50, cols=[k - 1, 0], bins=10)
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.nan, want.nan) and np.array_equal(got.ks, want.ks)
    assert got.counts.shape == (2, 8, 10) and np.all(got.counts.sum(axis=2) == 50) and s.rank_plot().counts.shape == (k, 8, 20)
    with pytest.raises(R.RainierHipError) as e:
        s.rank_plot(bins=1)
    assert e.value.code == _capi.RH_E_INVALID and np.array_equal(s.draws(), before)
    s.close(); m.close()
