"""Kernel density estimates on the device (rh_kde_device / rh_kde_pairs_device, csrc/device/rh_kde.hip.h) on an MI355X: the CPU tier's
cases through the kernels against the same np.longdouble reference at the same derived tolerance (|got - ref| <= 1e-12 ref + 1e-300),
a second call, a window against its copy, a subset against the whole, and a sampler's own draws.  (No torch in a test process.)"""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_kde_device_cpu import CURVES, SURFACES, case, close, grid_of

pytestmark = pytest.mark.gpu


def curves(d, c, cols, first=None):
    first = c["first"] if first is None else first
    sel = range(d.x.shape[2]) if cols is None else cols
    return R.kde_device(d.ptr.value, *d.x.shape, device=0, first=first, count=c["count"], thin=c["thin"], cols=cols, points=c["points"],
                        bw=[c["bw"][k] for k in sel], range=[c["range"][k] for k in sel])


def surfaces(d, c, sel=None, first=None):
    first, sel = c["first"] if first is None else first, list(range(len(c["sel"]))) if sel is None else sel
    return R.kde_pairs_device(d.ptr.value, *d.x.shape, [c["sel"][p] for p in sel], device=0, first=first, count=c["count"], thin=c["thin"],
                              points=c["points"], bw=[c["bw"][p] for p in sel], range=[c["range"][p] for p in sel])


same = lambda a, b: np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", CURVES)
def test_curves_equal_the_longdouble_reference(name):
    c = case(name)
    with DeviceDraws(c["x"]) as d:
        got, again, sub = curves(d, c, None), curves(d, c, None), curves(d, c, c["sel"])
    with DeviceDraws(c["x"][:, c["first"]:c["first"] + c["count"], :]) as d:
        copy = curves(d, c, None, first=0)
    for k in c["ref"]:
        assert np.array_equal(got.grid[k], grid_of(*c["range"][k], c["points"])) and close(got.density[k], c["want"][k]), (name, k)
    assert same(again.density, got.density) and same(copy.density, got.density) and same(sub.density, got.density[c["sel"]])
    assert sub.cols == tuple(c["sel"]) and np.array_equal(sub.grid, got.grid[c["sel"]]) and np.array_equal(got.bw, c["bw"])


@pytest.mark.parametrize("name", SURFACES)
def test_surfaces_equal_the_longdouble_reference(name):
    c = case(name)
    npx, npy = c["points"]
    with DeviceDraws(c["x"]) as d:
        got, again, sub = surfaces(d, c), surfaces(d, c), surfaces(d, c, [len(c["sel"]) - 1, 0])
        turned = surfaces(d, dict(c, points=(npy, npx), sel=[c["sel"][0][::-1]], range=[c["range"][0][::-1]], bw=[c["bw"][0][::-1]]))
    with DeviceDraws(c["x"][:, c["first"]:c["first"] + c["count"], :]) as d:
        copy = surfaces(d, c, first=0)
    for p, (r, want) in enumerate(zip(c["range"], c["want"])):
        assert np.array_equal(got.xgrid[p], grid_of(*r[0], npx)) and np.array_equal(got.ygrid[p], grid_of(*r[1], npy)) and close(got.density[p], want), (name, p)
    assert same(again.density, got.density) and same(copy.density, got.density) and same(sub.density, got.density[[len(c["sel"]) - 1, 0]])
    assert close(turned.density[0], c["want"][0].T) and got.pairs == tuple(c["sel"])                # (b, a) on the turned grid: the transpose


def test_sampler_kde_equals_the_call_on_its_draws_pointer():
    spec = models.linreg(n=8, k=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(60, 50), list(range(40, 48)))
    s.warmup(); s.run(60)
    before, k, compiles = s.draws(), spec.n_params, _capi.lib().rh_compile_count()
    got, pair = s.kde(3, 50, thin=2, cols=[k - 1, 0], points=33), s.kde_pairs([(0, 1), (k - 1, 0)], 3, 50, points=(20, 70))
    assert _capi.lib().rh_compile_count() == compiles                                             # the code objects come from the kernel cache build() filled
    want = R.kde_device(s.draws_device_ptr(), 8, 60, k, device=0, first=3, count=50, thin=2, cols=[k - 1, 0], points=33)
    wpair = R.kde_pairs_device(s.draws_device_ptr(), 8, 60, k, [(0, 1), (k - 1, 0)], device=0, first=3, count=50, points=(20, 70))
    assert np.array_equal(got.density, want.density) and np.array_equal(got.grid, want.grid) and np.array_equal(got.bw, want.bw)
    assert np.array_equal(pair.density, wpair.density) and np.array_equal(pair.xgrid, wpair.xgrid) and np.array_equal(pair.bw, wpair.bw)
    assert got.density.shape == (2, 33) and pair.density.shape == (2, 20, 70) and np.isclose(got.grid[1, 0], before[:, 3:53:2, 0].min() - 3.0 * got.bw[1], rtol=1e-12)
    with pytest.raises(R.RainierHipError) as e:
        s.kde(points=1)
    assert e.value.code == _capi.RH_E_INVALID and np.array_equal(s.draws(), before)
    s.close(); m.close()
