"""Multivariate ESS and MPSRF on the device (rh_sampler_joint_diagnostics / rh_joint_diagnostics_device, csrc/device/rh_joint.hip.h)
on an MI355X: the CPU tier's fixtures through the kernels -- the derived bounds against the np.longdouble reference, the bits of the
host emulation of the device text in mu and every matrix, a second call -- and a sampler's own draws."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, models
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_joint_device_cpu import CASES, KS, MATS, check, emulate, fixture, reference, same_bits

pytestmark = pytest.mark.gpu
FIGURES = ("mean", "ess_bm", "mess", "mpsrf") + MATS


def on_device(d, **kw):
    m, n, k = d.x.shape
    return R.joint_diagnostics_device(d.ptr.value, m, n, k, device=0, **kw)


def check_against_emulation(got, emu, what):
    """The emulation takes v_mfma_f64_16x16x4_f64 for a chain of fma over k = 0, 1, 2, 3, as the covariance kernels' does; the
    finish on the host is the same code.  So: the same bits, in every figure."""
    for q in FIGURES:
        assert same_bits(getattr(got, q), emu[q]), (what, q)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("chains,count", CASES)
def test_device_within_the_bounds_and_against_the_host_emulation(chains, count, k):
    x = fixture(chains, count, k)
    with DeviceDraws(x) as d:
        got, again = on_device(d), on_device(d)
    check(got, reference(x), (chains, count, k))
    check_against_emulation(got, emulate(x), (chains, count, k))
    check_against_emulation(again, got._asdict(), (chains, count, k, "a second call"))


def test_device_window_batch_and_column_list():
    x = fixture(3, 120, 65)
    cols = [int(c) for c in np.random.default_rng(65).permutation(65)[:43]]
    with DeviceDraws(x) as d:
        full, sub = on_device(d, first=7, count=100, batch=9), on_device(d, first=7, count=100, batch=9, cols=cols)
    check(full, reference(x, 7, 100, 9), "window")
    check(sub, reference(x, 7, 100, 9, cols), "cols")
    check_against_emulation(sub, emulate(x, 7, 100, 9, cols), "cols")
    assert sub.cols == tuple(cols) and (full.batch, full.batches, full.dropped) == (9, 11, 1)
    for q in MATS:
        assert same_bits(getattr(sub, q), getattr(full, q)[np.ix_(cols, cols)]), q


def test_device_repeated_out_of_order_column_list_in_every_family_that_takes_one():
    """cols = [2, 0, 2] over 4 chains x 32 iterations x 3 parameters through the six calls that take a column list (covariance,
    histogram, rank diagnostics, standard errors, joint diagnostics, WAIC / PSIS-LOO): entry k of every per-column result has the bits
    of the call that asks for column cols[k] alone -- in the matrices, entry (k, k)."""
    x = fixture(4, 32, 3)
    cols = [2, 0, 2]
    calls = {
        "covariance": (lambda c: R.covariance_device(d.ptr.value, 4, 32, 3, device=0, cols=c, corr=True), ("mean",), ("cov", "corr")),
        "histogram": (lambda c: R.histogram_device(d.ptr.value, 4, 32, 3, device=0, cols=c, bins=7), ("edges", "counts", "under", "over", "nan"), ()),
        "rank": (lambda c: R.rank_diagnostics_device(d.ptr.value, 4, 32, 3, device=0, cols=c), ("rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "truncated"), ()),
        "mcse": (lambda c: R.mcse_device(d.ptr.value, 4, 32, 3, device=0, cols=c, nlags=3),
                 ("mean", "sd", "ess_mean", "ess_sd", "mcse_mean", "mcse_sd", "quantile", "ess_quantile", "mcse_quantile", "acf", "truncated"), ()),
        "joint": (lambda c: on_device(d, cols=c), ("mean",), MATS),
        "loo": (lambda c: R.loo_device(d.ptr.value, 4, 32, 3, device=0, cols=c), ("lpd", "p_waic", "elpd_loo", "pareto_k", "tail_n"), ()),
    }
    with DeviceDraws(x) as d:
        for family, (call, per_column, matrices) in calls.items():
            got = call(cols)
            alone = {c: call([c]) for c in set(cols)}
            for k, c in enumerate(cols):
                for q in per_column:
                    assert same_bits(np.asarray(getattr(got, q))[k], np.asarray(getattr(alone[c], q))[0]), (family, q, k)
                for q in matrices:
                    assert same_bits(np.asarray(getattr(got, q))[k, k], np.asarray(getattr(alone[c], q))[0, 0]), (family, q, k)


def test_sampler_joint_diagnostics_linreg():
    spec = models.linreg(n=2000, k=3)
    m = R.Model(spec, device=0, math_mode=_capi.MATH_STRICT)
    s = R.Sampler(m, R.make_config(100, 100), list(range(300, 364)))
    s.warmup(); s.run(100)
    before = s.draws()
    got = s.joint_diagnostics()
    ref = reference(before)
    check(got, ref, "linreg")
    check_against_emulation(got, emulate(before), "linreg")
    assert (got.batch, got.batches, got.dropped) == (10, 10, 0) and got.within.shape == (spec.n_params,) * 2
    assert 0 < got.mess <= 64 * 100 * 4 and 1.0 <= got.mpsrf < 1.5
    check(s.joint_diagnostics(5, 90, cols=[4, 0, 2], batch=7), reference(before, 5, 90, 7, [4, 0, 2]), "linreg, window")
    assert np.array_equal(s.draws(), before)               # the chains are unaltered
    s.close(); m.close()
