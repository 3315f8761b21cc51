"""Posterior-predictive sampling on the device (rh_generate_device / rh_sampler_generate, csrc/device/rh_generate.hip.h) on an
MI355X: the CPU tier's fixtures through the kernel -- the oracle's bits and the host emulation's bits, every family, both branches
of Gamma and Poisson, every tile and slab boundary --, sharding by chain0, a sampler's own draws through a predictor end to end
with the summary of the samples taken where they lie, and the argument errors.  Every parameter is in its domain: the guards and
the iteration cap are exercised on the CPU only (tests/test_generate_device_cpu.py)."""
import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, gen, models
from tests.test_generate_device_cpu import FEW_OPS, NIN, NOUTS, SEED, SHAPES, bits, emulate, inputs, oracle, reference, same_bits, table
from tests.test_gpu_trace_device import DeviceDraws
from tests.test_summary_device_cpu import Reference, check_against_reference

pytestmark = pytest.mark.gpu

_generators = {}


def generator(nout):
    if nout not in _generators:
        _generators[nout] = R.Generator(table(nout), nin=NIN, device=0)
    return _generators[nout]


def on_device(g, d, seed, chain0=0, to_host=True):
    chains, kept, nin = d.x.shape
    return R.generate_device(g, d.ptr.value, chains, kept, nin, seed, chain0=chain0, device=0, to_host=to_host)


# ---- 1. synthetic parameter buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,kept", SHAPES)
def test_device_has_the_oracles_and_the_host_emulations_bits(chains, kept):
    for nout in NOUTS:
        x, want, _, _ = reference(chains, kept, nout)
        g = generator(nout)
        with DeviceDraws(x) as d:
            got = on_device(g, d, SEED)
        assert got.shape == (chains, kept, nout) and g.flags == 0
        assert same_bits(got, want), (chains, kept, nout, np.argwhere(bits(got) != bits(want))[:4])
        assert same_bits(got, emulate(x, table(nout), SEED)[0]), (chains, kept, nout)


# ---- 2. sharding, shape, repeatability ------------------------------------------------------------------------------------------------
def test_device_results_do_not_depend_on_shape_or_sharding():
    g = R.Generator(FEW_OPS, nin=NIN, device=0)
    x = inputs(3, 86, seed=5)
    with DeviceDraws(x) as d, DeviceDraws(x.reshape(1, 258, NIN)) as flat:
        whole = on_device(g, d, SEED)
        assert same_bits(whole.reshape(-1), on_device(g, flat, SEED).reshape(-1))
        assert same_bits(on_device(g, d, SEED), whole)                       # a second call on the same handle
        assert not np.any(bits(on_device(g, d, SEED + 1)[..., 0]) == bits(whole[..., 0]))
        assert same_bits(whole, emulate(x, FEW_OPS, SEED)[0])
    y = inputs(4, 86, seed=6)
    with DeviceDraws(y) as d, DeviceDraws(y[2:]) as shard:
        run = on_device(g, d, SEED)
        assert same_bits(on_device(g, shard, SEED, chain0=2), run[2:])       # chains 2..3, as another device would hold them
        assert g.flags == 0
    g.close()


# ---- 3. end to end: a sampler's draws -> a predictor -> the generator -> the summary ------------------------------------------------------
def test_sampler_generate_end_to_end_with_the_summary_of_the_samples():
    spec = models.linreg(n=3000, k=3)
    m = R.Model(spec, device=0)
    cfg = R.make_config(40, 20, R.HMCSampler(3), engine=_capi.ENGINE_TICK)
    s = R.Sampler(m, cfg, [11, 12, 13, 14, 15, 16])
    s.warmup(); s.run(40)
    p = R.Predictor(models.linreg_predict(3, [0.5, -1.0, 2.0]), device=0)   # (mu, sigma) at a new x
    ops = [gen.Normal(gen.col(0), gen.col(1))]                               # yhat ~ Normal(mu, sigma)
    g = R.Generator(ops, nin=2)
    pred = s.predict(p, thin=2)
    got = s.generate(p, g, SEED, thin=2)
    assert got.shape == (6, 20, 1) and g.flags == 0
    want, flags = oracle(pred, ops, SEED)
    assert flags == 0 and same_bits(got, want)
    assert same_bits(s.predict(p, thin=2), pred)                             # the predictions are the predictor's, untouched
    # a window, and a shard's chain0
    assert same_bits(s.generate(p, g, SEED + 3, first=5, count=30, thin=4, chain0=7), oracle(s.predict(p, 5, 30, 4), ops, SEED + 3, chain0=7)[0])
    # the samples where they lie: an 89 % predictive interval without a copy
    ptr = s.generate(p, g, SEED, thin=2, to_host=False)
    check_against_reference(R.summary_device(ptr, 6, 20, 1, device=0), Reference(want), "posterior-predictive samples")
    assert "generate" not in s.timing()["dominant_kernel"]
    # ---- invalid arguments
    with DeviceDraws(pred) as d:
        assert same_bits(R.generate_device(g, d.ptr.value, 6, 20, 2, SEED, device=0), want)   # the device form over a copy of the predictions
        with pytest.raises(R.RainierHipError) as e:
            R.generate_device(g, d.ptr.value, 6, 20, 3, SEED, device=0)       # another nin than the handle's
        assert e.value.code == _capi.RH_E_INVALID
    three = R.Generator([gen.Normal(gen.col(0), gen.col(2))], nin=3)
    with pytest.raises(R.RainierHipError) as e:
        s.generate(p, three, SEED)                                           # the predictor has 2 requirements
    assert e.value.code == _capi.RH_E_INVALID and "2 requirements" in str(e.value)
    for first, count, thin in ((0, 41, 1), (0, 0, 1), (0, 10, 0)):
        with pytest.raises(R.RainierHipError) as e:
            s.generate(p, g, SEED, first, count, thin)
        assert e.value.code == _capi.RH_E_INVALID
    three.close(); g.close(); p.close(); s.close(); m.close()
