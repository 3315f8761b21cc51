"""The count families and the composites of posterior-predictive sampling on an MI355X (rh_generate_ext_kernel,
csrc/device/rh_generate_ext.hip.h): the CPU tier's fixtures through the kernel -- the oracle's bits and the host emulation's bits,
every branch of Binomial and NegativeBinomial, Categorical, BetaBinomial, the mixtures, the slab boundary with its hidden op, carry
and guarded run --, shape and chain0 independence, a sampler's own draws through a predictor into a zero-inflated Poisson and a
binomial with the predictive check over them, an old table next to it, and the domain and cap fixtures (bounded by construction: at
most 4096 iterations, nothing drawn), of which only the NaN positions and the flags are compared."""
import math

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, gen, models
from tests.test_generate_device_cpu import FEW_OPS, SEED
from tests.test_generate_device_cpu import NIN as OLD_NIN, emulate as emulate_old, inputs as old_inputs
from tests.test_generate_families_cpu import (BAD, BRANCHES, FEW, MIX3, NIN, SHAPES, TABLES, W3, WIDE, bits, emulate, flat_ops, inputs, oracle, reference,
                                              same_bits, visible)
from tests.test_gpu_trace_device import DeviceDraws

pytestmark = pytest.mark.gpu
F_DOMAIN, F_CAP = _capi.GEN_F_DOMAIN, _capi.GEN_F_CAP

_generators = {}


def generator(name):
    if name not in _generators:
        _generators[name] = R.Generator(TABLES[name], nin=NIN, device=0)
    return _generators[name]


def on_device(g, d, seed, chain0=0):
    chains, kept, nin = d.x.shape
    return R.generate_device(g, d.ptr.value, chains, kept, nin, seed, chain0=chain0, device=0)


def run(ops, x, seed, chain0=0):
    """a table over x on the device -> (samples, flags)"""
    g = R.Generator(ops, nin=x.shape[2], device=0)
    with DeviceDraws(x) as d:
        got = on_device(g, d, seed, chain0)
    flags = g.flags
    g.close()
    return got, flags


# ---- 1. the CPU tier's in-domain fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,kept", SHAPES)
def test_device_has_the_oracles_and_the_host_emulations_bits(chains, kept):
    for name in TABLES:
        x, want, _, _ = reference(chains, kept, name)
        g = generator(name)
        with DeviceDraws(x) as d:
            got = on_device(g, d, SEED)
        assert got.shape == (chains, kept, len(visible(flat_ops(TABLES[name])))) == (chains, kept, g.nout) and g.flags == 0
        assert same_bits(got, want), (chains, kept, name, np.argwhere(bits(got) != bits(want))[:4])
        assert same_bits(got, emulate(x, TABLES[name], SEED)[0]), (chains, kept, name)


def test_every_branch_and_the_composites_on_the_device():
    x = np.zeros((2, 60, 1))
    ops = [op for op, _ in BRANCHES]
    got, flags = run(ops, x, SEED + 2)
    assert flags == 0 and same_bits(got, oracle(x, ops, SEED + 2)[0]) and same_bits(got, emulate(x, ops, SEED + 2)[0])
    for m in (2, 3, 5):                                            # Categorical: weights that sum below 1, a zero weight
        w = np.random.default_rng(40 + m).dirichlet(np.ones(m), size=300)
        w[:100] *= 0.25
        w[100:200, 0] = 0.0
        cat = [gen.Categorical(0, m), gen.Uniform(0.0, 1.0)]
        got, flags = run(cat, w.reshape(3, 100, m), SEED + m)
        assert flags == 0 and same_bits(got, oracle(w.reshape(3, 100, m), cat, SEED + m)[0])


# ---- 2. shape, sharding, repeatability ------------------------------------------------------------------------------------------------
def test_device_results_do_not_depend_on_shape_or_sharding():
    g = R.Generator(WIDE, nin=NIN, device=0)
    x = inputs(3, 86, seed=5)
    with DeviceDraws(x) as d, DeviceDraws(x.reshape(1, 258, NIN)) as flat:
        whole = on_device(g, d, SEED)
        assert same_bits(whole.reshape(-1), on_device(g, flat, SEED).reshape(-1))
        assert same_bits(on_device(g, d, SEED), whole)                       # a second call on the same handle
        assert same_bits(whole, emulate(x, WIDE, SEED)[0]) and g.flags == 0
    g.close()
    g = R.Generator(FEW, nin=NIN, device=0)
    y = inputs(4, 86, seed=6)
    with DeviceDraws(y) as d, DeviceDraws(y[2:]) as shard:
        ran = on_device(g, d, SEED)
        assert same_bits(on_device(g, shard, SEED, chain0=2), ran[2:])       # chains 2..3, as another device would hold them
        assert same_bits(ran, emulate(y, FEW, SEED)[0]) and g.flags == 0
    g.close()


# ---- 3. end to end: a sampler's draws -> a predictor -> a zero-inflated Poisson and a binomial -> the check ---------------------------------
def test_sampler_generate_and_ppc_over_a_count_table():
    spec = models.linreg(n=3000, k=3)
    m = R.Model(spec, device=0)
    cfg = R.make_config(40, 20, R.HMCSampler(3), engine=_capi.ENGINE_TICK)
    s = R.Sampler(m, cfg, [11, 12, 13, 14, 15, 16])
    s.warmup(); s.run(40)
    old = R.Generator(FEW_OPS, nin=OLD_NIN, device=0)                        # an old-family generator in the same process, before ...
    ox = old_inputs(3, 86, seed=5)
    with DeviceDraws(ox) as d:
        old_bits = on_device(old, d, SEED)
    assert same_bits(old_bits, emulate_old(ox, FEW_OPS, SEED)[0])
    p = R.Predictor(models.linreg_counts_predict(3, [0.5, -1.0, 2.0]), device=0)   # (psi, 1 - psi, a rate) at a new x
    ops = [gen.ZeroInflated(0, gen.Poisson(gen.col(2))), gen.Binomial(gen.col(0), 40.0), gen.NegativeBinomial(gen.col(1), 6.0)]
    g = R.Generator(ops, nin=3)
    assert g.nout == 3
    pred = s.predict(p, thin=2)
    assert np.all((0 < pred[..., 0]) & (pred[..., 0] < 1)) and np.all(pred[..., 2] > 0)
    got = s.generate(p, g, SEED, thin=2)
    want, flags = oracle(pred, ops, SEED)
    assert got.shape == (6, 20, 3) and g.flags == 0 and flags == 0 and same_bits(got, want)
    assert same_bits(s.generate(p, g, SEED + 3, first=5, count=30, thin=4, chain0=7), oracle(s.predict(p, 5, 30, 4), ops, SEED + 3, chain0=7)[0])
    # the check reads the generator's VISIBLE columns
    chk = R.Check([R.ppc.mean(), R.ppc.max(), R.ppc.frac_le(0.0)], g.nout, segments=[[0], [1, 2]], device=0)
    y = np.array([0.0, 20.0, 5.0])
    res = s.ppc(p, g, chk, SEED, y=y)
    rep = s.generate(p, g, SEED)                                             # that call's replicated observations
    assert res.t_rep.shape == (6, 40, 6) and np.all(res.n_bad == 0)
    segs = [rep[..., [0]], rep[..., [1, 2]]]
    stats = (lambda v: v.mean(axis=-1), lambda v: v.max(axis=-1), lambda v: (v <= 0.0).mean(axis=-1))
    t = np.stack([f(v) for v in segs for f in stats], axis=-1)               # output g * nstat + k
    assert np.allclose(res.t_rep, t, rtol=1e-13, atol=0)                     # (max and the share exact; a mean of at most two values)
    assert np.array_equal(res.t_obs, [[0.0, 0.0, 1.0], [12.5, 20.0, 0.0]])   # [segment][statistic]
    assert np.array_equal(res.n_gt.reshape(-1), (res.t_rep > res.t_obs.reshape(-1)).sum(axis=(0, 1)))
    wide = R.Check([R.ppc.mean()], len(flat_ops(ops)), device=0)             # the table's 5 ops, hidden ones too: not its width
    with pytest.raises(R.RainierHipError) as e:
        s.ppc(p, g, wide, SEED)
    assert e.value.code == _capi.RH_E_INVALID and "the generator has 3 outputs" in str(e.value)
    with DeviceDraws(ox) as d:                                               # ... and after: its own earlier bits
        assert same_bits(on_device(old, d, SEED), old_bits)
    wide.close(); chk.close(); g.close(); p.close(); old.close(); s.close(); m.close()


# ---- 4. the domain and cap fixtures: NaN positions and flags ----------------------------------------------------------------------------
def test_domain_and_cap_fixtures_on_the_device():
    for what, bad in sorted(BAD.items()):
        guarded = {"binomial_p": gen.Binomial(gen.col(0), 20.0), "binomial_k": gen.Binomial(0.3, gen.col(0)), "negbin_p": gen.NegativeBinomial(gen.col(0), 5.0),
                   "negbin_n": gen.NegativeBinomial(0.3, gen.col(0)), "weight": gen.Categorical(0, 2)}[what]
        x = np.array([[v, 0.5] for v in bad] + [[0.5, 0.5]]).reshape(1, -1, 2)
        ops = [gen.Normal(0.0, 1.0), guarded, gen.Uniform(0.0, 1.0)]
        got, flags = run(ops, x, SEED)
        assert flags == F_DOMAIN and np.array_equal(np.isnan(got), np.isnan(oracle(x, ops, SEED)[0])), what
        assert np.all(np.isnan(got[0, :-1, 1])) and not np.isnan(got[0, -1, 1])
    x = np.zeros((1, 5, 1))
    for op in (gen.Binomial(1 - 5 / 8192, 8192.0), gen.NegativeBinomial(0.99, 8192.0)):
        got, flags = run([op, gen.Uniform(0.0, 1.0)], x, SEED)
        assert flags == F_CAP and np.all(np.isnan(got[..., 0])) and not np.any(np.isnan(got[..., 1]))
    y = inputs(1, 40, seed=8).copy()
    y[0, ::3, W3 + 1] = -1.0                                                 # a NaN selector: the mixture's column is NaN there
    got, flags = run([gen.Normal(0.0, 1.0), MIX3, gen.Uniform(0.0, 1.0)], y, SEED)
    assert flags == F_DOMAIN and np.all(np.isnan(got[0, ::3, 1])) and np.isnan(got).sum() == math.ceil(40 / 3)
