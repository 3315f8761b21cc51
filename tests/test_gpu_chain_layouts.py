"""rh_chain_kernel against the oracle, bit for bit, at every chain-state layout boundary (csrc/device/rh_engine.hip.h,
rh_prelude.hip.h): packed lane groups of 8 / 16 / 32, one chain per wavefront, one register slot up to its exact fit at 64, several
register slots; the dense mass matrix's per-lane rows up to its limit; the EHMC ring buffer's register and memory forms at their slot
boundaries; chains continued from a java.util.Random state with and without a pending gaussian.

A wrong lane mask or an off-by-one in any of these gives plausible draws, so every comparison is np.array_equal: the same
operations in the same order (register mode sums strictly left to right).  The cases are tests/chain_layout_cases.py's;
tests/test_chain_layout_cases_cpu.py shows on the oracle alone that every one of them is a chain that moves."""
import re

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi
from tests import chain_layout_cases as T
from tests import oracle_lib as O
from tests.test_gpu_parity import _assert_chains_bit_exact, _oracle_cfg

pytestmark = pytest.mark.gpu


def _model(d):
    return R.Model(T.spec_of(d), device=0, math_mode=_capi.MATH_STRICT)


def _assert_trace_is_the_oracles(case, tr):
    """the compared chains of a finished run against the oracle: draws, mass, step size and leapfrog counts"""
    for c in case.compare:
        want = T.oracle_run(case, c)
        assert np.array_equal(tr.chains[c], want.draws), (T.case_id(case), c, np.argwhere(tr.chains[c] != want.draws)[:3])
        assert np.array_equal(tr.mass[c], want.mass), (T.case_id(case), c)
        assert tr.stats[c].stepSize == want.stats.step_size, (T.case_id(case), c)
        assert tr.stats[c].leapfrogSteps == want.stats.leapfrog_steps, (T.case_id(case), c)
        assert tr.stats[c].warmupLeapfrogSteps == want.stats.warmup_leapfrog_steps, (T.case_id(case), c)
        assert tr.stats[c].accepted == want.stats.accepted, (T.case_id(case), c)


def _run(m, case):
    tr = m.sample(case.config, seeds=case.seeds) if case.rng is None else m.sample(case.config, rng_states=T.rng_states_of(case))
    _assert_trace_is_the_oracles(case, tr)
    return tr


# ---- 1. sizes and samplers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [d for d in T.SIZES if d not in T.REGISTER_LAYOUT_REFUSED])
def test_chain_kernel_bit_exact_at_layout_boundary(d, monkeypatch):
    spec, pack = T.spec_of(d), T.pack_of(d)
    m = _model(d)
    assert T.layout_of(m.hip_source) == (pack, T.slots_of(d), 0)
    cases = {c.label: c for c in T.size_cases(d)}
    # static HMC, 7 chains: packed where the model packs, and 7 is no multiple of 2, 4 or 8 chains per wavefront
    hmc = _assert_chains_bit_exact(spec, cases["hmc7"].config, list(cases["hmc7"].seeds))
    # EHMC / NUTS, 3 chains: one chain per wavefront (for a model that packs: the variant with RH_PACK_L 64, ring buffer in registers)
    for label in ("ehmc3", "nuts3"):
        _assert_chains_bit_exact(spec, cases[label].config, list(cases[label].seeds))
    if d <= 32:
        # 4099 diverging chains stay packed: the ring buffer behind a pointer, trajectories of different lengths in one wavefront
        for label in ("ehmc%d" % T.MANY, "nuts%d" % T.MANY):
            _run(m, cases[label])
        monkeypatch.setenv("RH_PACK", "0")
        unpacked = _model(d)
        monkeypatch.delenv("RH_PACK")
        assert T.layout_of(unpacked.hip_source) == (64, 1, 0)
        tr = unpacked.sample(cases["hmc7"].config, seeds=cases["hmc7"].seeds)
        assert np.array_equal(tr.chains, hmc.chains) and np.array_equal(tr.mass, hmc.mass)
        assert [s.stepSize for s in tr.stats] == [s.stepSize for s in hmc.stats]
        assert [s.leapfrogSteps for s in tr.stats] == [s.leapfrogSteps for s in hmc.stats]
    # the density seam packs too: one point more than two wavefronts' worth of the pack factor
    q = np.random.default_rng(d).normal(size=(2 * pack + 1, d))
    lp, g = m.density_batch(q)
    dens = O.OracleDensity(spec, O.JM_DET)
    for i in range(len(q)):
        out = dens.update(q[i])
        assert lp[i] == out[0] and np.array_equal(g[i], out[1:]), i


@pytest.mark.parametrize("d", sorted(T.REGISTER_LAYOUT_REFUSED))
def test_register_layout_this_toolchain_cannot_run_is_refused(d, monkeypatch):
    """128, 129, 511 and 512 parameters (two, three and eight register slots): not runnable on this toolchain.  Held to the
    register layout, rh_chain_kernel of a funnel of these sizes spills its vector registers (130, 140, 925 and 884 of them), the
    code-object inspection takes it out of use, and a data-free model has no other engine (at 511 rh_density_kernel spills one
    as well, and the model itself is refused).  Left to itself the engine lowers
    them memory-resident (big mode), whose sums are not the oracle's left-to-right ones."""
    stage, reason = T.REGISTER_LAYOUT_REFUSED[d]
    monkeypatch.setenv("RH_NO_CHUNKS", "1")
    monkeypatch.setenv("RH_NO_KERNEL_CACHE", "1")      # (the kernel cache keeps a marker for an attempt the engine abandons, not its code)
    if stage == "model":       # not even the density kernel fits: no kernel of the model is left, and creating it fails
        with pytest.raises(R.RainierHipError, match="no kernel of this model is fit to run on this toolchain .*: " + reason) as e:
            _model(d)
    else:
        m = _model(d)
        assert T.layout_of(m.hip_source) == (64, T.slots_of(d), 0)
        eng = m.engines()
        assert not eng["chain"] and not eng["tick"] and eng["density"] and re.search("chain engine: " + reason, eng["why"])
        hmc = T.size_cases(d)[0]
        with pytest.raises(R.RainierHipError, match="the chain engine's kernel of this model is not fit to run: " + reason) as e:
            m.sample(hmc.config, seeds=hmc.seeds)
    assert e.value.code == _capi.RH_E_UNSUPPORTED
    monkeypatch.delenv("RH_NO_CHUNKS"); monkeypatch.delenv("RH_NO_KERNEL_CACHE")
    # what the engine chooses by itself: big mode.  Its density is the oracle's bit for bit (same operations, same order); its
    # chains are held to rounding only (the kinetic energy is summed lane-partial + butterfly), on a tame run as for the models
    # beyond 512 parameters: a static step of 2e-3 accepts every proposal, so the positions do not depend on the energy's last bits
    big = _model(d)
    assert T.layout_of(big.hip_source) == (64, T.slots_of(d), 1) and big.engines()["chain"]
    q = np.random.default_rng(d).normal(size=(3, d))
    lp, g = big.density_batch(q)
    dens = O.OracleDensity(T.spec_of(d), O.JM_DET)
    for i in range(len(q)):
        out = dens.update(q[i])
        assert lp[i] == out[0] and np.array_equal(g[i], out[1:]), i
    cfg = R.make_config(5, 0, R.HMCSampler(4), R.StaticStepSize(2e-3), R.IdentityMassMatrixTuner())
    tr = big.sample(cfg, seeds=[70, 71])
    for c, seed in enumerate((70, 71)):
        want, _, st = O.sample_model(T.spec_of(d), _oracle_cfg(cfg, O.JM_DET), seed)
        assert tr.stats[c].leapfrogSteps == st.leapfrog_steps == 20 and tr.stats[c].accepted == st.accepted == 5
        np.testing.assert_allclose(tr.chains[c], want, rtol=1e-9, atol=1e-11)


# ---- 2. dense mass matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", T.DENSE_SIZES)
def test_dense_mass_matrix_bit_exact_at_layout_boundary(d):
    m = _model(d)
    assert T.layout_of(m.hip_source) == (T.pack_of(d), 1, 0)
    for case in T.dense_cases(d):
        cfg = case.config
        s = R.Sampler(m, cfg, list(case.seeds)); s.warmup(); s.run(cfg.iterations)
        got, dense = s.draws(), s.mass_dense(); stats, mdiag = s.stats(); s.close()
        for c in case.compare:
            want = T.oracle_run(case, c)
            assert np.array_equal(got[c], want.draws), (T.case_id(case), c, np.argwhere(got[c] != want.draws)[:3])
            assert np.array_equal(dense[c], want.dense), (T.case_id(case), c, np.argwhere(dense[c] != want.dense)[:3])
            assert np.array_equal(mdiag[c], want.mass), (T.case_id(case), c)
            assert stats[c].stepSize == want.stats.step_size and stats[c].leapfrogSteps == want.stats.leapfrog_steps, (T.case_id(case), c)
            assert stats[c].warmupLeapfrogSteps == want.stats.warmup_leapfrog_steps, (T.case_id(case), c)


# ---- 3. EHMC ring buffer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", T.RING_SIZES)
def test_ehmc_ring_buffer_bit_exact_at_slot_boundaries(B):
    m = _model(T.RING_DIM)
    assert T.layout_of(m.hip_source) == (16, 1, 0)
    for case in T.ring_cases(B):           # packed: entry i in the state image; unpacked: entry i in lane i % 64 of register slot i / 64
        _run(m, case)


def test_ehmc_ring_buffer_one_past_its_limit_is_refused():
    m = _model(T.RING_DIM)
    cfg = R.make_config(10, 10, R.EHMCSampler(16, 1, 64 * 4 + 1, 0.3))
    for seeds in ([1, 2, 3], list(range(T.MANY))):
        with pytest.raises(R.RainierHipError, match=r"ehmc_buf_size must be in \[1, 256\]") as e:
            m.sample(cfg, seeds=seeds)
        assert e.value.code == _capi.RH_E_INVALID
    for bad in (0, -1):
        with pytest.raises(R.RainierHipError) as e:
            m.sample(R.make_config(10, 10, R.EHMCSampler(16, 1, bad, 0.3)), seeds=[1])
        assert e.value.code == _capi.RH_E_INVALID


# ---- 4. continued RNG state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", T.RNG_SIZES)
def test_chain_continues_a_random_state_bit_exact(d):
    # rh_fill_normal's parallel polar-method path (one slot) hands element e its half of pair (e - first) / 2: first = 1 with a
    # pending gaussian, and an odd count of the remaining elements leaves a new one pending -- all four first x parity
    # combinations over odd and even d; 65 parameters take the serial fill
    m = _model(d)
    assert T.layout_of(m.hip_source) == (T.pack_of(d), T.slots_of(d), 0)
    for case in T.rng_cases(d):
        _run(m, case)
