"""What keeps tests/test_gpu_chain_layouts.py honest, without a device: every case of tests/chain_layout_cases.py is a healthy chain
on the oracle.  A chain that is stuck (a NaN Cholesky factor, a collapsed step size) compares equal whatever the kernel does, so
a case that does not move pins nothing.  A case that fails here gets another seed or window in the table -- never a skip."""
import numpy as np
import pytest

from rainier_amd import _capi
from tests import chain_layout_cases as T
from tests import oracle_lib as O


@pytest.mark.parametrize("case", T.ALL_CASES, ids=T.case_id)
def test_case_is_a_healthy_chain_on_the_oracle(case):
    assert max(case.compare) < len(case.seeds) and (case.rng is None or len(case.rng) == len(case.seeds))
    moves = []
    for chain in case.compare:
        run = T.oracle_run(case, chain)
        assert run.rc == 0 and run.stats.density_error == 0
        assert run.draws.shape == (case.config.iterations, case.d) and np.all(np.isfinite(run.draws))
        moves.append(np.any(run.draws[1:] != run.draws[:-1], axis=1))
        assert moves[-1].mean() >= 0.5, (chain, moves[-1].mean())     # no single chain of the case is stuck ...
        assert 1e-3 < run.stats.step_size < 10, (chain, run.stats.step_size)
        assert np.all(np.isfinite(run.mass)) and np.all(run.mass > 0)
        if T.is_dense(case):
            assert np.linalg.eigvalsh(run.dense).min() > 0, chain
            assert case.d == 1 or not np.allclose(run.dense, np.diag(np.diag(run.dense)))   # an estimate, not a diagonal
        if case.group == "ring":
            # the first B warm-up iterations each count a trajectory (the ring is not full), so iteration B + 1 on finds it full:
            # the write index has wrapped to slot 0 (Stats.scala:24-30)
            B = case.config.sampler().bufSize
            assert B == case.key and case.config.warmupIterations >= B + 1
            assert run.stats.warmup_leapfrog_steps >= B + 1
    # ... and at least 80 % of the case's consecutive draws differ (DualAvgTuner(0.8) aims at accepting 80 %: a single chain of 20
    # iterations scatters around that, so the bound is on the case's chains together)
    assert np.concatenate(moves).mean() >= 0.8, np.concatenate(moves).mean()


def test_dense_cases_complete_exactly_two_windows():
    for d in T.DENSE_SIZES:
        for c in T.dense_cases(d):
            mt, W = c.config.massMatrixTuner(), T.dense_window(d)
            assert (mt.initialWindowSize, mt.windowExpansion, mt.skipFirst, mt.skipLast) == (W, 1.5, 10, 10)
            assert c.config.warmupIterations == 10 + W + int(1.5 * W) + 10 and W == 3 * d + 20


def test_continued_states_cover_pending_and_fresh_streams():
    for d in T.RNG_SIZES:
        pending, fresh, mixed = T.rng_cases(d)
        assert T.rng_states_of(pending)[0][1] is not None and T.rng_states_of(fresh)[0][1] is None
        assert [g is None for _, g in T.rng_states_of(mixed)] == [False, True, False]
        # the same seed, one gaussian apart: a kernel that dropped or duplicated the pending value would land on the other chain
        assert not np.array_equal(T.oracle_run(pending, 0).draws, T.oracle_run(fresh, 0).draws)


@pytest.mark.parametrize("d", sorted(set(T.SIZES + T.DENSE_SIZES + T.RNG_SIZES + (T.RING_DIM,))))
def test_emitter_chooses_the_layout_the_table_expects(d, monkeypatch):
    # (source only: nothing is compiled)
    lower = lambda: _capi.lower_only(T.spec_of(d).rir, _capi.compile_opts(math_mode=_capi.MATH_STRICT), compile=False)[0]
    if d in T.REGISTER_LAYOUT_REFUSED:
        # (more than 1000 generated statements go to the memory-resident lowering at once: the register layout has to be asked for)
        assert T.layout_of(lower()) == (64, T.slots_of(d), 1 if d > 500 else 0)
        monkeypatch.setenv("RH_NO_CHUNKS", "1")
    src = lower()
    assert T.layout_of(src) == (T.pack_of(d), T.slots_of(d), 0)
    assert "#define RH_NVARS %d\n" % d in src


def test_kernel_variants_cover_what_the_gpu_tests_load():
    kv = T.kernel_variants()
    assert len(kv) == len(set((d, v, tuple(sorted((e or {}).items()))) for d, v, e in kv))
    have = {(d, v) for d, v, e in kv if not e}
    for d in T.SIZES:
        if d in T.REGISTER_LAYOUT_REFUSED:
            assert [k for k in kv if k[0] == d] == [(d, 0, None)]       # (the engine's own lowering of that size only)
            continue
        assert {(d, 0), (d, 1)} <= have and ({(d, 4), (d, 5)} <= have) == (d <= 32)
        assert ((d, 0, {"RH_PACK": "0"}) in kv) == (d <= 32)
    for d in T.DENSE_SIZES:
        assert ({(d, 2), (d, 6), (d, 7)} if d <= 32 else {(d, 2), (d, 3)}) <= have
    assert {(T.RING_DIM, 0), (T.RING_DIM, 4)} <= have and all((d, 0) in have for d in T.RNG_SIZES)


def test_table_covers_every_layout_boundary():
    ids = [T.case_id(c) for c in T.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert {T.pack_of(d) for d in T.SIZES} == {8, 16, 32, 64} and {T.slots_of(d) for d in T.SIZES} == {1, 2, 3, 8}
    assert {T.slots_of(d) for d in T.SIZES if d not in T.REGISTER_LAYOUT_REFUSED} == {1, 2}
    for edge in (8, 16, 32, 64, 128, 512):       # each boundary from both sides (512 is the last size below big mode)
        assert edge in T.SIZES and (edge + 1 in T.SIZES or edge == 512)
    assert max(T.DENSE_SIZES) == 64 and max(T.RING_SIZES) == 64 * 4
    assert O.JM_DET == 1
