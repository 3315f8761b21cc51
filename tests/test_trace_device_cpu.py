"""Trace.diagnostics on the device (csrc/device/rh_trace.hip.h), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its two block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in
    turn, is driven over whole buffers exactly as the kernels' launches walk them and compared with the sequential oracle
    (oracle/sampler.c: Trace.scala:52-120 restated) at the bars the project holds between the oracle and numpy
    (tests/test_oracle.py: rHat 1e-12, ess 1e-10 relative; NaN matches NaN);
  * the C ABI's argument errors, and its refusal to compute without a device.

tests/test_gpu_trace_device.py runs the same fixtures through the kernels and asks for the emulation's bits.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rainier_amd import _capi
from tests import oracle_lib as O
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_trace_chain_kernel", "rh_trace_finish_kernel")
RHAT_REL, ESS_REL = 1e-12, 1e-10          # tests/test_oracle.py:178-179

SHAPES = [(2, 2), (2, 3), (3, 99), (4, 100), (4, 101), (5, 300), (4, 1000), (3, 5000)]
NVARS = [1, 5, 64, 65]
PHIS = (0.0, 0.5, 0.9, 0.99)


def ar1_fixture(m, n, nvars, seed):
    """[m][n][nvars]: column p is a stationary AR(1) trace with phi = PHIS[p % 4] per chain, every chain moved by 0, +10 or -10
    marginal standard deviations (p % 3): the sums (x - mean)^2 must survive a mean that dwarfs the spread.
    (Seeds: checked with numpy that no column's scan comes within 1e-9 of its stopping rule -- `pt` crossing zero -- so that the
    stopping lag cannot differ between two summation orders; a seed that did would be replaced, not excused.)"""
    rng = np.random.default_rng(seed)
    phi = np.array([PHIS[p % 4] for p in range(nvars)])
    sd = 1.0 / np.sqrt(1.0 - phi * phi)
    x = np.empty((m, n, nvars))
    x[:, 0, :] = rng.normal(size=(m, nvars)) * sd
    e = rng.normal(size=(m, n, nvars))
    for i in range(1, n):
        x[:, i, :] = phi * x[:, i - 1, :] + e[:, i, :]
    shift = np.array([(0.0, 10.0, -10.0)[p % 3] for p in range(nvars)]) * sd
    return x + shift


def fixture_seed(m, n, nvars):
    return 1000 * m + 7 * n + nvars


def pt_margin(x):
    """min over columns of |pt| at the lags the scan visits (numpy, pairwise sums): how far the stopping rule is from a tie"""
    m, n, k = x.shape
    means = x.mean(axis=1)
    w = x.var(axis=1, ddof=1).mean(axis=0)
    v = (n - 1) / n * w + means.var(axis=0, ddof=1)
    worst = np.inf
    alive = np.ones(k, dtype=bool)
    for lag in range(1, min(99, n - 1) + 1):
        d = x[:, lag:, :] - x[:, :-lag, :]
        pt = 1.0 - (d * d).sum(axis=1).mean(axis=0) / (n - lag) / (2.0 * v)
        worst = min(worst, np.abs(pt[alive]).min()) if alive.any() else worst
        alive &= pt > 0
    return worst


def close(got, want, rel):
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(got - want) <= rel * abs(want)


def check_against_oracle(x, rhat, ess, what, cols=None):
    for p in (range(x.shape[2]) if cols is None else cols):
        r, e = O.diagnostics(x[:, :, p])
        assert close(rhat[p], r, RHAT_REL), (what, p, "rHat", rhat[p], r)
        assert close(ess[p], e, ESS_REL), (what, p, "ess", ess[p], e)


# ---- the device text on the host ---------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// trace_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; pc 0: the plan's chunk) and the kernels' index arithmetic, one workgroup after the other
extern "C" void rt_emulate(const double *draws, int chains, long long iterations, long long nvars, int first, int n, long long pc,
                           double *rhat, double *ess, double *mean, double *var) {
  if (pc == 0) pc = rh_plan::trace_chunk(chains, (int)nvars);
  std::vector<double> ws((size_t)pc * chains * RT_SL), lds(RT_LDS_DOUBLES + RT_TP), lds2(RT_SL + RT_FIN_BLOCK);
  for (long long p0 = 0; p0 < nvars; p0 += pc) {
    const int p_lo = (int)p0, p_cnt = (int)(pc < nvars - p0 ? pc : nvars - p0);
    const int tiles = (int)rh_plan::trace_tiles(p_cnt);
    for (int tile = 0; tile < tiles; tile++)
      for (int c = 0; c < chains; c++) {
        const int pl = tile * RT_TP;
        const int tpw = p_cnt - pl < RT_TP ? p_cnt - pl : RT_TP;
        const double *x = draws + ((long long)c * iterations + first) * nvars + p_lo + pl;
        rt_chain_block(x, nvars, n, tpw, lds.data(), ws.data() + ((long long)pl * chains + c) * RT_SL, (long long)chains * RT_SL, RT_BLOCK);
      }
    for (int pl = 0; pl < p_cnt; pl++) {
      const int p = p_lo + pl;
      rt_param_finish(ws.data() + (long long)pl * chains * RT_SL, chains, n, lds2.data(), rhat + p, ess + p, mean + p, var + p, RT_FIN_BLOCK);
    }
  }
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_trace.hip.h in host mode) + the driver above as a host shared library (g++ -O2 -ffp-contract=off: every a*b+c stays two roundings,
    as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_trace_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        L.rt_emulate.argtypes = [dp, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_longlong, dp, dp, dp, dp]
        _emu = L
    return _emu


def emulate(x, first=0, count=None, pc=0):
    """the host emulation over x [chains][iterations][nvars] -> rhat, ess, mean, var; pc: parameters per chunk (0: the engine's)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, k = x.shape
    count = iters - first if count is None else count
    out = [np.full(k, -1.0) for _ in range(4)]
    L.rt_emulate(_capi.dptr(x), m, iters, k, first, count, pc, *[_capi.dptr(o) for o in out])
    return out


def special_cases():
    """(name, draws): one chain constant, every chain constant, a chain constant in one column only"""
    x = ar1_fixture(4, 120, 5, 77)
    one = x.copy(); one[2, :, :] = 3.25
    allc = np.tile(np.arange(1.0, 6.0), (4, 120, 1))
    col = x.copy(); col[1, :, 3] = -1.5
    return [("one constant chain", one), ("all chains constant", allc), ("a constant chain in one column", col)]


# ---- 1. the code object ------------------------------------------------------------------------------------------------------------------
def test_trace_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.trace_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r       # kernel_health: metadata + isacheck's walk
    # exec restores the join-block rule cannot classify (tests/test_isacheck_cpu.py keeps such a census for the models' kernels): the
    # chain kernel has two, both the tail of an outer region's body behind an inner region's restore, neither ending in a register
    # copy (tools/unproven_census.py's classes); the finish kernel has none.  More than that is looked at before this moves.
    assert rep[("object", "rh_trace_chain_kernel")]["unproven"] <= 2 and rep[("object", "rh_trace_finish_kernel")]["unproven"] == 0
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.trace.co")))      # it travels in the kernel cache
    # a second call is served by the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.trace_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before


def test_the_model_sources_do_not_carry_the_trace_kernels():
    """model-independent: no per-model source (and so no per-model cache key) changes with it"""
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_trace" not in src


# ---- 2. the device text, on the host, against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SHAPES)
def test_host_emulation_matches_the_oracle(m, n):
    for k in NVARS:
        x = ar1_fixture(m, n, k, fixture_seed(m, n, k))
        rhat, ess, mean, var = emulate(x)
        check_against_oracle(x, rhat, ess, (m, n, k))
        np.testing.assert_allclose(mean, x.mean(axis=(0, 1)), rtol=1e-12, atol=0)
        # the chunking of the parameters is not part of the result (a chunk of 1, of 3 and of a tile and a bit)
        for pc in (1, 3, 17):
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(emulate(x, pc=pc), (rhat, ess, mean, var))), (m, n, k, pc)


def test_host_emulation_time_tiles_with_a_halo():
    """5000 rows of a 16-wide tile do not fit the staged rows: the window is walked in time tiles whose lags reach back into the
    halo -- and 1000 rows of a 5-wide tile do fit.  Both against the host entry point rh_diagnostics, whose sums run in the same
    order (i ascending, then chains ascending): the very same doubles."""
    import rainier_amd as R
    for m, n, k in ((3, 5000, 16), (4, 1000, 5), (3, 2000, 7)):
        x = ar1_fixture(m, n, k, fixture_seed(m, n, k))
        rhat, ess, _, _ = emulate(x)
        want = R.diagnostics(x)
        assert np.array_equal(rhat, [r for r, _ in want]) and np.array_equal(ess, [e for _, e in want]), (m, n, k)


def test_host_emulation_special_cases_and_windows():
    for name, x in special_cases():
        rhat, ess, _, _ = emulate(x)
        check_against_oracle(x, rhat, ess, name)
    assert np.all(np.isnan(emulate(special_cases()[1][1])[0]))            # a constant trace: rHat = sqrt(0 / 0), as in the reference
    # a window is its rows: the same bits as a copy analysed on its own, and the oracle's figures for those rows
    x = ar1_fixture(4, 700, 20, 5)
    for first, count in ((1, 699), (37, 2), (100, 101), (250, 450), (0, 600)):
        got = emulate(x, first, count)
        own = emulate(x[:, first:first + count, :].copy())
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, own)), (first, count)
        check_against_oracle(x[:, first:first + count, :], got[0], got[1], ("window", first, count))


def test_fixture_seeds_keep_the_stopping_rule_away_from_a_tie():
    for m, n in SHAPES:
        for k in NVARS:
            assert pt_margin(ar1_fixture(m, n, k, fixture_seed(m, n, k))) > 1e-9, (m, n, k)


# ---- 3. the C ABI without a device -----------------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    a, b = np.zeros(4), np.zeros(4)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    call = lambda ptr, chains, iters, nvars, first, count, r=a, e=b: L.rh_diagnostics_device(
        ptr, 0, chains, iters, nvars, first, count, _capi.dptr(r) if r is not None else None, _capi.dptr(e) if e is not None else None, None, None)
    err = lambda: L.rh_last_error(None).decode()
    assert call(None, 4, 10, 4, 0, 10) == _capi.RH_E_INVALID
    assert call(fake, 4, 10, 4, 0, 10, r=None) == _capi.RH_E_INVALID and call(fake, 4, 10, 4, 0, 10, e=None) == _capi.RH_E_INVALID
    for first, count in ((0, 1), (0, 0), (0, 11), (5, 6), (-1, 5), (10, 2)):
        assert call(fake, 4, 10, 4, first, count) == _capi.RH_E_INVALID, (first, count)
        assert "window" in err()
    assert call(fake, 4, 10, 0, 0, 10) == _capi.RH_E_INVALID
    assert call(fake, 1, 10, 4, 0, 10) == _capi.RH_E_INVALID
    assert err() == "requirement failed: diagnostics requires multiple chains"          # Trace.scala:12
    assert L.rh_sampler_diagnostics(None, 0, 10, _capi.dptr(a), _capi.dptr(b), None, None) == _capi.RH_E_INVALID
    if L.rh_device_count() == 0:
        assert call(fake, 4, 10, 4, 0, 10) == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.diagnostics_device(4096, 4, 10, 4)


def test_python_surface():
    import inspect
    import rainier_amd as R
    from rainier_amd import distributed
    assert list(inspect.signature(R.Sampler.diagnostics).parameters) == ["self", "first", "count", "moments"]
    assert list(inspect.signature(R.diagnostics_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "moments"]
    assert callable(distributed.Comm.diagnostics)
