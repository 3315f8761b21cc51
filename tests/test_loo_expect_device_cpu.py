"""PSIS leave-one-out expectations and LOO-PIT on the device (csrc/device/rh_loo_expect.hip.h), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) -- the emulation -- and
    compared with an independent numpy / longdouble restatement of the contract in include/rainier_hip.h, at four times the largest
    relative difference measured over SHAPES (LOOX_MEASURED); pareto_k and tail_n have the bits of rh_loo's emulation;
  * identities that need no tolerance of their own, ties (group-mean weights, and against the `loo` package's stable-order
    assignment), NaN and infinity, the plan's arithmetic, chunking and pair order, the C ABI's refusals;
  * what the figures mean: the conjugate normal model, whose leave-one-out posterior and predictive distribution are known.

How a relative difference is taken: |got - want| / |want| for var, pit, pit_lt and ess (sums of terms of one sign); for the mean the
divisor is sum W |v| / sum W, which is what the rounding of a sum of terms of both signs is relative to; for pareto_k max(1, |k|), as
tests/test_loo_device_cpu.py takes it (k may be near 0).  Where the restatement gives exactly 0 the emulation must too.

tests/test_gpu_loo_expect_device.py runs the same shapes through the kernels.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta
from tests.test_loo_device_cpu import (LOO_MEASURED, NKINDS, NVARS, SHAPES, case, conjugate, fixture, pooled, same_bits, tail_len, to_keys)  # noqa: F401
from tests import test_loo_device_cpu as LOO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_loo_expect_sort_kernel", "rh_loo_expect_merge_kernel", "rh_loo_expect_fit_kernel", "rh_loo_expect_reduce_kernel")
CAP, TILE, MERGE_TILE, TAIL_MAX = 128 << 20, 4096, 2048, 8064
LD = np.longdouble
DOUBLES = ("mean", "var", "pit", "pit_lt", "ess", "pareto_k")
FIELDS = DOUBLES + ("tail_n",)
VKINDS = 4
CONST = 3.7
# the largest relative difference (the module's docstring says of what) of mean, var, pit, pit_lt, ess, pareto_k and the draws' weights
# from the longdouble restatement, measured over SHAPES (profiles/loo_expect_device: on the host, never against the device).  All of
# it is the kind 1 columns', whose k is about 10 (ess 1.0001): a tail weight takes the fit's difference in k times |log1p(-p)| <= 6.3,
# and the mean and variance of such a column are a few tail weights'.  Every other column stays below 1.2e-13, pareto_k's own figure.
LOOX_MEASURED = 5.6e-12
# the conjugate fixture (seed 2017, S = 20000, y_rep from default_rng(7)): max |mean - exact|, max relative variance error,
# max |pit - exact|, max k (profiles/loo_expect_device)
CONJ_MEAN_MEASURED, CONJ_VAR_MEASURED, CONJ_PIT_MEASURED, CONJ_K_MEASURED = 0.0082, 0.031, 0.0040, 0.22


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def values(x, seed):
    """the value buffer that goes with a log-likelihood buffer x = fixture(.., seed) [chains][iters][nll]: column 4 p + r belongs to
    log-likelihood column p and is of kind r: 0 a smooth function of the same theta, 1 a copy of exp(l), 2 the constant CONST, 3
    y_rep-like noise around theta"""
    chains, iters, nll = x.shape
    t = np.random.default_rng(seed).standard_normal((chains, iters, nll))           # fixture()'s theta
    noise = np.random.default_rng(seed + 5000).standard_normal((chains, iters, nll))
    v = np.empty((chains, iters, VKINDS * nll))
    with np.errstate(all="ignore"):
        v[:, :, 0::4] = 0.5 * t + 0.1 * t * t
        v[:, :, 1::4] = np.exp(x)
        v[:, :, 2::4] = CONST
        v[:, :, 3::4] = t + noise
    return v


def all_pairs(nll):
    return [p for p in range(nll) for _ in range(VKINDS)], [VKINDS * p + r for p in range(nll) for r in range(VKINDS)]


def observations(v, first, count, thin, vcols):
    """y [K]: the value of the window's second draw, so that <= and < differ by at least that draw's weight"""
    pv = pooled(v, first, count, thin, vcols)
    return np.ascontiguousarray(pv[:, 1])


def case_x(i, bad=np.nan):
    """shape i of SHAPES -> (ll, val, first, count, thin, ll_cols, val_cols, y)"""
    x, first, count, thin = case(i, bad)
    v = values(x, 200 + i)
    lc, vc = all_pairs(x.shape[2])
    return x, v, first, count, thin, lc, vc, observations(v, first, count, thin, vc)


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
def logsumexp(v):
    top = v.max()
    return top + np.log(np.exp(v - top).sum())


def restate_weights(l, ties="group"):
    """The contract's (a) and (b) on one column l [S] in draw order, in longdouble where it is not a comparison of doubles
    -> (W [S] longdouble, pareto_k, tail_n); None where the column is not finite.  ties: "group" (the contract: the mean over the
    positions of equal values) or "stable" (the `loo` package: the tail's weights in the stable ascending order of the ratios)"""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    if not np.all(np.isfinite(l)):
        return None
    a = np.sort(l)
    x = a[0] - a                                               # descending along a, in double
    M = tail_len(S)
    lc = max(x[M], math.log(np.finfo(np.float64).tiny))
    n = int(np.count_nonzero(x > lc))
    assert np.all(x[:n] > lc) and n <= M
    W = np.exp((a[0] - l).astype(LD))
    k = math.inf
    if n > 4:
        elc = np.exp(LD(lc))
        t = (np.exp(x[:n].astype(LD)) - elc)[::-1]             # ascending
        m = 30 + int(math.floor(math.sqrt(n)))
        j = np.arange(1, m + 1).astype(LD)
        with np.errstate(all="ignore"):
            b = (LD(1) - np.sqrt(LD(m) / (j - LD(0.5)))) / (LD(3) * t[int(math.floor(n / 4.0 + 0.5)) - 1]) + LD(1) / t[n - 1]
            kj = np.log1p(-b[:, None] * t[None, :]).sum(axis=1) / LD(n)
            Lj = LD(n) * (np.log(-b / kj) - kj - LD(1))
            w = np.exp(Lj - logsumexp(Lj))
            bbar = (b * w).sum()
            khat = np.log1p(-bbar * t).sum() / LD(n)
            sigma = -khat / bbar
            kk = (LD(n) * khat + LD(5)) / LD(n + 10)
        if np.isfinite(kk) and np.isfinite(sigma):
            k = float(kk)
            p = (np.arange(1, n + 1).astype(LD) - LD(0.5)) / LD(n)
            with np.errstate(all="ignore"):
                q = -sigma * np.log1p(-p) if kk == 0 else sigma * np.expm1(-kk * np.log1p(-p)) / kk
                v = np.log(q + elc)
            e = np.exp(np.where(v > 0, LD(0), v))              # e [j - 1] = exp(lw_j), j = 1 .. n in ascending ratio
            if ties == "group":
                at = e[::-1]                                   # by position of a: position p holds j = n - p
                starts = np.flatnonzero(np.concatenate([[True], a[1:n] != a[:n - 1]]))
                ends = np.concatenate([starts[1:], [n]])
                assert a[n - 1] != a[n]                        # a group of ties lies wholly inside the tail
                gmean = np.add.reduceat(at, starts) / (ends - starts).astype(LD)
                lo = np.searchsorted(a, l, "left")
                inside = lo < n
                W[inside] = gmean[np.searchsorted(starts, lo[inside])]
            else:
                order = np.argsort(-l, kind="stable")          # ascending ratios, earlier draws first among equals
                W[order[S - n:]] = e
    return W, k, n


def restate_pair(l, v, y=None, ties="group"):
    """the contract on one pair -> dict of floats (pit, pit_lt only with y)"""
    v = np.asarray(v, dtype=np.float64)
    nan = float("nan")
    got = restate_weights(l, ties)
    if got is None:
        return dict(mean=nan, var=nan, pit=nan, pit_lt=nan, ess=nan, pareto_k=nan, tail_n=0, scale=nan)
    W, k, n = got
    den = W.sum()
    out = dict(ess=float(den * den / (W * W).sum()), pareto_k=k, tail_n=n)
    if not np.all(np.isfinite(v)):
        out.update(mean=nan, var=nan, pit=nan, pit_lt=nan, scale=nan)
        return out
    V = v.astype(LD)
    mean = (W * V).sum() / den
    out.update(mean=float(mean), var=float((W * (V - mean) ** 2).sum() / den), scale=float((W * np.abs(V)).sum() / den))
    if y is not None:
        ok = not math.isnan(y)
        out.update(pit=float(W[v <= y].sum() / den) if ok else nan, pit_lt=float(W[v < y].sum() / den) if ok else nan)
    return out


def rel_diffs(got, want, const_v=False):
    """the relative differences of the docstring, one per figure that is not NaN; asserts what must be equal.  const_v: the values are
    one constant, whose variance is rounding alone on either side (test_identities bounds it)"""
    out = {}
    for f in DOUBLES:
        if f == "var" and const_v:
            continue
        g, w = float(got[f]), float(want[f])
        assert math.isnan(g) == math.isnan(w) and math.isinf(g) == math.isinf(w), (f, g, w)
        if math.isnan(w) or math.isinf(w):
            continue
        if w == 0.0:
            assert g == 0.0, (f, g, w)
            continue
        div = want["scale"] if f == "mean" else max(1.0, abs(w)) if f == "pareto_k" else abs(w)
        out[f] = abs(g - w) / div
    return out


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// loo_expect_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter) and the kernels' index
// arithmetic, one workgroup after the other.  w_out [K][S] (the draws' weights) may be NULL.  Returns the number of chunks, -1 beyond the
// cap, -2 beyond the tail's LDS.
extern "C" int lx_emulate(const double *ll, long long nll, const double *val, long long nval, int chains, long long iterations, long long first, long long count,
                          long long thin, const int *lcols, const int *vcols, int K, const double *y, long long cap, double *mean, double *var, double *pit,
                          double *pit_lt, double *ess, double *pareto_k, int *tail_n, double *w_out) {
  const rh_plan::LooExpect P = rh_plan::loo_expect_plan(chains, count, thin, K, cap);
  if (P.over_cap) return -1;
  if (P.over_lds) return -2;
  const long long S = P.S;
  std::vector<rs_key> ka((size_t)(P.pc * S)), kb((size_t)(P.pc * S)), klds(RS_TILE_SLOTS > RS_MERGE_LDS ? RS_TILE_SLOTS : RS_MERGE_LDS);
  std::vector<double> lds(LL_LDS_DOUBLES > LX_LDS_DOUBLES ? LL_LDS_DOUBLES : LX_LDS_DOUBLES), tw((size_t)(P.pc * P.M));
  double unused = 0.0;
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0;
    rs_key *src = ka.data(), *dst = kb.data();
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
      const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE;
      if (g0 >= S) continue;
      rs_tile_sort(ll + first * nll + lcols[k0 + pl], iterations, nll, thin, P.kept, S, g0, klds.data(), src + pl * S + g0, LL_BLOCK);
    }
    for (int k = 0; k < P.passes; k++) {
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
        if (o0 >= S) continue;
        rs_merge_tile(src + pl * S, dst + pl * S, S, P.run(k), o0, klds.data(), LL_BLOCK);
      }
      std::swap(src, dst);
    }
    for (size_t i = 0; i < tw.size(); i++) tw[i] = -7.0;    // a weight that was not written shows
    for (long long pl = 0; pl < p_cnt; pl++) lx_fit_block(src + pl * S, S, P.M, lds.data(), tw.data() + pl * P.M, pareto_k + k0 + pl, tail_n + k0 + pl, LL_BLOCK);
    for (long long pl = 0; pl < p_cnt; pl++) {
      const long long k = k0 + pl;
      double *w = (double *)(dst + pl * S);
      lx_reduce_block(src + pl * S, S, tw.data() + pl * P.M, pareto_k[k], tail_n[k], ll + first * nll + lcols[k], nll, val + first * nval + vcols[k], nval, iterations,
                      thin, P.kept, y != nullptr, y ? y[k] : 0.0, w, lds.data(), mean + k, var + k, y ? pit + k : &unused, y ? pit_lt + k : &unused, ess + k, LL_BLOCK);
      if (w_out) for (long long s = 0; s < S; s++) w_out[k * S + s] = w[s];
    }
  }
  return chunks;
}
// kept, S, M, per_pair, pc, over_cap, over_lds, tiles, mtiles, passes
extern "C" void lx_plan(long long chains, long long count, long long thin, long long K, long long cap, long long *out) {
  const rh_plan::LooExpect P = cap ? rh_plan::loo_expect_plan(chains, count, thin, K, cap) : rh_plan::loo_expect_plan(chains, count, thin, K);
  const long long v[10] = {P.kept, P.S, P.M, P.per_pair, P.pc, P.over_cap ? 1 : 0, P.over_lds ? 1 : 0, P.tiles, P.mtiles, P.passes};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}
extern "C" void lx_constants(long long *out) { const long long v[4] = {LL_BLOCK, LL_LDS_DOUBLES, LX_LDS_DOUBLES, LX_WS_CAP_BYTES}; for (int i = 0; i < 4; i++) out[i] = v[i]; }
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h, rh_loo.hip.h and rh_loo_expect.hip.h in host mode) + the driver above as a host
    shared library (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_loox_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int)
        L.lx_emulate.argtypes = [dp, ll, dp, ll, C.c_int, ll, ll, ll, ll, ip, ip, C.c_int, dp, ll, dp, dp, dp, dp, dp, dp, ip, dp]
        L.lx_plan.argtypes = [ll, ll, ll, ll, ll, C.POINTER(ll)]
        L.lx_plan.restype = None
        L.lx_constants.argtypes = [C.POINTER(ll)]
        _emu = L
    return _emu


PLAN_FIELDS = ("kept", "S", "M", "per_pair", "pc", "over_cap", "over_lds", "tiles", "mtiles", "passes")


def plan(chains, count, thin, k, cap=0):
    out = (C.c_longlong * 10)()
    emulation().lx_plan(chains, count, thin, k, cap, out)
    return dict(zip(PLAN_FIELDS, list(out)))


def emulate(x, v, ll_cols, val_cols, y=None, first=0, count=None, thin=1, cap=CAP, dump=False):
    """the host emulation over x [chains][iterations][nll] and v [chains][iterations][nval] -> dict of the seven outputs [K] (pit,
    pit_lt None without y), "chunks", and with dump "w" [K][S] (the draws' weights)"""
    L = emulation()
    x, v = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    m, iters, nll = x.shape
    assert v.shape[:2] == (m, iters)
    count = iters - first if count is None else count
    lc, vc = np.ascontiguousarray(ll_cols, dtype=np.int32), np.ascontiguousarray(val_cols, dtype=np.int32)
    k = len(lc)
    assert len(vc) == k
    p = plan(m, count, thin, k, cap)
    out = {f: np.full(k, -1.0) for f in DOUBLES}
    out["tail_n"] = np.full(k, -1, dtype=np.int32)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    w = np.zeros((k, p["S"])) if dump else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    n = L.lx_emulate(_capi.dptr(x), nll, _capi.dptr(v), v.shape[2], m, iters, first, count, thin, ip(lc), ip(vc), k, _capi.dptr(yy) if yy is not None else None, cap,
                     *[_capi.dptr(out[f]) for f in DOUBLES], ip(out["tail_n"]), _capi.dptr(w) if dump else None)
    assert n >= 1, "refused"
    if yy is None:
        assert np.all(out["pit"] == -1.0) and np.all(out["pit_lt"] == -1.0)         # not written
        out["pit"] = out["pit_lt"] = None
    out["chunks"] = n
    if dump:
        out["w"] = w
    return out


_cases = {}


def emulated_case(i, bad=np.nan):
    """(ll, val, first, count, thin, ll_cols, val_cols, y, the emulation's result) of shape i, computed once and shared (the GPU tests
    compare with it)"""
    key = (i, "nan" if np.isnan(bad) else "inf")
    if key not in _cases:
        x, v, first, count, thin, lc, vc, y = case_x(i, bad)
        _cases[key] = (x, v, first, count, thin, lc, vc, y, emulate(x, v, lc, vc, y, first, count, thin, dump=True))
    return _cases[key]


def same_results(a, b, pick=None):
    """entry k of a has the bits of entry pick[k] of b (pit, pit_lt: where both have them)"""
    ix = slice(None) if pick is None else list(pick)
    for f in FIELDS:
        if a[f] is None or b[f] is None:
            assert f in ("pit", "pit_lt")
            continue
        if not same_bits(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64)[ix]):
            return False
    return True


def shuffled_with_duplicate(k, seed):
    rng = np.random.default_rng(seed)
    pick = list(rng.permutation(k)[:max(1, (2 * k) // 3)])
    return [int(c) for c in pick + pick[:1]]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_loo_expect_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.loo_expect_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r   # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.loo_expect.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.loo_expect_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_other_code_objects_do_not_carry_the_loo_expect_kernels():
    for other in (_capi.loo_lower_only, _capi.summary_lower_only, _capi.rank_lower_only):
        assert b"rh_loo_expect" not in other("gfx950")


# ---- 2. the public surface -----------------------------------------------------------------------------------------------------------
def test_exports_and_python_surface():
    import inspect
    import rainier_amd as R
    L = _capi.lib()
    for name in ("rh_loo_expect_device", "rh_sampler_loo_expect", "rh_loo_expect_lower_only"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert R.LooExpect._fields == ("mean", "var", "pit", "pit_lt", "ess", "pareto_k", "tail_n", "ll_cols", "val_cols")
    assert list(inspect.signature(R.loo_expect_device).parameters) == ["ll_ptr", "val_ptr", "chains", "iterations", "nll", "nval", "ll_cols", "val_cols", "y", "device",
                                                                       "first", "count", "thin"]
    sig = inspect.signature(R.loo_expect_device).parameters
    assert sig["y"].default is None and sig["device"].default == 0 and sig["first"].default == 0 and sig["count"].default is None and sig["thin"].default == 1
    assert list(inspect.signature(R.Sampler.loo_expect).parameters) == ["self", "ll_predictor", "predictor", "ll_cols", "val_cols", "y", "generator", "seed", "first",
                                                                        "count", "thin"]
    sig = inspect.signature(R.Sampler.loo_expect).parameters
    assert all(sig[n].default is None for n in ("ll_cols", "val_cols", "y", "generator", "count"))
    assert sig["seed"].default == 0 and sig["first"].default == 0 and sig["thin"].default == 1
    with pytest.raises(ValueError, match="pair up"):
        R.loo_expect_device(4096, 4096, 4, 10, 2, 2, [0, 1], [0])
    with pytest.raises(ValueError, match="y has"):
        R.loo_expect_device(4096, 4096, 4, 10, 2, 2, [0, 1], [0, 1], y=[0.5])


# ---- 3. bits and figures -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, -np.inf])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_figures_against_the_longdouble_restatement(i, bad):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, bad)
    pl, pv = pooled(x, first, count, thin, lc), pooled(v, first, count, thin, vc)
    S = pl.shape[1]
    assert S == SHAPES[i][0] * -(-count // thin) == emu["w"].shape[1]
    loo = LOO.emulated_case(i, bad)[4]                         # rh_loo's emulation of the same buffer
    worst = 0.0
    for k in range(len(lc)):
        got = {f: emu[f][k] for f in FIELDS}
        # the tail fit is rh_loo's, bit for bit
        assert same_bits(got["pareto_k"], loo["pareto_k"][lc[k]]) and got["tail_n"] == loo["tail_n"][lc[k]], (SHAPES[i], k)
        want = restate_pair(pl[k], pv[k], float(y[k]))
        assert got["tail_n"] == want["tail_n"], (SHAPES[i], k, got, want)
        if lc[k] % NKINDS == 5:
            assert all(np.isnan(got[f]) for f in DOUBLES) and got["tail_n"] == 0, (SHAPES[i], k)
            continue
        W = restate_weights(pl[k])[0]
        assert np.all(emu["w"][k] <= 1.0) and np.all(emu["w"][k] > 0.0)
        d = rel_diffs(got, want, bool(np.all(pv[k] == pv[k][0])))
        assert np.all(W > 0)
        d["w"] = float(np.max(np.abs(emu["w"][k].astype(LD) - W) / W))             # the draws' weights themselves
        assert all(e <= 4 * LOOX_MEASURED for e in d.values()), (SHAPES[i], k, d, got, want)
        worst = max([worst] + list(d.values()))
        assert got["pit_lt"] <= got["pit"] and 1.0 <= got["ess"] <= S, (SHAPES[i], k, got)
    print("largest relative difference of mean / var / pit / pit_lt / ess / pareto_k from the restatement: %.3g" % worst)
    assert worst <= LOOX_MEASURED


# ---- 4. identities that need no tolerance of their own -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_identities(i):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i)
    S = emu["w"].shape[1]
    loo = LOO.emulated_case(i)[4]
    pv = pooled(v, first, count, thin, vc)
    k = len(lc)
    hi = emulate(x, v, lc, vc, np.full(k, np.inf), first, count, thin)
    lo = emulate(x, v, lc, vc, np.full(k, -np.inf), first, count, thin)
    none = emulate(x, v, lc, vc, None, first, count, thin)
    assert none["pit"] is None and none["pit_lt"] is None and same_results(none, emu)
    for j in range(k):
        lkind, vkind = lc[j] % NKINDS, vc[j] % VKINDS
        if lkind == 5:
            assert np.isnan(hi["pit"][j]) and np.isnan(lo["pit_lt"][j])
            continue
        # y = +inf: the sums den runs, in den's order; y = -inf: nothing
        assert hi["pit"][j] == 1.0 and hi["pit_lt"][j] == 1.0 and lo["pit"][j] == 0.0 and lo["pit_lt"][j] == 0.0, (SHAPES[i], j)
        if vkind == 1 and lkind != 3:            # val = exp(l) (kind 3's exp(-1000) is not a double's): log(mean) is elpd_loo, by another route
            assert abs(math.log(emu["mean"][j]) - loo["elpd_loo"][lc[j]]) <= 8 * LOO_MEASURED * abs(loo["elpd_loo"][lc[j]]), (SHAPES[i], j)
        if vkind == 2:
            ulp = np.spacing(CONST)
            assert abs(emu["mean"][j] - CONST) <= 4 * ulp and 0.0 <= emu["var"][j] <= (4 * ulp * CONST) ** 2, (SHAPES[i], j, emu["mean"][j], emu["var"][j])
        if lkind == 4:                           # a constant log-likelihood: every weight is 1
            assert math.isinf(emu["pareto_k"][j]) and emu["tail_n"][j] == 0 and emu["ess"][j] == float(S) and np.all(emu["w"][j] == 1.0)
        if lkind == 4 and vkind in (0, 3):
            pm = pv[j].astype(LD).mean()
            assert abs(emu["mean"][j] - float(pm)) <= 4 * LOOX_MEASURED * float(np.abs(pv[j]).mean())
            assert abs(emu["var"][j] - float(((pv[j].astype(LD) - pm) ** 2).mean())) <= 4 * LOOX_MEASURED * emu["var"][j]
        assert emu["pit_lt"][j] <= emu["pit"][j] and 1.0 <= emu["ess"][j] <= S


# ---- 5. ties -------------------------------------------------------------------------------------------------------------------------
def test_ties_share_their_groups_mean_weight():
    # the quarter-rounded kind 2 at S = 20000: long groups of ties inside the tail
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(len(SHAPES) - 1)
    pl = pooled(x, first, count, thin, lc)
    for k in [j for j in range(len(lc)) if lc[j] % NKINDS == 2]:
        W, _, n = restate_weights(pl[k])
        assert n > 4 and len(np.unique(np.sort(pl[k])[:n])) < n                     # the tail has ties
        w = emu["w"][k]
        for val in np.unique(pl[k]):
            assert len(np.unique(w[pl[k] == val])) == 1                            # equal log-likelihoods, equal weights
        assert np.max(np.abs(w.astype(LD) - W) / W) <= 4 * LOOX_MEASURED


def test_repeated_draws_agree_with_the_stable_order_assignment():
    # every draw repeated once with identical l and v (a rejected proposal): the group-mean rule against the `loo` package's
    ll, _ = conjugate()
    rng = np.random.default_rng(2017)
    yobs = rng.standard_normal(10) + 0.7
    theta = yobs.mean() + rng.standard_normal((16, 1250)) / math.sqrt(10)
    yrep = theta + np.random.default_rng(7).standard_normal((16, 1250))
    x = np.ascontiguousarray(np.repeat(ll[:, :400, :], 2, axis=1))                 # [16][800][10]: S = 12800
    v = np.ascontiguousarray(np.repeat(np.stack([theta, yrep], axis=2)[:, :400, :], 2, axis=1))
    lc, vc = list(range(10)) * 2, [0] * 10 + [1] * 10
    y = np.concatenate([yobs, yobs])
    emu = emulate(x, v, lc, vc, y)
    pl, pv = pooled(x, cols=lc), pooled(v, cols=vc)
    worst = 0.0
    for k in range(len(lc)):
        got = {f: emu[f][k] for f in FIELDS}
        assert emu["tail_n"][k] > 4 and np.isfinite(emu["pareto_k"][k])
        for ties in ("group", "stable"):
            want = restate_pair(pl[k], pv[k], float(y[k]), ties)
            d = rel_diffs(got, want)
            if ties == "stable":
                # sum W^2 is not the same sum under the two rules -- w1^2 + w2^2 against 2 ((w1 + w2) / 2)^2 for a repeated tail draw --,
                # so ess differs by what the tail holds of it and is left to the group-mean restatement; every sum of W f(v) is the
                # same sum under both, since repeated draws have one v
                assert abs(got["ess"] - want["ess"]) <= 1e-3 * want["ess"]
                del d["ess"]
            assert got["tail_n"] == want["tail_n"] and all(e <= 4 * LOOX_MEASURED for e in d.values()), (ties, k, d)
            worst = max([worst] + list(d.values()))
    print("repeated draws: largest relative difference from the group-mean and the stable-order restatements: %.3g" % worst)


# ---- 6. NaN and infinity -------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_in_either_window_touch_their_own_pairs_only():
    x, v, first, count, thin, lc, vc, y = case_x(5)         # 5 chains, count 819, 13 log-likelihood columns; 5 and 11 hold a NaN already
    clean = emulate(x, v, lc, vc, y, first, count, thin)
    bx, bv = x.copy(), v.copy()
    bx[2, first + 100, 0] = np.nan
    bx[4, first + 7, 6] = np.inf
    bx[0, first + count - 1, 9] = -np.inf
    bx[0, first - 1, 1] = np.nan                            # outside the window
    bx[1, first + count, 2] = np.inf                        # outside the window
    bv[3, first + 5, 4 * 3 + 0] = np.nan
    bv[0, first, 4 * 4 + 3] = np.inf
    bv[1, first + count - 1, 4 * 7 + 2] = -np.inf
    bv[0, first - 1, 4 * 8 + 0] = np.nan                    # outside the window
    bv[2, first + count, 4 * 8 + 3] = np.inf                # outside the window
    yy = y.copy()
    yy[4 * 10 + 1] = np.nan
    got = emulate(bx, bv, lc, vc, yy, first, count, thin)
    for k in range(len(lc)):
        if lc[k] in (0, 6, 9, 5, 11):
            assert all(np.isnan(got[f][k]) for f in DOUBLES) and got["tail_n"][k] == 0, k
        elif vc[k] in (4 * 3, 4 * 4 + 3, 4 * 7 + 2):
            assert all(np.isnan(got[f][k]) for f in ("mean", "var", "pit", "pit_lt")), k
            assert all(same_bits(got[f][k], clean[f][k]) for f in ("ess", "pareto_k", "tail_n")) and np.isfinite(got["ess"][k]), k
        elif k == 4 * 10 + 1:
            assert np.isnan(got["pit"][k]) and np.isnan(got["pit_lt"][k]), k
            assert all(same_bits(got[f][k], clean[f][k]) for f in ("mean", "var", "ess", "pareto_k", "tail_n")), k
        else:
            assert all(same_bits(got[f][k], clean[f][k]) for f in FIELDS), k
            assert np.isfinite(got["mean"][k]) and np.isfinite(got["pit"][k])
    # thinning steps over a bad value
    x2, v2, first, count, thin, lc, vc, y = case_x(8)
    assert thin == 2
    x2[0, first + 1, 0] = np.nan
    v2[1, first + 3, 1] = -np.inf
    assert same_results(emulate(x2, v2, lc, vc, y, first, count, thin), emulated_case(8)[8])


# ---- 7. the plan, chunking, pair order -----------------------------------------------------------------------------------------------
def test_the_plan_is_arithmetic_over_the_headers_constants():
    consts = (C.c_longlong * 4)()
    emulation().lx_constants(consts)
    assert list(consts) == [256, TAIL_MAX + 768, 7 * 256, CAP]
    for chains, count, thin, k in ((1, 2, 1, 1), (4, 5, 1, 6), (2, 8194, 2, 6), (16, 1250, 1, 13), (1024, 200, 1, 434), (64, 2000, 1, 70), (3, 100, 7, 5)):
        kept = -(-count // thin)
        S = chains * kept
        M = tail_len(S)
        tiles, passes = -(-S // TILE), 0
        while TILE << passes < S:
            passes += 1
        per = 16 * S + 8 * M
        want = dict(kept=kept, S=S, M=M, per_pair=per, pc=max(1, min(CAP // per, k)), over_cap=0, over_lds=0, tiles=tiles, mtiles=-(-S // MERGE_TILE), passes=passes)
        assert plan(chains, count, thin, k) == want, (chains, count, thin, k)
        q = LOO.plan(chains, count, thin, k)
        assert all(want[f] == q[f] for f in ("kept", "S", "M", "tiles", "mtiles", "passes"))      # the sort plan is the summary's, the tail rh_loo's
    # the GPU tier's buffer that crosses the cap: 70 pairs of 128 000 draws, 65 + 5
    assert plan(64, 2000, 1, 70)["pc"] == 65
    # refused from the shape alone: M beyond the tail's LDS, one pair beyond the cap
    assert plan(1, 7225344, 1, 1)["over_lds"] == 0 and plan(1, 7225345, 1, 1)["over_lds"] == 1 and plan(1, 7225345, 1, 1)["over_cap"] == 0
    assert plan(1, 1 << 23, 1, 1)["over_cap"] == 1 and plan(1, 8384000, 1, 1)["over_cap"] == 0 and plan(1, 1 << 23, 1, 1)["pc"] == 1
    x = fixture(2, 40, 3, 1)
    sel = (C.c_int * 3)(0, 1, 2)
    assert emulation().lx_emulate(_capi.dptr(x), 3, _capi.dptr(x), 3, 2, 40, 0, 40, 1, sel, sel, 3, None, plan(2, 40, 1, 3)["per_pair"] - 1, *[None] * 8) == -1


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_properties_of_the_contract(i):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i)
    chains, k = SHAPES[i][0], len(lc)
    # a second call gives the same bits
    assert same_results(emulate(x, v, lc, vc, y, first, count, thin), emu), SHAPES[i]
    # a window gives the bits of its copy (thinned on the host)
    cut = lambda a: np.ascontiguousarray(a[:, first:first + count:thin, :])
    assert same_results(emulate(cut(x), cut(v), lc, vc, y), emu), SHAPES[i]
    # a shuffled pair list with a duplicate gives the bits of the full call's entries
    pick = shuffled_with_duplicate(k, i)
    assert same_results(emulate(x, v, [lc[j] for j in pick], [vc[j] for j in pick], y[pick], first, count, thin), emu, pick), SHAPES[i]
    # forcing several chunks gives the same bits
    p = plan(chains, count, thin, k)
    small = emulate(x, v, lc, vc, y, first, count, thin, cap=3 * p["per_pair"])
    assert small["chunks"] == -(-k // 3) and emu["chunks"] == 1 and same_results(small, emu), SHAPES[i]
    # one buffer for both: the value is the log-likelihood itself
    both = emulate(x, x, lc, lc, None, first, count, thin)
    assert same_bits(both["pareto_k"], emu["pareto_k"]) and same_bits(both["ess"], emu["ess"])


# ---- 8. what the figures mean --------------------------------------------------------------------------------------------------------
def test_conjugate_normal_model_against_the_analytic_leave_one_out_distribution():
    n = 10
    ll, exact_elpd = conjugate()
    rng = np.random.default_rng(2017)                          # conjugate()'s own draws
    yobs = rng.standard_normal(n) + 0.7
    theta = yobs.mean() + rng.standard_normal((16, 1250)) / math.sqrt(n)
    assert np.array_equal(ll, -0.5 * math.log(2.0 * math.pi) - 0.5 * (yobs[None, None, :] - theta[:, :, None]) ** 2)
    yrep = theta + np.random.default_rng(7).standard_normal((16, 1250))
    v = np.ascontiguousarray(np.stack([theta, yrep, np.exp(ll[:, :, 0])], axis=2))
    lc, vc = list(range(n)) * 2 + [0], [0] * n + [1] * n + [2]
    emu = emulate(ll, v, lc, vc, np.concatenate([yobs, yobs, [0.0]]))
    others = (yobs.sum() - yobs) / (n - 1)
    pit_exact = np.array([0.5 * (1.0 + math.erf((yobs[i] - others[i]) / math.sqrt(2.0 * (1.0 + 1.0 / (n - 1))))) for i in range(n)])
    d_mean = float(np.max(np.abs(emu["mean"][:n] - others)))
    d_var = float(np.max(np.abs(emu["var"][:n] * (n - 1) - 1.0)))
    d_pit = float(np.max(np.abs(emu["pit"][n:2 * n] - pit_exact)))
    k = float(np.max(emu["pareto_k"]))
    d_elpd = abs(math.log(emu["mean"][2 * n]) - exact_elpd[0])
    print("conjugate fixture: max |mean - exact| %.4f, max relative variance error %.4f, max |pit - exact| %.4f, max k %.3f, |log E_loo[exp l_0] - exact| %.4f"
          % (d_mean, d_var, d_pit, k, d_elpd))
    assert d_mean <= CONJ_MEAN_MEASURED and d_var <= CONJ_VAR_MEASURED and d_pit <= CONJ_PIT_MEASURED and k <= CONJ_K_MEASURED   # the README's figures are what is measured
    assert d_mean <= 2 * CONJ_MEAN_MEASURED and d_var <= 2 * CONJ_VAR_MEASURED and d_pit <= 2 * CONJ_PIT_MEASURED and k < 0.7        # the bound: twice them
    assert d_elpd <= LOO.CONJ_LOO_MEASURED
    assert np.all(emu["pit_lt"] <= emu["pit"]) and np.all(emu["ess"] > 0.5 * 20000) and np.all(emu["tail_n"] == tail_len(20000))


# ---- 9. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    outs = [np.zeros(8) for _ in range(6)]
    tn = np.zeros(8, dtype=np.int32)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ll=fake, val=fake, chains=4, iters=10, nll=2, nval=3, first=0, count=10, thin=1, lc=(0, 1), vc=(2, 0), ncols=None, y=None, null=None, no_lc=False,
             no_vc=False):
        a, b = np.array(lc, dtype=np.int32), np.array(vc, dtype=np.int32)
        yy = None if y is None else np.array(y, dtype=np.float64)
        o = [_capi.dptr(z) for z in outs] + [tn.ctypes.data_as(ip)]
        for i in ([] if null is None else null):
            o[i] = None
        return L.rh_loo_expect_device(ll, nll, val, nval, 0, chains, iters, first, count, thin, None if no_lc else a.ctypes.data_as(ip),
                                      None if no_vc else b.ctypes.data_as(ip), len(a) if ncols is None else ncols, _capi.dptr(yy) if yy is not None else None, *o)
    err = lambda: L.rh_last_error(None).decode()
    assert call(ll=None) == _capi.RH_E_INVALID and call(val=None) == _capi.RH_E_INVALID
    assert call(no_lc=True) == _capi.RH_E_INVALID and "NULL" in err() and call(no_vc=True) == _capi.RH_E_INVALID and "NULL" in err()
    for null in (0, 1, 4, 5, 6):
        assert call(null=[null]) == _capi.RH_E_INVALID and "NULL" in err()
    for null in (2, 3):                                     # pit, pit_lt: needed with y only
        assert call(null=[null], y=[0.0, 1.0]) == _capi.RH_E_INVALID and "NULL" in err()
    for first, count, thin in ((0, 0, 1), (0, 11, 1), (7, 4, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):
        assert call(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
        assert "window" in err()
    assert call(nll=0) == _capi.RH_E_INVALID and call(nval=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    # S < 2: one chain, one kept draw
    assert call(chains=1, count=1) == _capi.RH_E_INVALID and "at least 2" in err()
    assert call(chains=1, count=10, thin=10) == _capi.RH_E_INVALID and "at least 2" in err()
    for lc, vc in (((2, 0), (0, 0)), ((-1, 0), (0, 0)), ((0, 1), (3, 0)), ((0, 1), (0, -1))):
        assert call(lc=lc, vc=vc) == _capi.RH_E_INVALID and "outside" in err(), (lc, vc)
    assert call(ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    o = [_capi.dptr(z) for z in outs] + [tn.ctypes.data_as(ip)]
    sel = np.zeros(2, dtype=np.int32)
    assert L.rh_sampler_loo_expect(None, None, None, None, 0, 0, 10, 1, sel.ctypes.data_as(ip), sel.ctypes.data_as(ip), 2, None, *o) == _capi.RH_E_INVALID
    # one pair beyond the workspace cap, and one whose tail is beyond the LDS: refused from the shape, whatever the machine
    assert call(chains=4097, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    assert call(chains=3600, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "LDS" in err()
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(null=[2, 3]) == _capi.RH_E_DEVICE and call(y=[0.5, np.nan]) == _capi.RH_E_DEVICE
        assert call(lc=(1, 1, 0), vc=(0, 0, 2)) == _capi.RH_E_DEVICE and call(chains=1, count=2) == _capi.RH_E_DEVICE and call(thin=3) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.loo_expect_device(4096, 4096, 4, 10, 4, 4, [0], [1])
