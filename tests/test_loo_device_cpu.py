"""Pointwise WAIC and PSIS-LOO on the device (csrc/device/rh_loo.hip.h; Vehtari, Gelman, Gabry 2017), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routine, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) -- the emulation -- and
    compared with an independent numpy / longdouble restatement of the contract in include/rainier_hip.h:
      - exp, log, log1p, expm1: with numpy's longdouble functions at four times the largest relative difference measured here;
      - lpd and p_waic at bounds that are derived, not tuned: with u = 2^-53, exp and log within one ulp (2u relative),
            |lpd - ref|    <= u (S + 4 + max|l - max| + 4 (|max| + |log sum| + log S))      (the argument's rounding, exp, S - 1 adds in
                                                                                          any order, two logs, two adds)
            |p_waic - ref| <= ((S + 6) u sum (l - mean)^2 + 2 S d^2) / (S - 1),  d = (S + 2) u sum|l| / S the mean's error
      - elpd_loo and pareto_k: with the restatement fed the emulation's own sorted column, at four times the largest relative
        difference measured over SHAPES (|dk| / max(1, |k|) for k, which may be near 0); tail_n and the k = +inf cases exactly;
  * the properties of the contract (a shuffled column list with a duplicate, chunking, a window and its copy, NaN / inf / constant
    columns), the plan's arithmetic, the shape-only refusals, the C ABI's argument errors and its refusal to compute without a device;
  * what the figures mean: a conjugate normal model whose leave-one-out densities are known in closed form.

tests/test_gpu_loo_device.py runs the same shapes through the kernels.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_loo_sort_kernel", "rh_loo_merge_kernel", "rh_loo_column_kernel")
CAP, TILE, MERGE_TILE, TAIL_MAX = 128 << 20, 4096, 2048, 8064
U53 = 2.0 ** -53
LD = np.longdouble
# the largest relative difference of ll_exp, ll_log, ll_log1p, ll_expm1 from numpy's longdouble functions over the grids of
# test_transcendentals_against_numpy (profiles/loo_device: measured against numpy on the host, never against the device)
EXP_MEASURED, LOG_MEASURED, LOG1P_MEASURED, EXPM1_MEASURED = 1.4e-16, 1.5e-16, 3.2e-16, 3.2e-16
# the largest relative difference of elpd_loo and pareto_k from the longdouble restatement fed the emulation's sorted column, measured
# over SHAPES (profiles/loo_device)
LOO_MEASURED = 1.2e-13
# the conjugate fixture (seed 2017, S = 20000): max |elpd_loo - exact|, max |elpd_waic - exact|, max k (profiles/loo_device)
CONJ_LOO_MEASURED, CONJ_WAIC_MEASURED, CONJ_K_MEASURED = 0.0112, 0.0074, 0.22

# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
NKINDS = 6
# (chains, count, thin): the smallest S; S = 20 and 21 (n = 4 against 5: the k = +inf boundary); 26; S just under, at and just over one
# sort tile; thinning with two merge passes; S = 20000
SHAPES = ((1, 2, 1), (1, 4, 1), (4, 5, 1), (3, 7, 1), (2, 13, 1), (5, 819, 1), (4, 1024, 1), (1, 4097, 1), (2, 8194, 2), (16, 1250, 1))
NVARS = (6, 7, 13)
FIELDS = ("lpd", "p_waic", "elpd_loo", "pareto_k", "tail_n")


def fixture(chains, iters, nvars, seed, bad=np.nan, bad_at=0):
    """[chains][iters][nvars]; column p is of kind p % 6 over theta ~ N(0, 1): 0 -(theta - 0.3)^2 / 8, 1 -(3 theta - 4)^2 / 2, 2 kind 0
    rounded to quarters (ties), 3 -1000 - (0.05 theta)^2 / 2, 4 the constant -2.0, 5 kind 0 with `bad` at (chain 0, iteration bad_at)"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((chains, iters, nvars))
    x = -(t - 0.3) ** 2 / 8.0
    for p in range(nvars):
        kind = p % NKINDS
        if kind == 1:
            x[:, :, p] = -0.5 * (3.0 * t[:, :, p] - 4.0) ** 2
        elif kind == 2:
            x[:, :, p] = np.round(4.0 * x[:, :, p]) / 4.0
        elif kind == 3:
            x[:, :, p] = -1000.0 - 0.5 * (0.05 * t[:, :, p]) ** 2
        elif kind == 4:
            x[:, :, p] = -2.0
        elif kind == 5:
            x[0, bad_at, p] = bad
    return x


def case(i, bad=np.nan):
    """shape i of SHAPES -> (x, first, count, thin): nvars cycles through NVARS, the window starts late and ends early in a longer buffer"""
    chains, count, thin = SHAPES[i]
    first = 1 + i % 3
    return fixture(chains, first + count + 2, NVARS[i % 3], 200 + i, bad, first), first, count, thin


def pooled(x, first=0, count=None, thin=1, cols=None):
    """[K][S]: the kept iterations first + j * thin of every chain, chains outer"""
    count = x.shape[1] - first if count is None else count
    sel = range(x.shape[2]) if cols is None else cols
    w = x[:, first:first + count:thin, :]
    return np.ascontiguousarray(np.stack([w[:, :, p].reshape(-1) for p in sel]))


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
def to_keys(v):
    """Double.compare's order as uint64: negatives with all bits flipped, the others with the sign bit; every NaN the positive quiet one"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
    b[(b & np.uint64(0x7fffffffffffffff)) > np.uint64(0x7ff0000000000000)] = np.uint64(0x7ff8000000000000)
    return np.where((b >> np.uint64(63)) == 1, ~b, b ^ np.uint64(0x8000000000000000))


def from_keys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> np.uint64(63)) == 1, k ^ np.uint64(0x8000000000000000), ~k).view(np.float64)


def logsumexp(v):
    top = v.max()
    return top + np.log(np.exp(v - top).sum())


def tail_len(S):
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S))))


def restate_column(l):
    """The contract of include/rainier_hip.h on one column l [S] (in any order), in longdouble where it is not a comparison of
    doubles -> (lpd, p_waic, elpd_loo, pareto_k, tail_n)"""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    if not np.all(np.isfinite(l)):
        return (float("nan"),) * 4 + (0,)
    L = l.astype(LD)
    lpd = logsumexp(L) - np.log(LD(S))
    mean = L.sum() / LD(S)
    p_waic = ((L - mean) ** 2).sum() / LD(S - 1)
    r = np.sort(-l)
    x = r - r[-1]                                            # in double: the ratios are what the doubles say
    M = tail_len(S)
    lc = max(x[S - M - 1], math.log(np.finfo(np.float64).tiny))
    n = int(np.count_nonzero(x > lc))
    assert np.all(x[S - n:] > lc) and n <= M
    lw = x.astype(LD)
    k = math.inf
    if n > 4:
        elc = np.exp(LD(lc))
        t = np.exp(x[S - n:].astype(LD)) - elc
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
            lw[S - n:] = np.where(v > 0, LD(0), v)
    elpd_loo = logsumexp((-r).astype(LD) + lw) - logsumexp(lw)
    return float(lpd), float(p_waic), float(elpd_loo), k, n


def restate(x, first=0, count=None, thin=1, cols=None):
    """the whole contract in numpy -> dict of arrays [K]"""
    rows = [restate_column(c) for c in pooled(x, first, count, thin, cols)]
    out = {f: np.array([r[i] for r in rows]) for i, f in enumerate(FIELDS)}
    out["tail_n"] = out["tail_n"].astype(np.int32)
    return out


def same_bits(a, b):
    """NaN matches NaN, -0.0 does not match +0.0"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)))


def same_results(a, b, cols=None):
    """entry k of a has the bits of entry cols[k] of b"""
    ix = slice(None) if cols is None else list(cols)
    return all(same_bits(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64)[ix]) for f in FIELDS)


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// loo_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter) and the kernels' index arithmetic, one
// workgroup after the other.  sorted_out [K][S] (the keys the column kernel reads) may be NULL.  Returns the number of chunks, -1 beyond
// the cap, -2 beyond the tail's LDS.
extern "C" int ll_emulate(const double *ll, int chains, long long iterations, long long nvars, long long first, long long count, long long thin, const int *cols,
                          int K, long long cap, double *lpd, double *p_waic, double *elpd_loo, double *pareto_k, int *tail_n, rs_key *sorted_out) {
  const rh_plan::Loo P = rh_plan::loo_plan(chains, count, thin, K, cap);
  if (P.over_cap) return -1;
  if (P.over_lds) return -2;
  const long long S = P.S;
  std::vector<rs_key> ka((size_t)(P.pc * S)), kb((size_t)(P.pc * S)), klds(RS_TILE_SLOTS > RS_MERGE_LDS ? RS_TILE_SLOTS : RS_MERGE_LDS);
  std::vector<double> lds(LL_LDS_DOUBLES);
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0;
    rs_key *src = ka.data(), *dst = kb.data();
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
      const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE;
      if (g0 >= S) continue;
      rs_tile_sort(ll + first * nvars + cols[k0 + pl], iterations, nvars, thin, P.kept, S, g0, klds.data(), src + pl * S + g0, LL_BLOCK);
    }
    for (int k = 0; k < P.passes; k++) {
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
        if (o0 >= S) continue;
        rs_merge_tile(src + pl * S, dst + pl * S, S, P.run(k), o0, klds.data(), LL_BLOCK);
      }
      std::swap(src, dst);
    }
    for (long long pl = 0; pl < p_cnt; pl++) {
      const long long k = k0 + pl;
      ll_column_block(src + pl * S, S, P.M, lds.data(), lpd + k, p_waic + k, elpd_loo + k, pareto_k + k, tail_n + k, LL_BLOCK);
      if (sorted_out) for (long long s = 0; s < S; s++) sorted_out[k * S + s] = src[pl * S + s];
    }
  }
  return chunks;
}
// kept, S, M, cut, per_col, pc, over_cap, over_lds, tiles, mtiles, passes
extern "C" void ll_plan(long long chains, long long count, long long thin, long long K, long long cap, long long *out) {
  const rh_plan::Loo P = cap ? rh_plan::loo_plan(chains, count, thin, K, cap) : rh_plan::loo_plan(chains, count, thin, K);
  const long long v[11] = {P.kept, P.S, P.M, P.cut, P.per_col, P.pc, P.over_cap ? 1 : 0, P.over_lds ? 1 : 0, P.tiles, P.mtiles, P.passes};
  for (int i = 0; i < 11; i++) out[i] = v[i];
}
extern "C" void ll_fn_many(int which, const double *x, long long n, double *out) {
  for (long long i = 0; i < n; i++) out[i] = which == 0 ? ll_exp(x[i]) : which == 1 ? ll_log(x[i]) : which == 2 ? ll_log1p(x[i]) : ll_expm1(x[i]);
}
extern "C" void ll_constants(long long *out) { const long long v[5] = {LL_BLOCK, LL_TAIL_MAX, LL_LDS_DOUBLES, LL_MAX_CAND, LL_WS_CAP_BYTES}; for (int i = 0; i < 5; i++) out[i] = v[i]; }
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h and rh_loo.hip.h in host mode) + the driver above as a host shared library
    (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_loo_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int)
        L.ll_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, ll, dp, dp, dp, dp, ip, C.POINTER(C.c_ulonglong)]
        L.ll_plan.argtypes = [ll, ll, ll, ll, ll, C.POINTER(ll)]
        L.ll_plan.restype = None
        L.ll_fn_many.argtypes = [C.c_int, dp, ll, dp]
        L.ll_constants.argtypes = [C.POINTER(ll)]
        _emu = L
    return _emu


PLAN_FIELDS = ("kept", "S", "M", "cut", "per_col", "pc", "over_cap", "over_lds", "tiles", "mtiles", "passes")


def plan(chains, count, thin, k, cap=0):
    out = (C.c_longlong * 11)()
    emulation().ll_plan(chains, count, thin, k, cap, out)
    return dict(zip(PLAN_FIELDS, list(out)))


def emulate(x, first=0, count=None, thin=1, cols=None, cap=CAP, dump=False):
    """the host emulation over x [chains][iterations][nvars] -> dict of the five outputs [K], "chunks", and with dump "sorted" [K][S]
    (the ascending column as doubles)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    k = len(sel)
    p = plan(m, count, thin, k, cap)
    out = {f: np.full(k, -1.0) for f in FIELDS[:4]}
    out["tail_n"] = np.full(k, -1, dtype=np.int32)
    keys = np.zeros((k, p["S"]), dtype=np.uint64) if dump else None
    n = L.ll_emulate(_capi.dptr(x), m, iters, nv, first, count, thin, sel.ctypes.data_as(C.POINTER(C.c_int)), k, cap, *[_capi.dptr(out[f]) for f in FIELDS[:4]],
                     out["tail_n"].ctypes.data_as(C.POINTER(C.c_int)), keys.ctypes.data_as(C.POINTER(C.c_ulonglong)) if dump else None)
    assert n >= 1, "refused"
    out["chunks"] = n
    if dump:
        out["keys"], out["sorted"] = keys, from_keys(keys)
    return out


_cases = {}


def emulated_case(i, bad=np.nan):
    """(x, first, count, thin, the emulation's result with its sorted columns) of shape i, computed once and shared (the GPU tests
    compare with it)"""
    key = (i, "nan" if np.isnan(bad) else "inf")
    if key not in _cases:
        x, first, count, thin = case(i, bad)
        _cases[key] = (x, first, count, thin, emulate(x, first, count, thin, dump=True))
    return _cases[key]


def shuffled_with_duplicate(k, seed):
    rng = np.random.default_rng(seed)
    pick = list(rng.permutation(k)[:max(1, (2 * k) // 3)])
    return [int(c) for c in pick + pick[:1]]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_loo_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.loo_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r   # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.loo.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.loo_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_other_sources_do_not_carry_the_loo_kernels():
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_loo" not in src and b"rh_loo" not in _capi.summary_lower_only("gfx950") and b"rh_loo" not in _capi.rank_lower_only("gfx950")


def test_exports_and_python_surface():
    import inspect
    import rainier_amd as R
    L = _capi.lib()
    for name in ("rh_loo_device", "rh_sampler_loo", "rh_loo_lower_only"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert R.Loo._fields == ("lpd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "pareto_k", "tail_n", "cols")
    assert list(inspect.signature(R.Sampler.loo).parameters) == ["self", "predictor", "first", "count", "thin", "cols"]
    assert list(inspect.signature(R.loo_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "thin", "cols"]
    assert list(inspect.signature(R.loo_compare).parameters) == ["a", "b"]
    sig = inspect.signature(R.Sampler.loo).parameters
    assert sig["first"].default == 0 and sig["count"].default is None and sig["thin"].default == 1 and sig["cols"].default is None
    # the totals, their standard errors and the comparison are a few lines on the host
    rng = np.random.default_rng(5)
    lpd, pw, el = rng.standard_normal(7) - 3.0, rng.random(7), rng.standard_normal(7) - 3.5
    a = R.Loo(lpd, pw, lpd - pw, el, lpd - el, np.zeros(7), np.zeros(7, dtype=np.int32), tuple(range(7)))
    b = a._replace(elpd_loo=el - rng.random(7))
    se = lambda v: math.sqrt(7 * np.var(v, ddof=1))
    assert a.loo() == (float(el.sum()), se(el)) and a.waic() == (float((lpd - pw).sum()), se(lpd - pw))
    assert a.p_loo_total() == (float((lpd - el).sum()), se(lpd - el)) and a.p_waic_total() == (float(pw.sum()), se(pw))
    d = a.elpd_loo - b.elpd_loo
    assert R.loo_compare(a, b) == (float(d.sum()), se(d)) and R.loo_compare(a, b)[0] > 0.0 and R.loo_compare(a, a) == (0.0, 0.0)
    from rainier_amd import models
    assert models.eight_schools_loglik()[1] == 8 and models.linreg_loglik(2, [[0.0, 1.0], [1.0, 2.0], [3.0, 1.0]], [1.0, 2.0, 0.5])[1] == 3


# ---- 2. the device text, on the host -------------------------------------------------------------------------------------------------
def fn_many(which, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    got = np.empty_like(x)
    emulation().ll_fn_many(which, _capi.dptr(x), len(x), _capi.dptr(got))
    return got


def test_transcendentals_against_numpy():
    rng = np.random.default_rng(9)
    tiny = np.finfo(np.float64).tiny
    grids = {
        0: np.concatenate([np.linspace(-708.0, 709.0, 200001), -np.exp(rng.uniform(-40.0, 6.5, 100000)), [0.0, -0.0, 1e-300, -1e-300]]),
        1: np.concatenate([np.exp(rng.uniform(-700.0, 700.0, 200000)), np.linspace(0.5, 2.0, 100001), [tiny, 1.0, float(2 ** 20), 20000.0]]),
        2: np.concatenate([-np.exp(rng.uniform(-45.0, 0.0, 200000)) * 0.999999, (np.arange(1, 8065) - 0.5) / -8064.0, np.exp(rng.uniform(-45.0, 5.0, 50000))]),
        3: np.concatenate([rng.uniform(-40.0, 40.0, 100000), np.exp(rng.uniform(-45.0, 3.0, 100000)), -np.exp(rng.uniform(-45.0, 3.0, 100000))]),
    }
    refs = {0: np.exp, 1: np.log, 2: np.log1p, 3: np.expm1}
    measured = {0: EXP_MEASURED, 1: LOG_MEASURED, 2: LOG1P_MEASURED, 3: EXPM1_MEASURED}
    for which, x in grids.items():
        got, want = fn_many(which, x), refs[which](x.astype(LD))
        ok = want != 0
        worst = float(np.max(np.abs((got[ok].astype(LD) - want[ok]) / want[ok])))
        print("function %d: largest relative difference from numpy's longdouble: %.3g" % (which, worst))
        assert np.array_equal(got[~ok], want[~ok].astype(np.float64))
        assert worst <= measured[which], (which, worst)          # the figure in the README is what is measured
        assert 4 * measured[which] <= 2e-15                        # the bound: four times it, capped
    # the edges the contract names
    with np.errstate(all="ignore"):
        assert np.array_equal(fn_many(0, [-np.inf, np.inf, -746.0, 710.0]), [0.0, np.inf, 0.0, np.inf]) and np.isnan(fn_many(0, [np.nan])[0])
        assert np.array_equal(fn_many(1, [0.0, np.inf, 1.0]), [-np.inf, np.inf, 0.0]) and np.isnan(fn_many(1, [-1.0])[0])
        assert np.array_equal(fn_many(2, [-1.0, 0.0, 1e-300, np.inf]), [-np.inf, 0.0, 1e-300, np.inf]) and np.isnan(fn_many(2, [-1.5])[0])
        assert np.array_equal(fn_many(3, [-np.inf, 0.0, 1e-300, np.inf, -800.0]), [-1.0, 0.0, 1e-300, np.inf, -1.0])
    assert fn_many(1, [tiny])[0] == math.log(tiny)


def waic_bounds(l):
    """(lpd, its bound, p_waic, its bound) of one finite column in longdouble, as derived in the module's docstring"""
    S = l.size
    L = l.astype(LD)
    top = L.max()
    logsum = np.log(np.exp(L - top).sum())
    lpd = top + logsum - np.log(LD(S))
    b_lpd = U53 * (S + 4 + float(np.max(np.abs(L - top))) + 4.0 * (abs(float(top)) + abs(float(logsum)) + math.log(S)))
    mean = L.sum() / LD(S)
    ssq = ((L - mean) ** 2).sum()
    d = (S + 2) * U53 * float(np.abs(L).sum()) / S
    return float(lpd), b_lpd, float(ssq / LD(S - 1)), float(((S + 6) * U53 * ssq + 2 * S * d * d) / (S - 1))


def rel(got, want, floor=0.0):
    return abs(got - want) / max(abs(want), floor)


@pytest.mark.parametrize("bad", [np.nan, -np.inf])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_figures_against_the_longdouble_restatement(i, bad):
    x, first, count, thin, emu = emulated_case(i, bad)
    cols = pooled(x, first, count, thin)
    S = cols.shape[1]
    assert S == SHAPES[i][0] * -(-count // thin) == emu["sorted"].shape[1]
    worst = 0.0
    for k in range(x.shape[2]):
        # the sorted column is the column in key order
        assert np.array_equal(emu["keys"][k], np.sort(to_keys(cols[k]))), (SHAPES[i], k)
        got = [emu[f][k] for f in FIELDS]
        if k % NKINDS == 5:
            assert all(np.isnan(g) for g in got[:4]) and got[4] == 0, (SHAPES[i], k)
            continue
        lpd, b_lpd, pw, b_pw = waic_bounds(cols[k])
        assert abs(got[0] - lpd) <= b_lpd and abs(got[1] - pw) <= b_pw, (SHAPES[i], k, got, lpd, b_lpd, pw, b_pw)
        want = restate_column(emu["sorted"][k])
        assert got[4] == want[4] and got[4] <= tail_len(S), (SHAPES[i], k, got, want)          # tail_n: exact
        assert math.isinf(got[3]) == math.isinf(want[3]) and (got[4] > 4 or math.isinf(got[3])), (SHAPES[i], k, got, want)
        assert rel(got[2], want[2]) <= 4 * LOO_MEASURED, (SHAPES[i], k, got, want)
        worst = max(worst, rel(got[2], want[2]))
        if not math.isinf(want[3]):
            assert rel(got[3], want[3], 1.0) <= 4 * LOO_MEASURED, (SHAPES[i], k, got, want)
            worst = max(worst, rel(got[3], want[3], 1.0))
        # the restatement does not care whether it is handed the column or the sorted column
        again = restate_column(cols[k])
        assert again[3:] == want[3:] and rel(again[2], want[2]) <= 1e-15
        if k % NKINDS == 4:                                   # the constant column
            assert got[0] == -2.0 and got[1] == 0.0 and got[2] == -2.0 and got[3] == math.inf and got[4] == 0
        assert got[1] >= 0.0 and got[2] <= got[0] + 4 * LOO_MEASURED * abs(got[0])      # leaving an observation out cannot help predicting it
    print("largest relative difference of elpd_loo / pareto_k from the restatement: %.3g" % worst)
    assert worst <= LOO_MEASURED


def test_the_k_infinity_boundary_and_what_k_says():
    # S = 20: M = 4, so n <= 4 and nothing is smoothed; S = 21: M = 5, and the columns without ties have n = 5
    for i, S, n in ((2, 20, 4), (3, 21, 5)):
        x, first, count, thin, emu = emulated_case(i)
        assert plan(SHAPES[i][0], count, thin, 1)["S"] == S and tail_len(S) == n
        for k in (0, 1):
            assert emu["tail_n"][k] == n and math.isinf(emu["pareto_k"][k]) == (n == 4), (S, k, emu["tail_n"][k], emu["pareto_k"][k])
    x, first, count, thin, emu = emulated_case(len(SHAPES) - 1)     # S = 20000
    print("k of the kinds at S = 20000:", emu["pareto_k"][:6])
    assert 0.0 < emu["pareto_k"][0] < 0.5 and emu["pareto_k"][1] > 0.7
    assert emu["tail_n"][0] == tail_len(20000) == 425 and emu["tail_n"][2] <= 425


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_properties_of_the_contract(i):
    x, first, count, thin, emu = emulated_case(i)
    chains = SHAPES[i][0]
    nv = x.shape[2]
    # a second call gives the same bits
    assert same_results(emulate(x, first, count, thin), emu), SHAPES[i]
    # a window gives the bits of its copy (thinned on the host)
    assert same_results(emulate(np.ascontiguousarray(x[:, first:first + count:thin, :])), emu), SHAPES[i]
    # a shuffled column list with a duplicate gives the bits of the full call's entries
    cols = shuffled_with_duplicate(nv, i)
    assert same_results(emulate(x, first, count, thin, cols=cols), emu, cols), SHAPES[i]
    # forcing several chunks gives the same bits
    p = plan(chains, count, thin, nv)
    small = emulate(x, first, count, thin, cap=2 * p["per_col"])
    assert small["chunks"] == -(-nv // 2) and emu["chunks"] == 1 and same_results(small, emu), SHAPES[i]


def test_nan_and_inf_columns_are_nan_and_touch_nothing_else():
    x, first, count, thin = case(5)                         # 5 chains, count 819, 13 columns; column 5 and 11 hold a NaN already
    clean = emulate(x, first, count, thin)
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[0, first - 1, 1] = np.nan                           # outside the window
    bad[1, first + count, 2] = np.inf                       # outside the window
    got = emulate(bad, first, count, thin)
    for k in range(x.shape[2]):
        if k in (0, 6, 9, 5, 11):
            assert all(np.isnan(got[f][k]) for f in FIELDS[:4]) and got["tail_n"][k] == 0, k
        else:
            assert all(same_bits(got[f][k], clean[f][k]) for f in FIELDS), k
            assert np.isfinite(got["lpd"][k]) and np.isfinite(got["elpd_loo"][k])
    # thinning steps over a bad value
    x2, first, count, thin = case(8)                        # thin 2
    assert thin == 2
    x2[0, first + 1, 0] = np.nan
    x2[1, first + 3, 1] = -np.inf
    assert same_results(emulate(x2, first, count, thin), emulated_case(8)[4])


def test_the_plan_is_arithmetic_over_the_headers_constants():
    consts = (C.c_longlong * 5)()
    emulation().ll_constants(consts)
    assert list(consts) == [256, TAIL_MAX, TAIL_MAX + 768, 30 + int(math.sqrt(TAIL_MAX)), CAP]
    # M and the cutoff's order statistic x_(S - M)
    for S, M in ((2, 1), (20, 4), (21, 5), (25, 5), (4096, 192), (7200000, 8050)):
        p = plan(1, S, 1, 1)
        assert (p["S"], p["M"], p["cut"]) == (S, M, S - M) and M == tail_len(S) and 1 <= M < S, (S, p)
    for chains, count, thin, k in ((1, 2, 1, 1), (4, 5, 1, 6), (2, 8194, 2, 6), (16, 1250, 1, 13), (1024, 200, 1, 434), (64, 2000, 1, 70), (3, 100, 7, 5)):
        kept = -(-count // thin)
        S = chains * kept
        tiles, passes = -(-S // TILE), 0
        while TILE << passes < S:
            passes += 1
        want = dict(kept=kept, S=S, M=tail_len(S), cut=S - tail_len(S), per_col=16 * S, pc=max(1, min(CAP // (16 * S), k)), over_cap=0, over_lds=0, tiles=tiles,
                    mtiles=-(-S // MERGE_TILE), passes=passes)
        assert plan(chains, count, thin, k) == want, (chains, count, thin, k)
    # KidIQ's matrix: 434 columns of 204 800 values, 40 to a chunk; the GPU tier's buffer that crosses the cap: 70 columns of 128 000, 65 + 5
    assert plan(1024, 200, 1, 434)["pc"] == 40 and plan(64, 2000, 1, 70)["pc"] == 65
    # refused from the shape alone: M beyond the tail's LDS (S above about 7.2 million), one column beyond the cap
    assert plan(1, 7225344, 1, 1)["over_lds"] == 0 and plan(1, 7225345, 1, 1)["over_lds"] == 1 and plan(1, 7225345, 1, 1)["over_cap"] == 0
    assert plan(1, 1 << 23, 1, 1)["over_cap"] == 0 and plan(1, (1 << 23) + 1, 1, 1)["over_cap"] == 1 and plan(1, (1 << 23) + 1, 1, 1)["pc"] == 1
    x = fixture(2, 40, 3, 1)
    sel = (C.c_int * 3)(0, 1, 2)
    assert emulation().ll_emulate(_capi.dptr(x), 2, 40, 3, 0, 40, 1, sel, 3, plan(2, 40, 1, 3)["per_col"] - 1, *[None] * 6) == -1


# ---- 3. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    outs = [np.zeros(8) for _ in range(4)]
    tn = np.zeros(8, dtype=np.int32)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, thin=1, cols=None, ncols=None, null=None):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        nc = (len(sel) if sel is not None else 0) if ncols is None else ncols
        o = [_capi.dptr(a) for a in outs] + [tn.ctypes.data_as(ip)]
        if null is not None:
            o[null] = None
        return L.rh_loo_device(ptr, 0, chains, iters, nvars, first, count, thin, sel.ctypes.data_as(ip) if sel is not None else None, nc, *o)
    err = lambda: L.rh_last_error(None).decode()
    assert call(ptr=None) == _capi.RH_E_INVALID
    for null in range(5):
        assert call(null=null) == _capi.RH_E_INVALID and "NULL" in err()
    for first, count, thin in ((0, 0, 1), (0, 11, 1), (7, 4, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):
        assert call(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
        assert "window" in err()
    assert call(nvars=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    # S < 2: one chain, one kept draw
    assert call(chains=1, count=1) == _capi.RH_E_INVALID and "at least 2" in err()
    assert call(chains=1, count=10, thin=10) == _capi.RH_E_INVALID and "at least 2" in err()
    for cols in ([2], [-1], [0, 1, 7]):
        assert call(cols=cols) == _capi.RH_E_INVALID and "outside" in err(), cols
    assert call(cols=[0], ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(cols=[0], ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=1) == _capi.RH_E_INVALID and "ncols" in err()            # no list: 0 or nvars
    o = [_capi.dptr(a) for a in outs] + [tn.ctypes.data_as(ip)]
    assert L.rh_sampler_loo(None, None, 0, 10, 1, None, 0, *o) == _capi.RH_E_INVALID
    # one column beyond the workspace cap, and one whose tail is beyond the LDS: refused from the shape, whatever the machine
    assert call(chains=4097, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    assert call(chains=3600, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "LDS" in err()
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(ncols=2) == _capi.RH_E_DEVICE and call(cols=[1, 1, 0]) == _capi.RH_E_DEVICE and call(chains=1, count=2) == _capi.RH_E_DEVICE
        assert call(thin=3) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.loo_device(4096, 4, 10, 4)


# ---- 4. what the figures mean --------------------------------------------------------------------------------------------------------
def conjugate(seed=2017, n=10, chains=16, kept=1250):
    """y_i ~ N(theta, 1), i = 1 .. n, a flat prior: theta | y ~ N(ybar, 1 / n), drawn exactly.  -> (ll [chains][kept][n], the analytic
    log leave-one-out densities log N(y_i | ybar_-i, 1 + 1 / (n - 1)))"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n) + 0.7
    theta = y.mean() + rng.standard_normal((chains, kept)) / math.sqrt(n)
    ll = -0.5 * math.log(2.0 * math.pi) - 0.5 * (y[None, None, :] - theta[:, :, None]) ** 2
    others = (y.sum() - y) / (n - 1)
    var = 1.0 + 1.0 / (n - 1)
    return np.ascontiguousarray(ll), -0.5 * math.log(2.0 * math.pi * var) - 0.5 * (y - others) ** 2 / var


def test_conjugate_normal_model_against_the_analytic_leave_one_out_density():
    ll, exact = conjugate()
    emu, ref = emulate(ll), restate(ll)
    for f in FIELDS[:4]:
        assert np.all(np.abs(emu[f] - ref[f]) <= 1e-9 * np.maximum(1.0, np.abs(ref[f]))), f
    assert np.array_equal(emu["tail_n"], ref["tail_n"])
    d_loo, d_waic, k = np.max(np.abs(emu["elpd_loo"] - exact)), np.max(np.abs(emu["lpd"] - emu["p_waic"] - exact)), np.max(emu["pareto_k"])
    print("conjugate fixture: max |elpd_loo - exact| %.4f, max |elpd_waic - exact| %.4f, max k %.3f" % (d_loo, d_waic, k))
    assert d_loo <= CONJ_LOO_MEASURED and d_waic <= CONJ_WAIC_MEASURED and k <= CONJ_K_MEASURED      # the README's figures are what is measured
    assert d_loo <= 2 * CONJ_LOO_MEASURED and d_waic <= 2 * CONJ_WAIC_MEASURED and k < 0.7             # the bound: twice them
    assert np.all(emu["lpd"] > emu["elpd_loo"]) and np.all(emu["p_waic"] > 0.0) and np.all(emu["tail_n"] == tail_len(20000))
