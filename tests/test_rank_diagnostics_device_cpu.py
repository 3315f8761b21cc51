"""Rank-normalised split R-hat, bulk ESS and tail ESS on the device (csrc/device/rh_rank.hip.h; Vehtari, Gelman, Simpson, Carpenter,
Buerkner 2021), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) -- the emulation -- and
    compared
      - ranks: equal to numpy's searchsorted (left and right) on the uint64 keys;
      - rk_ndtri: with scipy.special.ndtri at four times the largest difference measured here (1.8e-15), capped at 1e-14 absolute;
      - m_q and g_q(t) of every series: with np.longdouble sums of the products of the values centred with the RETURNED mean, at
        bounds that are derived, not tuned: with u = 2^-53,
            |m_q - sum / h|  <= (h + 2) u sum|u_i| / h                       (h - 1 adds in any order, the division)
            |g_q(t) - ref|   <= (h + 4) u sum_i |d_i d_{i+t}| / h            (the centring's rounding in either factor, the product,
                                                                              at most h - 1 adds, the division)
      - the four figures and the flags: with a longdouble restatement of the estimator fed with the emulation's own series, whose
        every comparison is first shown to be decided by more than 1e-6;
  * the properties of the contract (a shuffled column list with a duplicate, chunking, a window and its copy, NaN / inf / constant
    columns), the plan's arithmetic, the C ABI's argument errors and its refusal to compute without a device;
  * what the figures mean, on fixtures with fixed seeds: AR(1), a trend that all chains share (which the reference's R-hat cannot
    see), a chain of another scale, Cauchy draws.

tests/test_gpu_rank_diagnostics_device.py runs the same shapes through the kernels.
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
KERNELS = ("rh_rank_stage_kernel", "rh_rank_fold_kernel", "rh_rank_sort_kernel", "rh_rank_merge_kernel", "rh_rank_normal_kernel",
           "rh_rank_indicator_kernel", "rh_rank_chain_kernel", "rh_rank_finish_kernel", "rh_rank_combine_kernel")
CAP, MAXLAG, TILE, MERGE_TILE = 128 << 20, 255, 4096, 2048
U53 = 2.0 ** -53
LD = np.longdouble
# the largest |rk_ndtri - scipy.special.ndtri| measured over the grids of test_rk_ndtri_against_scipy (profiles/rank_diagnostics_device)
NDTRI_MEASURED = 1.8e-15
# the largest relative difference of a figure from the longdouble restatement measured over SHAPES (profiles/rank_diagnostics_device)
FIGURE_MEASURED = 1.1e-13


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
NKINDS = 6
# (chains, count): h = 2, 4, 255, 256, 257 (L at and around the cap); S below, at and above one sort tile, two merge passes;
# h = 8064 resident, 8065 tiled with a halo, an odd count across that boundary
SHAPES = ((1, 4), (2, 9), (3, 511), (3, 513), (3, 515), (5, 819), (4, 1024), (1, 4098), (1, 8194), (1, 16128), (1, 16130), (1, 16131))
NVARS = (1, 5, 17)


def fixture(chains, iters, nvars, seed):
    """[chains][iters][nvars]; column p is of kind p % 6: 0 iid normal, 1 AR(0.9), 2 moved by 1e6 with chain 0 scaled by 3, 3 rounded
    to integers (ties), 4 the constant 2.0, 5 standard Cauchy"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((chains, iters, nvars))
    for p in range(nvars):
        kind = p % NKINDS
        if kind == 1:
            for i in range(1, iters):
                x[:, i, p] = 0.9 * x[:, i - 1, p] + math.sqrt(1.0 - 0.81) * x[:, i, p]
        elif kind == 2:
            x[0, :, p] *= 3.0
            x[:, :, p] += 1e6
        elif kind == 3:
            x[:, :, p] = np.round(2.0 * x[:, :, p])
        elif kind == 4:
            x[:, :, p] = 2.0
        elif kind == 5:
            x[:, :, p] = rng.standard_cauchy((chains, iters))
    return x


def case(i):
    """shape i of SHAPES -> (x, first, count): nvars cycles through NVARS, the window starts late and ends early in a longer buffer"""
    chains, count = SHAPES[i]
    first = 1 + i % 3
    return fixture(chains, first + count + 2, NVARS[i % 3], 100 + i), first, count


def split(x, first=0, count=None, cols=None):
    """y [K][M][h]: sequence 2c is (c, first + i), 2c + 1 is (c, first + count - h + i)"""
    count = x.shape[1] - first if count is None else count
    h = count // 2
    sel = range(x.shape[2]) if cols is None else cols
    w = x[:, first:first + count, :]
    halves = np.stack([w[:, :h, :], w[:, count - h:, :]], axis=1)            # [chains][2][h][nvars]
    return np.ascontiguousarray(np.stack([halves[:, :, :, p].reshape(-1, h) for p in sel]))


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
def to_keys(v):
    """Double.compare's order as uint64: negatives with all bits flipped, the others with the sign bit; every NaN the positive quiet one"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
    b[(b & np.uint64(0x7fffffffffffffff)) > np.uint64(0x7ff0000000000000)] = np.uint64(0x7ff8000000000000)
    return np.where((b >> np.uint64(63)) == 1, ~b, b ^ np.uint64(0x8000000000000000))


def rank2_of(v):
    """L + U + 1 (twice the average rank) of every value among all of v, in key order"""
    k = to_keys(v.ravel())
    s = np.sort(k)
    return (np.searchsorted(s, k, "left") + np.searchsorted(s, k, "right") + 1).reshape(v.shape)


def z_of(v):
    from scipy.special import ndtri
    return ndtri((rank2_of(v) * 0.5 - 0.375) / (v.size + 0.25))


def series_of(y):
    """y [M][h] -> the four series [4][M][h]: bulk, folded, lower-tail indicator, upper-tail indicator"""
    S = y.size
    k = to_keys(y.ravel())
    order = np.argsort(k, kind="stable")
    sv, sk = y.ravel()[order], k[order]
    med = 0.5 * sv[S // 2 - 1] + 0.5 * sv[S // 2]
    with np.errstate(invalid="ignore"):
        folded = np.abs(y - med)
    ind = lambda q: (to_keys(y) <= sk[min(S - 1, int(math.floor(S * q)))]).astype(np.float64)
    return np.stack([z_of(y), z_of(folded), ind(0.05), ind(0.95)])


def estimator(u, lags=True, dtype=np.float64, mean=None):
    """The contract's estimator on u [M][h] in `dtype`: (rhat, ess, truncated, stopped at pair k or None, the smallest margin by which
    a comparison of the scan was decided, m [M], g [L + 1][M]).  mean: the m_q to centre with (None: u's own)"""
    M, h = u.shape
    S = M * h
    L = min(h - 1, MAXLAG) if lags else 0
    u = u.astype(dtype)
    m = u.sum(axis=1) / dtype(h) if mean is None else np.asarray(mean).astype(dtype)
    d = u - m[:, None]
    g = np.stack([(d[:, :h - t] * d[:, t:]).sum(axis=1) / dtype(h) for t in range(L + 1)])
    gm = g.sum(axis=1) / dtype(M)
    W = gm[0] * dtype(h) / dtype(h - 1)
    B = ((m - m.sum() / dtype(M)) ** 2).sum() / dtype(M - 1)
    V = dtype(h - 1) / dtype(h) * W + B
    nan = float("nan")
    if not W > 0:
        return nan, nan, 0, None, math.inf, m, g
    rhat = float(np.sqrt(V / W))
    if L == 0:
        return rhat, nan, 0, None, math.inf, m, g
    rho = dtype(1) - (W - gm) / V
    rho[0] = dtype(1)
    tau, prev, stop, margin = dtype(-1), dtype(np.inf), None, math.inf
    for k in range((L - 1) // 2 + 1):
        P = rho[2 * k] + rho[2 * k + 1]
        margin = min(margin, abs(float(P)))
        if not P > 0:
            tau += max(rho[2 * k], dtype(0))
            stop = k
            break
        if np.isfinite(prev):
            margin = min(margin, abs(float(P - prev)))
        P = min(P, prev)
        prev = P
        tau += 2 * P
    tau_min = dtype(1) / np.log10(dtype(S))
    margin = min(margin, abs(float(tau - tau_min)))
    tau = max(tau, tau_min)
    return rhat, float(dtype(S) / tau), 0 if stop is not None else 1, stop, margin, m, g


def restate(x, first=0, count=None, cols=None):
    """the whole contract in numpy and scipy -> dict of arrays [K]"""
    y = split(x, first, count, cols)
    out = {k: [] for k in ("rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "truncated")}
    for yk in y:
        if not np.all(np.isfinite(yk)):
            for k in out:
                out[k].append(0 if k == "truncated" else float("nan"))
            continue
        s = series_of(yk)
        bulk, fold, lo, hi = estimator(s[0]), estimator(s[1], lags=False), estimator(s[2]), estimator(s[3])
        out["rhat_bulk"].append(bulk[0])
        out["rhat_folded"].append(fold[0])
        out["ess_bulk"].append(bulk[1])
        out["ess_tail"].append(float("nan") if math.isnan(lo[1]) or math.isnan(hi[1]) else min(lo[1], hi[1]))
        out["truncated"].append(bulk[2] | lo[2] << 1 | hi[2] << 2)
    res = {k: np.array(v) for k, v in out.items()}
    with np.errstate(invalid="ignore"):
        res["rhat"] = np.where(np.isnan(res["rhat_bulk"]) | np.isnan(res["rhat_folded"]), np.nan, np.maximum(res["rhat_bulk"], res["rhat_folded"]))
    return res


def same_bits(a, b):
    """NaN matches NaN, -0.0 does not match +0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)))


FIELDS = ("rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "truncated")


def same_results(a, b, cols=None):
    """entry k of a has the bits of entry cols[k] of b"""
    ix = slice(None) if cols is None else list(cols)
    return all(same_bits(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64)[ix]) for f in FIELDS)


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// the values of v [p_cnt][S] sorted, as rank_run's sorted_of launches it: tile sorts, then merge passes between the two key buffers
static const rs_key *emu_sorted_of(const double *v, const rh_plan::Rank &P, long long p_cnt, std::vector<rs_key> &ka, std::vector<rs_key> &kb, rs_key *lds) {
  rs_key *src = ka.data(), *dst = kb.data();
  for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
    const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE;
    if (g0 >= P.S) continue;
    rs_tile_sort(v + pl * P.S, P.S, 1, 1, P.S, P.S, g0, lds, src + pl * P.S + g0, RK_BLOCK);
  }
  for (int k = 0; k < P.passes; k++) {
    for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
      const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
      if (o0 >= P.S) continue;
      rs_merge_tile(src + pl * P.S, dst + pl * P.S, P.S, P.run(k), o0, lds, RK_BLOCK);
    }
    std::swap(src, dst);
  }
  return src;
}
// rank_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter) and the kernels' index arithmetic, one
// workgroup after the other.  series_out [K][4][S], ws_out [K][4][M][sl], rank2_out [K][S] (twice the rank of y, through the routine
// the z-scores use) and fin_out [K][4][3] may be NULL.  Returns the number of chunks, -1 beyond the cap.
extern "C" int rk_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, const int *cols, int K,
                          long long cap, double *rhat_bulk, double *rhat_folded, double *ess_bulk, double *ess_tail, int *truncated, double *series_out,
                          double *ws_out, long long *rank2_out, double *fin_out) {
  const rh_plan::Rank P = rh_plan::rank_plan(chains, count, K, cap);
  if (P.over_cap) return -1;
  const long long S = P.S, M = P.M;
  const int h = (int)P.h;
  std::vector<double> y((size_t)(P.pc * S)), u((size_t)(P.pc * S)), ws((size_t)(P.pc * M * P.sl)), fin((size_t)K * RK_NSERIES * RK_NFIN), lds(RK_LDS_DOUBLES);
  std::vector<rs_key> ka((size_t)(P.pc * S)), kb((size_t)(P.pc * S)), klds(RS_TILE_SLOTS > RS_MERGE_LDS ? RS_TILE_SLOTS : RS_MERGE_LDS);
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0, ctiles = (p_cnt + RK_TP - 1) / RK_TP;
    auto series = [&](const rs_key *sorted, int L, int which) {
      for (long long bid = 0; bid < p_cnt * M; bid++) rk_chain_block(u.data() + bid * h, h, L, lds.data(), ws.data() + bid * P.sl, RK_BLOCK);
      for (long long pl = 0; pl < p_cnt; pl++) {
        rk_series_finish(ws.data() + pl * M * P.sl, sorted + pl * S, S, (int)M, h, L, P.sl, P.tau_min, lds.data(), fin.data() + ((k0 + pl) * RK_NSERIES + which) * RK_NFIN, RK_BLOCK);
        if (series_out) for (long long s = 0; s < S; s++) series_out[((k0 + pl) * RK_NSERIES + which) * S + s] = u[pl * S + s];
        if (ws_out)
          for (long long q = 0; q < M; q++)
            for (int e = 0; e < L + 2; e++) ws_out[(((k0 + pl) * RK_NSERIES + which) * M + q) * P.sl + e] = ws[(pl * M + q) * P.sl + e];
      }
    };
    for (long long bid = 0; bid < P.stiles * ctiles; bid++) {
      const long long rt = bid / ctiles, pl = (bid - rt * ctiles) * RK_TP, s0 = rt * RK_ROWS;
      if (s0 >= S || pl >= p_cnt) continue;
      rk_stage_tile(draws, iterations, nvars, first, count, P.h, S, cols + k0 + pl, (int)(p_cnt - pl < RK_TP ? p_cnt - pl : RK_TP), s0, lds.data(), y.data() + pl * S, RK_BLOCK);
    }
    const rs_key *sy = emu_sorted_of(y.data(), P, p_cnt, ka, kb, klds.data());
    for (long long pl = 0; pl < p_cnt; pl++)
      for (long long s = 0; s < S; s++) {
        u[pl * S + s] = rk_rank_z(sy + pl * S, S, y[pl * S + s]);
        if (rank2_out) rank2_out[(k0 + pl) * S + s] = rk_rank2(sy + pl * S, S, y[pl * S + s]);
      }
    series(sy, P.L, 0);
    for (int t = 0; t < 2; t++) {
      for (long long pl = 0; pl < p_cnt; pl++)
        for (long long s = 0; s < S; s++) u[pl * S + s] = rk_indicator(sy[pl * S + (t ? P.i95 : P.i05)], y[pl * S + s]);
      series(sy, P.L, 2 + t);
    }
    for (long long pl = 0; pl < p_cnt; pl++)
      for (long long s = 0; s < S; s++) u[pl * S + s] = rk_fold(y[pl * S + s], rk_median(sy + pl * S, S));
    const rs_key *sf = emu_sorted_of(u.data(), P, p_cnt, ka, kb, klds.data());
    for (long long pl = 0; pl < p_cnt; pl++)
      for (long long s = 0; s < S; s++) u[pl * S + s] = rk_rank_z(sf + pl * S, S, u[pl * S + s]);
    series(sf, 0, 1);
  }
  for (int k = 0; k < K; k++) rk_combine(fin.data() + (size_t)k * RK_NSERIES * RK_NFIN, rhat_bulk + k, rhat_folded + k, ess_bulk + k, ess_tail + k, truncated + k);
  if (fin_out) for (size_t i = 0; i < fin.size(); i++) fin_out[i] = fin[i];
  return chunks;
}
// h, M, S, L, sl, per_col, pc, over_cap, tiles, mtiles, passes, stiles, blocks, i05, i95
extern "C" double rk_plan(long long chains, long long count, long long K, long long cap, long long *out) {
  const rh_plan::Rank P = cap ? rh_plan::rank_plan(chains, count, K, cap) : rh_plan::rank_plan(chains, count, K);
  const long long v[15] = {P.h, P.M, P.S, P.L, P.sl, P.per_col, P.pc, P.over_cap ? 1 : 0, P.tiles, P.mtiles, P.passes, P.stiles, P.blocks, P.i05, P.i95};
  for (int i = 0; i < 15; i++) out[i] = v[i];
  return P.tau_min;
}
extern "C" void rk_ndtri_many(const double *p, long long n, double *out) { for (long long i = 0; i < n; i++) out[i] = rk_ndtri(p[i]); }
extern "C" void rk_log_many(const double *x, long long n, double *out) { for (long long i = 0; i < n; i++) out[i] = rk_log(x[i]); }
extern "C" void rk_constants(int *out) { const int v[6] = {RK_BLOCK, RK_MAXLAG, RK_SL, RK_LDS_DOUBLES, RK_TP, RK_ROWS}; for (int i = 0; i < 6; i++) out[i] = v[i]; }
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h and rh_rank.hip.h in host mode) + the driver above as a host shared library
    (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_rank_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int)
        L.rk_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ip, C.c_int, ll, dp, dp, dp, dp, ip, dp, dp, C.POINTER(ll), dp]
        L.rk_plan.argtypes = [ll, ll, ll, ll, C.POINTER(ll)]
        L.rk_plan.restype = C.c_double
        L.rk_ndtri_many.argtypes = [dp, ll, dp]
        L.rk_log_many.argtypes = [dp, ll, dp]
        _emu = L
    return _emu


PLAN_FIELDS = ("h", "M", "S", "L", "sl", "per_col", "pc", "over_cap", "tiles", "mtiles", "passes", "stiles", "blocks", "i05", "i95")


def plan(chains, count, k, cap=0):
    out = (C.c_longlong * 15)()
    tau_min = emulation().rk_plan(chains, count, k, cap, out)
    return dict(zip(PLAN_FIELDS, list(out)), tau_min=tau_min)


def emulate(x, first=0, count=None, cols=None, cap=CAP, dump=False):
    """the host emulation over x [chains][iterations][nvars] -> dict of the five outputs [K], "chunks", and with dump the series
    [K][4][M][h], ws [K][4][M][sl], rank2 [K][M][h] and fin [K][4][3]"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    k = len(sel)
    p = plan(m, count, k, cap)
    out = {f: np.full(k, -1.0) for f in FIELDS[:4]}
    out["truncated"] = np.full(k, -1, dtype=np.int32)
    dumps = {}
    if dump:
        dumps = dict(series=np.zeros((k, 4, p["M"], p["h"])), ws=np.zeros((k, 4, p["M"], p["sl"])), rank2=np.zeros((k, p["M"], p["h"]), dtype=np.int64),
                     fin=np.zeros((k, 4, 3)))
    dptr = lambda name: _capi.dptr(dumps[name]) if dump else None
    n = L.rk_emulate(_capi.dptr(x), m, iters, nv, first, count, sel.ctypes.data_as(C.POINTER(C.c_int)), k, cap, *[_capi.dptr(out[f]) for f in FIELDS[:4]],
                     out["truncated"].ctypes.data_as(C.POINTER(C.c_int)), dptr("series"), dptr("ws"),
                     dumps["rank2"].ctypes.data_as(C.POINTER(C.c_longlong)) if dump else None, dptr("fin"))
    assert n >= 1, "beyond the cap"
    out.update(dumps, chunks=n)
    with np.errstate(invalid="ignore"):
        out["rhat"] = np.where(np.isnan(out["rhat_bulk"]) | np.isnan(out["rhat_folded"]), np.nan, np.maximum(out["rhat_bulk"], out["rhat_folded"]))
    return out


_cases = {}


def emulated_case(i):
    """(x, first, count, the emulation's result with its dumps) of shape i, computed once and shared (the GPU tests compare with it)"""
    if i not in _cases:
        x, first, count = case(i)
        _cases[i] = (x, first, count, emulate(x, first, count, dump=True))
    return _cases[i]


def shuffled_with_duplicate(k, seed):
    rng = np.random.default_rng(seed)
    pick = list(rng.permutation(k)[:max(1, (2 * k) // 3)])
    return [int(c) for c in pick + pick[:1]]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_rank_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.rank_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r   # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.rank.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.rank_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_other_sources_do_not_carry_the_rank_kernels():
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_rank" not in src and b"rh_rank" not in _capi.summary_lower_only("gfx950")


def test_exports_and_python_surface():
    import inspect
    import rainier_amd as R
    L = _capi.lib()
    for name in ("rh_sampler_rank_diagnostics", "rh_rank_diagnostics_device", "rh_rank_lower_only"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert R.RankDiagnostics._fields == ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "truncated", "cols")
    assert list(inspect.signature(R.Sampler.rank_diagnostics).parameters) == ["self", "first", "count", "cols"]
    assert list(inspect.signature(R.rank_diagnostics_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "cols"]
    sig = inspect.signature(R.Sampler.rank_diagnostics).parameters
    assert sig["first"].default == 0 and sig["count"].default is None and sig["cols"].default is None


# ---- 2. the device text, on the host -------------------------------------------------------------------------------------------------
def test_rk_ndtri_against_scipy():
    from scipy.special import ndtri
    L = emulation()
    worst = 0.0
    grids = [(np.arange(1, 2 * S + 1) * 0.5 - 0.375) / (S + 0.25) for S in (4, 16, 4094, 4096, 4098, 8194)]     # every rank and half rank
    S = 204800
    r = np.concatenate([np.arange(1, 2001) * 0.5, np.arange(2 * S - 1999, 2 * S + 1) * 0.5, np.linspace(1.0, S, 20001), S * np.array([0.075, 0.925])])
    grids.append((r - 0.375) / (S + 0.25))
    grids = [np.ascontiguousarray(p) for p in grids]
    for p in grids:
        got = np.empty_like(p)
        L.rk_ndtri_many(_capi.dptr(p), len(p), _capi.dptr(got))
        worst = max(worst, float(np.max(np.abs(got - ndtri(p)))))
        if p is not grids[-1]:
            assert np.all(np.diff(got) > 0.0)             # the ranks in order: increasing across the branches' seams
    print("largest |rk_ndtri - scipy.special.ndtri|: %.3g" % worst)
    assert worst <= NDTRI_MEASURED, worst                  # the figure in the README is what is measured
    assert 4 * NDTRI_MEASURED <= 1e-14                      # the bound: four times it, capped
    # the three branches: the centre, the tails, the far tail
    p = np.array([0.5, 0.075, 0.925, 1e-9, 1e-12, 1.0 - 2.0 ** -40])
    got = np.empty_like(p)
    L.rk_ndtri_many(_capi.dptr(p), len(p), _capi.dptr(got))
    assert got[0] == 0.0 and np.all(np.abs(got - ndtri(p)) <= 4 * NDTRI_MEASURED * np.maximum(1.0, np.abs(got)))


def test_rk_log_is_within_an_ulp():
    L = emulation()
    x = np.concatenate([np.linspace(2.0 ** -40, 0.5, 100001), 2.0 ** -np.arange(1.0, 40.0), np.nextafter(1.0, 0.0) * 2.0 ** -np.arange(1.0, 40.0)])
    got = np.empty_like(x)
    L.rk_log_many(_capi.dptr(x), len(x), _capi.dptr(got))
    ref = np.log(x.astype(LD))
    assert np.all(np.abs(got.astype(LD) - ref) <= np.spacing(np.abs(got)))


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_ranks_equal_searchsorted_on_the_keys(i):
    x, first, count, emu = emulated_case(i)
    y = split(x, first, count)
    for k in range(y.shape[0]):
        assert np.array_equal(emu["rank2"][k], rank2_of(y[k])), (SHAPES[i], k)
        # the bulk series is rk_ndtri of those ranks, the indicators are the order statistics' in key order
        want = series_of(y[k])
        assert np.max(np.abs(emu["series"][k, 0] - want[0])) <= 4 * NDTRI_MEASURED * 8.0
        assert np.array_equal(emu["series"][k, 2], want[2]) and np.array_equal(emu["series"][k, 3], want[3])
        assert np.max(np.abs(emu["series"][k, 1] - want[1])) <= 4 * NDTRI_MEASURED * 8.0


def test_ranks_with_ties_signed_zeros_and_a_constant():
    x = np.zeros((2, 8, 3))
    x[:, :, 0] = [[0.0, -0.0, 1.0, 1.0, -0.0, 0.0, 1.0, -1.0], [-0.0, 0.0, 0.0, 2.0, 2.0, -1.0, -1.0, 5.0]]
    x[:, :, 1] = 7.0
    x[:, :, 2] = np.arange(16.0).reshape(2, 8)
    emu = emulate(x, dump=True)
    y = split(x)
    for k in range(3):
        assert np.array_equal(emu["rank2"][k], rank2_of(y[k]))
    # -0.0 ranks below +0.0: three of the one (ranks 4 .. 6) and four of the other (7 .. 10), above the three -1.0
    r = emu["rank2"][0].ravel() / 2.0
    v = y[0].ravel()
    assert set(r[(v == 0.0) & np.signbit(v)]) == {5.0} and set(r[(v == 0.0) & ~np.signbit(v)]) == {8.5} and set(r[v == -1.0]) == {2.0}
    assert set(emu["rank2"][1].ravel()) == {17} and np.array_equal(np.sort(emu["rank2"][2].ravel()), 2 * np.arange(1, 17))
    for f in FIELDS[:4]:
        assert np.isnan(emu[f][1]), f                       # the constant column: W == 0


def check_sums(u, ws, L, what):
    """m_q and g_q(t) of one series u [M][h] against longdouble sums, at the derived bounds"""
    M, h = u.shape
    ul = u.astype(LD)
    m = ws[:, 0]
    ref = ul.sum(axis=1) / LD(h)
    bound = LD((h + 2) * U53) * np.abs(ul).sum(axis=1) / LD(h)
    assert np.all(np.abs(m.astype(LD) - ref) <= bound), (what, "mean")
    d = ul - m.astype(LD)[:, None]
    for t in range(L + 1):
        prod = d[:, :h - t] * d[:, t:]
        ref = prod.sum(axis=1) / LD(h)
        bound = LD((h + 4) * U53) * np.abs(prod).sum(axis=1) / LD(h)
        err = np.abs(ws[:, 1 + t].astype(LD) - ref)
        assert np.all(err <= bound), (what, "g", t, float(np.max(err - bound)))


def figure_close(got, want, tol):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol * abs(want)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_sums_and_figures_against_the_longdouble_restatement(i):
    x, first, count, emu = emulated_case(i)
    chains, _ = SHAPES[i]
    h = count // 2
    L = min(h - 1, MAXLAG)
    tol = min(100 * FIGURE_MEASURED, 1e-9)
    worst = 0.0
    for k in range(min(x.shape[2], NKINDS)):                # every kind of column
        if not np.all(np.isfinite(split(x, first, count)[k])):
            continue
        for s in range(4):
            u = emu["series"][k, s]
            Ls = 0 if s == 1 else L
            check_sums(u, emu["ws"][k, s], Ls, (SHAPES[i], k, s))
            rhat, ess, trunc, stop, margin, _, _ = estimator(u, lags=s != 1, dtype=LD)
            got = emu["fin"][k, s]
            # the restatement decides every comparison of its scan clearly (else the fixture's seed is changed) ...
            assert margin > 1e-6, (SHAPES[i], k, s, margin)
            # ... so the flags are equal and the figures close
            assert int(got[2]) == trunc, (SHAPES[i], k, s)
            assert figure_close(got[0], rhat, tol) and figure_close(got[1], ess, tol), (SHAPES[i], k, s, got, rhat, ess)
            for a, b in ((got[0], rhat), (got[1], ess)):
                if not math.isnan(b):
                    worst = max(worst, abs(a - b) / abs(b))
        fin = emu["fin"][k]
        tail = float("nan") if math.isnan(fin[2, 1]) or math.isnan(fin[3, 1]) else min(fin[2, 1], fin[3, 1])
        assert same_bits([emu["rhat_bulk"][k], emu["rhat_folded"][k], emu["ess_bulk"][k], emu["ess_tail"][k]], [fin[0, 0], fin[1, 0], fin[0, 1], tail])
        assert emu["truncated"][k] == int(fin[0, 2]) | int(fin[2, 2]) << 1 | int(fin[3, 2]) << 2
    print("largest relative difference of a figure from the longdouble restatement: %.3g" % worst)
    assert worst <= FIGURE_MEASURED


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_properties_of_the_contract(i):
    x, first, count, emu = emulated_case(i)
    chains, _ = SHAPES[i]
    nv = x.shape[2]
    # a window gives the bits of its copy
    assert same_results(emulate(np.ascontiguousarray(x[:, first:first + count, :])), emu), SHAPES[i]
    # a shuffled column list with a duplicate gives the bits of the full call's entries
    cols = shuffled_with_duplicate(nv, i)
    assert same_results(emulate(x, first, count, cols=cols), emu, cols), SHAPES[i]
    # forcing several chunks gives the same bits
    if nv > 1:
        p = plan(chains, count, nv)
        small = emulate(x, first, count, cap=2 * p["per_col"])
        assert small["chunks"] == -(-nv // 2) and emu["chunks"] == 1 and same_results(small, emu), SHAPES[i]
    # a constant column is NaN; no column of these fixtures is NaN otherwise, but for the upper indicator where S < 20
    for k in range(nv):
        if k % NKINDS == 4:
            assert all(np.isnan(emu[f][k]) for f in FIELDS[:4]) and emu["truncated"][k] == 0
        else:
            assert np.isfinite(emu["rhat_bulk"][k]) and np.isfinite(emu["rhat_folded"][k]) and np.isfinite(emu["ess_bulk"][k])
            assert np.isfinite(emu["ess_tail"][k]) == (2 * chains * (count // 2) >= 20), (SHAPES[i], k)


def test_nan_and_inf_columns_are_nan_and_touch_nothing_else():
    x, first, count = case(5)                               # 5 chains, count 819, 17 columns
    clean = emulate(x, first, count)
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[1, first + count // 2, 3] = np.nan                  # count is odd: the middle draw is left out, the column stays clean
    bad[0, first - 1, 1] = np.nan                           # outside the window
    got = emulate(bad, first, count)
    for k in range(x.shape[2]):
        if k in (0, 6, 9):
            assert all(np.isnan(got[f][k]) for f in FIELDS[:4]) and got["truncated"][k] == 0, k
        else:
            assert all(same_bits(got[f][k], clean[f][k]) for f in FIELDS), k
    assert same_results(got, restate_nan_rule(bad, first, count, got))


def restate_nan_rule(x, first, count, got):
    """got with NaN wherever the window of a column holds a NaN or an infinity"""
    bad = ~np.all(np.isfinite(split(x, first, count)), axis=(1, 2))
    out = {f: np.array(got[f], dtype=np.float64) for f in FIELDS}
    for f in FIELDS[:4]:
        out[f][bad] = np.nan
    out["truncated"][bad] = 0
    return out


def test_the_plan_is_arithmetic_over_the_headers_constants():
    consts = (C.c_int * 6)()
    emulation().rk_constants(consts)
    assert list(consts) == [256, MAXLAG, MAXLAG + 2, 8064, 16, 256]
    for chains, count, k in ((1, 4, 1), (2, 9, 5), (3, 513, 17), (1, 16131, 3), (1024, 1000, 5), (64, 2000, 512), (64, 2000, 40)):
        h, M = count // 2, 2 * chains
        S, L = M * h, min(h - 1, MAXLAG)
        per = 32 * S + 8 * M * (L + 2)
        tiles, passes = -(-S // TILE), 0
        while TILE << passes < S:
            passes += 1
        want = dict(h=h, M=M, S=S, L=L, sl=L + 2, per_col=per, pc=max(1, min(CAP // per, k)), over_cap=0, tiles=tiles, mtiles=-(-S // MERGE_TILE), passes=passes,
                    stiles=-(-S // 256), blocks=-(-S // 256), i05=min(S - 1, int(math.floor(S * 0.05))), i95=min(S - 1, int(math.floor(S * 0.95))),
                    tau_min=1.0 / math.log10(S))
        assert plan(chains, count, k) == want, (chains, count, k)
    # the GPU tier's buffer that crosses the cap: 40 columns of 128 000 values, 30 to a chunk
    p = plan(64, 2000, 40)
    assert (p["S"], p["per_col"], p["pc"]) == (128000, 4096000 + 8 * 128 * 257, 30) and 40 * p["per_col"] > CAP
    # a single column beyond the cap: M (32 * 1024 + 8 * 257) bytes against 2^27
    assert plan(1927, 2048, 1)["over_cap"] == 0 and plan(1928, 2048, 1)["over_cap"] == 1 and plan(1928, 2048, 1)["pc"] == 1
    x = fixture(2, 40, 3, 1)
    assert emulation().rk_emulate(_capi.dptr(x), 2, 40, 3, 0, 40, None, 3, plan(2, 40, 3)["per_col"] - 1, *[None] * 9) == -1


# ---- 3. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    outs = [np.zeros(8) for _ in range(4)]
    tr = np.zeros(8, dtype=np.int32)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, cols=None, ncols=None, null=None):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        nc = (len(sel) if sel is not None else 0) if ncols is None else ncols
        o = [_capi.dptr(a) for a in outs] + [tr.ctypes.data_as(ip)]
        if null is not None:
            o[null] = None
        return L.rh_rank_diagnostics_device(ptr, 0, chains, iters, nvars, first, count, sel.ctypes.data_as(ip) if sel is not None else None, nc, *o)
    err = lambda: L.rh_last_error(None).decode()
    assert call(ptr=None) == _capi.RH_E_INVALID
    for null in range(5):
        assert call(null=null) == _capi.RH_E_INVALID and "NULL" in err()
    for first, count in ((0, 3), (0, 0), (0, 11), (7, 4), (-1, 5), (10, 4)):
        assert call(first=first, count=count) == _capi.RH_E_INVALID, (first, count)
        assert "window" in err() and "at least 4" in err()
    assert call(nvars=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    for cols in ([2], [-1], [0, 1, 7]):
        assert call(cols=cols) == _capi.RH_E_INVALID and "outside" in err(), cols
    assert call(cols=[0], ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(cols=[0], ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=1) == _capi.RH_E_INVALID and "ncols" in err()            # no list: 0 or nvars
    assert L.rh_sampler_rank_diagnostics(None, 0, 10, None, 0, *[_capi.dptr(a) for a in outs], tr.ctypes.data_as(ip)) == _capi.RH_E_INVALID
    # one column beyond the workspace cap: refused from the shape, whatever the machine
    assert call(chains=2049, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(ncols=2) == _capi.RH_E_DEVICE and call(cols=[1, 1, 0]) == _capi.RH_E_DEVICE and call(chains=1, count=4) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.rank_diagnostics_device(4096, 4, 10, 4)


# ---- 4. what the figures mean --------------------------------------------------------------------------------------------------------
def ar1(chains, n, phi, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((chains, n))
    x = np.empty((chains, n))
    x[:, 0] = e[:, 0]
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + math.sqrt(1.0 - phi * phi) * e[:, i]
    return x


def both(x):
    """the restatement's and the emulation's result over x [chains][n] as one column; the emulation's must be the restatement's"""
    x = np.ascontiguousarray(x[:, :, None])
    ref, emu = restate(x), emulate(x)
    for f in FIELDS[:4]:
        assert figure_close(float(emu[f][0]), float(ref[f][0]), 1e-9), (f, emu[f][0], ref[f][0])
    assert emu["truncated"][0] == ref["truncated"][0]
    return ref, emu


@pytest.mark.parametrize("phi, seed", [(0.5, 11), (0.9, 12)])
def test_bulk_ess_of_ar1_is_the_textbook_figure(phi, seed):
    x = ar1(4, 1000, phi, seed)
    want = 4000 * (1.0 - phi) / (1.0 + phi)
    for r in both(x):
        print(phi, r["ess_bulk"][0], want)
        assert abs(r["ess_bulk"][0] - want) <= 0.15 * want and r["rhat"][0] < 1.05 and r["truncated"][0] == 0


def test_a_trend_all_chains_share_is_seen():
    """4 chains x 1000 draws of AR(0.3), the first half of every chain moved by +1 and the second by -1: the chain means agree, so
    the reference's unsplit R-hat says 1; the split one does not"""
    import rainier_amd as R
    x = ar1(4, 1000, 0.3, 13)
    x[:, :500] += 1.0
    x[:, 500:] -= 1.0
    rhat_ref = [R.diagnostics(np.ascontiguousarray(x[:, :, None]))[0][0]]
    assert rhat_ref[0] < 1.01
    for r in both(x):
        print(rhat_ref[0], r["rhat_bulk"][0])
        assert r["rhat_bulk"][0] > 1.2 and r["rhat"][0] > 1.2


def test_a_chain_of_another_scale_is_seen_by_the_folded_rhat():
    x = ar1(4, 1000, 0.0, 14)
    x[3] *= 3.0
    for r in both(x):
        print(r["rhat_bulk"][0], r["rhat_folded"][0])
        assert r["rhat_bulk"][0] < 1.01 and r["rhat_folded"][0] > 1.1 and r["rhat"][0] == r["rhat_folded"][0]


def test_cauchy_draws_give_finite_figures():
    x = np.random.default_rng(15).standard_cauchy((4, 1000))
    for r in both(x):
        assert all(np.isfinite(r[f][0]) for f in FIELDS[:4]) and r["rhat"][0] < 1.01 and r["truncated"][0] == 0
