"""Posterior histograms and joint count grids on the device (csrc/device/rh_hist.hip.h: one binning pass with LDS integer adds),
the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ with every "thread" of a phase run in turn (the LDS add a plain
    add), is driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) and compared
    for EQUALITY with an independent oracle: np.histogram(col[finite], bins=returned edges) / np.histogram2d, the under / over / nan
    tallies with their definitions, the automatic bounds with min / max of the finite values bit for bit, the edges with the
    contract's formula restated in Python.  Counts are integers: there is no tolerance to choose;
  * the properties of the contract (a second call, a shuffled column list with a duplicate, chunking not being part of the result,
    the diagonal of a pair (a, a), the marginals of a grid), the plan's arithmetic, the C ABI's argument errors and its refusal to
    compute without a device.

tests/test_gpu_histogram_device.py runs the same fixtures through the kernels.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_hist_minmax_kernel", "rh_hist_minmax_finish_kernel", "rh_hist_bin_kernel", "rh_hist_pair_kernel", "rh_hist_finish_kernel")
SPLIT, TC, CAP, LDS_BYTES, TALLIES = 4096, 64, 128 << 20, 63 * 1024, 3
NS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
KS = (1, 3, 64, 65, 130)
NBINS = (1, 2, 20, 64, 257, 1024)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
NKINDS = 7
NORMAL, FAR, QUARTERS, CONSTANT, HUGE, SPECIAL, ALLNAN = range(NKINDS)


def fixture(chains, iters, nvars, seed):
    """[chains][iters][nvars]; column p is of kind p % 7: 0 a standard normal scaled by 1 + p / 7; 1 a normal at 1e6 with sd 1e-6
    (a width of few ulps per bin at 1024 bins: repeated guesses); 2 multiples of 0.25 in [-2, 2] (with the bounds (-2, 2) and 16 bins
    every value is on an edge, x == lo and x == hi occur); 3 the constant 2.0 (the +-0.5 rule; every row on one LDS address);
    4 1e16 + 2 * (an integer in 0 .. 4) (the edges collapse to 5 distinct values: the walk takes several steps); 5 |normal| with -0.0, +-inf and NaN among it (the
    smallest finite value is -0.0); 6 all NaN"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((chains, iters, nvars))
    flat = np.arange(chains * iters).reshape(chains, iters)
    for p in range(nvars):
        kind = p % NKINDS
        if kind == NORMAL:
            x[:, :, p] *= 1.0 + p / 7.0
        elif kind == FAR:
            x[:, :, p] = 1e6 + 1e-6 * x[:, :, p]
        elif kind == QUARTERS:
            x[:, :, p] = rng.integers(-8, 9, size=(chains, iters)) * 0.25
        elif kind == CONSTANT:
            x[:, :, p] = 2.0
        elif kind == HUGE:
            x[:, :, p] = 1e16 + 2.0 * rng.integers(0, 5, size=(chains, iters))
        elif kind == SPECIAL:
            v = np.abs(x[:, :, p])
            v[flat % 11 == 0] = -0.0
            v[flat % 13 == 5] = np.inf
            v[flat % 17 == 3] = -np.inf
            v[flat % 19 == 7] = np.nan
            x[:, :, p] = v
        else:
            x[:, :, p] = np.nan
    return x


def pooled(x, first=0, count=None, thin=1, cols=None):
    """[N][K]: flat row r = c * kept + j is draw (c, first + j * thin); column k is parameter cols[k]"""
    count = x.shape[1] - first if count is None else count
    rows = x[:, first:first + count:thin, :].reshape(-1, x.shape[2])
    return np.ascontiguousarray(rows if cols is None else rows[:, list(cols)])


def window(kept, thin):
    """(first, count, iterations) for `kept` kept iterations: the window starts late and ends early, and at thin 3 the count is no
    multiple of thin"""
    count = kept if thin == 1 else (kept - 1) * thin + 2
    return 2, count, 2 + count + 3


def shape_for(n):
    """(chains, kept) with chains * kept == n: three chains where 3 divides n (63, 4095, 8193: splits straddle chain boundaries),
    else the smallest other odd divisor, else two chains"""
    for m in (3, 5, 7, 17, 241, 2):
        if n % m == 0 and n // m >= 1:
            return m, n // m
    return 1, n


# ---- the contract restated and the independent oracle ---------------------------------------------------------------------------------
def edges_py(lo, hi, nbins):
    """the contract's edge formula, one IEEE operation at a time (Python floats are doubles)"""
    lo, hi = float(lo), float(hi)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    if lo != lo or hi != hi:
        return np.full(nbins + 1, np.nan)
    w = hi - lo
    e = [lo]
    for i in range(1, nbins):
        e.append(min(hi, max(e[-1], lo + (float(i) * w) / float(nbins))))
    e.append(hi)
    return np.array(e)


def auto_bounds(col):
    """(smallest, largest) finite value, a -0.0 as +0.0; none: (nan, nan)"""
    f = col[np.isfinite(col)]
    return (float(f.min()) + 0.0, float(f.max()) + 0.0) if len(f) else (np.nan, np.nan)


def bounds_for(col, given):
    return auto_bounds(col) if given is None or (np.isnan(given[0]) and np.isnan(given[1])) else (float(given[0]), float(given[1]))


def same_bits(a, b):
    """NaN matches NaN, -0.0 does not match +0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)))


def check_1d(rows, got, nbins, what, rng=None):
    """rows [N][K] (the pooled, selected draws); got = (edges, counts, under, over, nan); rng: None or [K][2] with NaN pairs"""
    edges, counts, under, over, nan = got
    n, k = rows.shape
    assert edges.shape == (k, nbins + 1) and counts.shape == (k, nbins) and counts.dtype == np.int64
    for p in range(k):
        col, e = rows[:, p], edges[p]
        lo, hi = bounds_for(col, None if rng is None else rng[p])
        assert same_bits(e, edges_py(lo, hi, nbins)), (what, p, "edges", e[:3], lo, hi)
        assert nan[p] == np.isnan(col).sum(), (what, p, "nan")
        if np.isnan(e).any():                                # no finite value: zero counts, the rows in under / over / nan
            assert not counts[p].any() and under[p] == (col == -np.inf).sum() and over[p] == (col == np.inf).sum(), (what, p)
        else:
            assert np.all(e[1:] >= e[:-1])
            want = np.histogram(col[np.isfinite(col)], bins=e)[0]
            assert np.array_equal(counts[p], want), (what, p, "counts", np.flatnonzero(counts[p] != want)[:5])
            assert under[p] == (col < e[0]).sum() and over[p] == (col > e[-1]).sum(), (what, p, "under / over")
        assert counts[p].sum() + under[p] + over[p] + nan[p] == n, (what, p, "the sum invariant")


def check_2d(rows, pairs, got, nbx, nby, what, rng=None):
    """rows [N][nvars] (the pooled draws, all columns); got = (xedges, yedges, grid, outside)"""
    xe, ye, grid, outside = got
    n = rows.shape[0]
    assert xe.shape == (len(pairs), nbx + 1) and ye.shape == (len(pairs), nby + 1) and grid.shape == (len(pairs), nbx, nby)
    for p, (a, b) in enumerate(pairs):
        x, y = rows[:, a], rows[:, b]
        for col, e, nb, ax in ((x, xe[p], nbx, 0), (y, ye[p], nby, 1)):
            lo, hi = bounds_for(col, None if rng is None else rng[p][ax])
            assert same_bits(e, edges_py(lo, hi, nb)), (what, p, ax, "edges")
        if np.isnan(xe[p]).any() or np.isnan(ye[p]).any():
            assert not grid[p].any() and outside[p] == n, (what, p)
            continue
        ok = np.isfinite(x) & np.isfinite(y)
        want = np.histogram2d(x[ok], y[ok], bins=[xe[p], ye[p]])[0]
        assert np.array_equal(grid[p], want.astype(np.int64)), (what, p, "grid")
        inside = (x >= xe[p][0]) & (x <= xe[p][-1]) & (y >= ye[p][0]) & (y <= ye[p][-1])
        assert outside[p] == n - inside.sum() and grid[p].sum() + outside[p] == n, (what, p, "outside")


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// histogram_run's / histogram2d_run's launches (csrc/draws.cpp) by their own plans (csrc/draws_plan.hpp; the cap a parameter) and the
// kernels' index arithmetic, one workgroup after the other
static void rhh_axes_edges(const double *base, long long iterations, long long nvars, long long thin, long long kept, long long N, long long S,
                           const int *sel, int n, const double *range, const int *nbins_of, double **edges_of) {
  std::vector<int> au_cols, au_of(n, -1);                       // the min / max pass runs over the automatic axes only
  for (int k = 0; k < n; k++)
    if (rh_plan::histogram_auto(range ? range + 2 * k : nullptr)) { au_of[k] = (int)au_cols.size(); au_cols.push_back(sel[k]); }
  const int na = (int)au_cols.size();
  std::vector<double> b(2 * (size_t)na + 2), part(2 * (size_t)(S * na) + 2), lds(2 * RHH_BLOCK);
  if (na) {
    const long long ctiles = (na + RHH_TC - 1) / RHH_TC;
    for (long long bid = 0; bid < S * ctiles; bid++) {
      const long long s = bid / ctiles, ct = bid - s * ctiles;
      rhh_minmax_split(base, iterations, nvars, thin, kept, N, au_cols.data(), na, (int)ct * RHH_TC, s, S, lds.data(), part.data(), RHH_BLOCK);
    }
    for (int k = 0; k < na; k++) rhh_minmax_finish(part.data(), S, na, k, b.data());
  }
  for (int k = 0; k < n; k++) {
    const int a = au_of[k];
    rh_plan::histogram_edges(a >= 0 ? b[2 * a] : range[2 * k], a >= 0 ? b[2 * a + 1] : range[2 * k + 1], nbins_of[k], edges_of[k]);
  }
}
static void rhh_finish(const std::vector<unsigned> &ws, long long S, long long L, long long u_lo, long long u_cnt, long long *out) {
  for (long long i = 0; i < u_cnt * L; i++) out[(u_lo + i / L) * L + i % L] = (long long)rhh_finish_word(ws.data(), S, L, i / L, i % L);
}
extern "C" int rhh_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, long long thin,
                           const int *cols, int K, int nbins, const double *range, long long cap, double *edges, long long *counts,
                           long long *under, long long *over, long long *nan) {
  const rh_plan::Histogram P = rh_plan::histogram_plan(chains, count, thin, K, nbins, cap);
  if (P.over_cap) return -1;
  const double *base = draws + first * nvars;
  std::vector<double *> edges_of(K);
  std::vector<int> nbins_of(K, nbins);
  for (int k = 0; k < K; k++) edges_of[k] = edges + (size_t)k * (nbins + 1);
  rhh_axes_edges(base, iterations, nvars, thin, P.kept, P.N, P.S, cols, K, range, nbins_of.data(), edges_of.data());
  const long long L = P.cpt * (nbins + RHH_TALLIES);
  std::vector<unsigned> ws((size_t)(P.tc * P.S * L), 0xdeadbeefu);
  std::vector<double> lds((size_t)P.lds_bytes / 8 + 1);
  std::vector<long long> out((size_t)(P.tiles * L));
  int chunks = 0;
  for (long long t0 = 0; t0 < P.tiles; t0 += P.tc, chunks++) {
    const long long t_cnt = P.tc < P.tiles - t0 ? P.tc : P.tiles - t0;
    for (long long bid = 0; bid < t_cnt * P.S; bid++) {
      const long long tl = bid / P.S, s = bid - tl * P.S;
      rhh_bin_split(base, iterations, nvars, thin, P.kept, P.N, cols, K, (int)((t0 + tl) * P.cpt), (int)P.cpt, nbins, edges, s, lds.data(),
                    ws.data() + (tl * P.S + s) * L, RHH_BLOCK);
    }
    rhh_finish(ws, P.S, L, t0, t_cnt, out.data());
  }
  for (int k = 0; k < K; k++) {
    const long long *h = out.data() + (size_t)k * (nbins + RHH_TALLIES);
    for (int b = 0; b < nbins; b++) counts[(size_t)k * nbins + b] = h[b];
    under[k] = h[nbins]; over[k] = h[nbins + 1]; nan[k] = h[nbins + 2];
  }
  return chunks;
}
extern "C" int rhh_emulate2d(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count,
                             long long thin, const int *pairs, int npairs, int nbx, int nby, const double *range, long long cap, double *xedges,
                             double *yedges, long long *grid, long long *outside) {
  const rh_plan::Histogram2d P = rh_plan::histogram2d_plan(chains, count, thin, npairs, nbx, nby, cap);
  if (P.over_cap) return -1;
  const double *base = draws + first * nvars;
  std::vector<double *> edges_of(2 * npairs);
  std::vector<int> nbins_of(2 * npairs);
  for (int p = 0; p < npairs; p++) {
    edges_of[2 * p] = xedges + (size_t)p * (nbx + 1); nbins_of[2 * p] = nbx;
    edges_of[2 * p + 1] = yedges + (size_t)p * (nby + 1); nbins_of[2 * p + 1] = nby;
  }
  rhh_axes_edges(base, iterations, nvars, thin, P.kept, P.N, P.S, pairs, 2 * npairs, range, nbins_of.data(), edges_of.data());
  const long long L = P.words;
  std::vector<unsigned> ws((size_t)(P.pc * P.S * L), 0xdeadbeefu);
  std::vector<double> lds((size_t)P.lds_bytes / 8 + 1);
  std::vector<long long> out((size_t)(npairs * L));
  int chunks = 0;
  for (long long p0 = 0; p0 < npairs; p0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < npairs - p0 ? P.pc : npairs - p0;
    for (long long bid = 0; bid < p_cnt * P.S; bid++) {
      const long long pl = bid / P.S, s = bid - pl * P.S, p = p0 + pl;
      rhh_pair_split(base, iterations, nvars, thin, P.kept, P.N, pairs[2 * p], pairs[2 * p + 1], nbx, nby, xedges + p * (nbx + 1),
                     yedges + p * (nby + 1), s, lds.data(), ws.data() + (pl * P.S + s) * L, RHH_BLOCK);
    }
    rhh_finish(ws, P.S, L, p0, p_cnt, out.data());
  }
  for (int p = 0; p < npairs; p++) {
    for (long long i = 0; i < L - 1; i++) grid[(size_t)p * (L - 1) + i] = out[(size_t)p * L + i];
    outside[p] = out[(size_t)p * L + L - 1];
  }
  return chunks;
}
// kept, N, S, cpt, tiles, mtiles, lds_bytes, per_tile, tc, over_cap
extern "C" void rhh_plan(long long chains, long long count, long long thin, long long K, int nbins, long long cap, long long *out) {
  const rh_plan::Histogram P = cap ? rh_plan::histogram_plan(chains, count, thin, K, nbins, cap) : rh_plan::histogram_plan(chains, count, thin, K, nbins);
  const long long v[10] = {P.kept, P.N, P.S, P.cpt, P.tiles, P.mtiles, P.lds_bytes, P.per_tile, P.tc, P.over_cap ? 1 : 0};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}
// kept, N, S, words, lds_bytes, per_pair, pc, over_cap
extern "C" void rhh_plan2d(long long chains, long long count, long long thin, long long npairs, int nbx, int nby, long long cap, long long *out) {
  const rh_plan::Histogram2d P = cap ? rh_plan::histogram2d_plan(chains, count, thin, npairs, nbx, nby, cap) : rh_plan::histogram2d_plan(chains, count, thin, npairs, nbx, nby);
  const long long v[8] = {P.kept, P.N, P.S, P.words, P.lds_bytes, P.per_pair, P.pc, P.over_cap ? 1 : 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}
// how many steps the walk takes from the uniform guess: the word by the device text, and the guess it started from
extern "C" int rhh_word_of(double x, const double *e, int nbins, int *guess) {
  const double lo = e[0], hi = e[nbins], inv = (double)nbins / (hi - lo), t = (x - lo) * inv;
  *guess = t >= 0.0 ? (t < (double)nbins ? (int)t : nbins - 1) : 0;
  return rhh_word(x, e, nbins, lo, hi, inv);
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_hist.hip.h in host mode) + the driver above as a host shared library (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_hist_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip, lp = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
        L.rhh_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, C.c_int, dp, ll, dp, lp, lp, lp, lp]
        L.rhh_emulate2d.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, C.c_int, C.c_int, dp, ll, dp, dp, lp, lp]
        L.rhh_plan.argtypes = [ll, ll, ll, ll, C.c_int, ll, lp]
        L.rhh_plan2d.argtypes = [ll, ll, ll, ll, C.c_int, C.c_int, ll, lp]
        L.rhh_word_of.argtypes = [C.c_double, dp, C.c_int, ip]
        _emu = L
    return _emu


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _range(rng, shape):
    if rng is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(rng, dtype=np.float64), shape))


def emulate(x, first=0, count=None, thin=1, cols=None, bins=20, rng=None, cap=CAP, chunks=False):
    """the host emulation over x [chains][iterations][nvars] -> edges, counts, under, over, nan (and the number of chunks)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    k = len(sel)
    r = _range(rng, (k, 2))
    edges, counts = np.full((k, bins + 1), -1.0), np.full((k, bins), -1, dtype=np.int64)
    under, over, nan = (np.full(k, -1, dtype=np.int64) for _ in range(3))
    n = L.rhh_emulate(_capi.dptr(x), m, iters, nv, first, count, thin, sel.ctypes.data_as(C.POINTER(C.c_int)), k, bins,
                      _capi.dptr(r) if r is not None else None, cap, _capi.dptr(edges), _lp(counts), _lp(under), _lp(over), _lp(nan))
    assert n >= 1, "beyond the cap"
    return (edges, counts, under, over, nan, n) if chunks else (edges, counts, under, over, nan)


def emulate2d(x, pairs, first=0, count=None, thin=1, bins=(32, 32), rng=None, cap=CAP, chunks=False):
    """-> xedges, yedges, grid, outside (and the number of chunks)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    p, (nbx, nby) = len(pr), bins
    r = _range(rng, (p, 2, 2))
    xe, ye = np.full((p, nbx + 1), -1.0), np.full((p, nby + 1), -1.0)
    grid, outside = np.full((p, nbx, nby), -1, dtype=np.int64), np.full(p, -1, dtype=np.int64)
    n = L.rhh_emulate2d(_capi.dptr(x), m, iters, nv, first, count, thin, pr.ctypes.data_as(C.POINTER(C.c_int)), p, nbx, nby,
                        _capi.dptr(r) if r is not None else None, cap, _capi.dptr(xe), _capi.dptr(ye), _lp(grid), _lp(outside))
    assert n >= 1, "beyond the cap"
    return (xe, ye, grid, outside, n) if chunks else (xe, ye, grid, outside)


def same_results(a, b):
    """edges bit for bit, every count equal"""
    nf = sum(1 for u in a if np.asarray(u).dtype == np.float64)
    return all(same_bits(u, v) for u, v in zip(a[:nf], b[:nf])) and all(np.array_equal(u, v) for u, v in zip(a[nf:5], b[nf:5]))


def plan(chains, count, thin, k, nbins, cap=0):
    out = (C.c_longlong * 10)()
    emulation().rhh_plan(chains, count, thin, k, nbins, cap, out)
    return dict(zip(("kept", "N", "S", "cpt", "tiles", "mtiles", "lds_bytes", "per_tile", "tc", "over_cap"), list(out)))


def plan2d(chains, count, thin, npairs, nbx, nby, cap=0):
    out = (C.c_longlong * 8)()
    emulation().rhh_plan2d(chains, count, thin, npairs, nbx, nby, cap, out)
    return dict(zip(("kept", "N", "S", "words", "lds_bytes", "per_pair", "pc", "over_cap"), list(out)))


def shuffled_with_duplicate(k, seed):
    """a column list for the sub-result property: a shuffle of about two thirds of the columns, one of them twice"""
    rng = np.random.default_rng(seed)
    pick = list(rng.permutation(k)[:max(1, (2 * k) // 3)])
    return [int(c) for c in pick + pick[:1]]


def check_sublist(full, sub, cols, what):
    """entry k of the call over cols is entry cols[k] of the call over all columns (automatic bounds depend on the column alone)"""
    assert same_bits(sub[0], full[0][cols]), (what, "edges")
    for q in range(1, 5):
        assert np.array_equal(sub[q], full[q][cols]), (what, q)


def pairs_for(k):
    """pairs over the fixture's kinds present among k columns: distinct kinds, a column with itself, the special and the collapsed columns"""
    want = [(0, 1), (2, 0), (3, 4), (5, 2), (4, 4), (6, 0), (1, 5), (k - 1, 0)]
    return [(a, b) for a, b in want if a < k and b < k] or [(0, 0)]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_histogram_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.histogram_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "" and r["unproven"] == 0, r   # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.histogram.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.histogram_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_model_sources_do_not_carry_the_histogram_kernels():
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_hist" not in src


# ---- 2. the device text, on the host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", NBINS)
@pytest.mark.parametrize("n", NS)
def test_host_emulation_equals_numpy(n, nbins):
    chains, kept = shape_for(n)
    for k in KS:
        for thin in (1, 3):
            first, count, iters = window(kept, thin)
            x = fixture(chains, iters, k, 7 * n + 31 * k + thin)
            got = emulate(x, first, count, thin, bins=nbins)
            check_1d(pooled(x, first, count, thin), got, nbins, (n, k, nbins, thin))
        # a second call; a window is its rows (the same result as a thinned copy on its own)
        assert same_results(emulate(x, first, count, thin, bins=nbins), got)
        assert same_results(emulate(np.ascontiguousarray(x[:, first:first + count:thin, :]), bins=nbins), got)
        # a shuffled column list with one duplicate returns the rows of the full call
        cols = shuffled_with_duplicate(k, n + k)
        check_sublist(got, emulate(x, first, count, thin, cols=cols, bins=nbins), cols, (n, k, nbins))


def test_given_bounds_values_on_edges_and_mixed_ranges():
    """multiples of 0.25 with the bounds (-2, 2) and 16 bins: every value is on an edge, x == lo and x == hi occur; the special column
    with lo = 0.0 (-0.0 counts in the first bin, not under); bounds that cut values off on both sides; NaN pairs among given ones"""
    for n in (65, 4097):
        chains, kept = shape_for(n)
        x = fixture(chains, kept, 14, n)
        rows = pooled(x)
        got = emulate(x, cols=[QUARTERS, QUARTERS + 7], bins=16, rng=(-2.0, 2.0))
        check_1d(rows[:, [QUARTERS, QUARTERS + 7]], got, 16, ("quarters", n), [(-2.0, 2.0)] * 2)
        assert same_bits(got[0][0], np.arange(-2.0, 2.25, 0.25)) and got[2].sum() == 0 and got[3].sum() == 0
        assert got[1][0, 15] == ((rows[:, QUARTERS] == 1.75) | (rows[:, QUARTERS] == 2.0)).sum()       # the last bin is closed
        got = emulate(x, cols=[SPECIAL], bins=8, rng=(0.0, 1.5))
        check_1d(rows[:, [SPECIAL]], got, 8, ("special", n), [(0.0, 1.5)])
        assert got[2][0] == (rows[:, SPECIAL] == -np.inf).sum() and got[3][0] >= (rows[:, SPECIAL] == np.inf).sum() > 0
        assert got[1][0, 0] >= (rows[:, SPECIAL] == 0.0).sum() > 0
        rng = [(-1.0, 1.0), (np.nan, np.nan), (-0.5, 0.25), (2.0, 2.0), (1e16, 1e16 + 6.0), (np.nan, np.nan), (0.0, 1.0)] * 2
        got = emulate(x, bins=20, rng=rng)
        check_1d(rows, got, 20, ("mixed", n), rng)
        assert same_bits(got[0][CONSTANT], edges_py(1.5, 2.5, 20))                                      # lo == hi, given
    # the automatic bounds of the special column: the smallest finite value is -0.0 and comes back as +0.0
    e = emulate(fixture(3, 100, 6, 5), cols=[SPECIAL])[0]
    assert e[0, 0] == 0.0 and not np.signbit(e[0, 0])
    e = emulate(np.full((1, 1, 6), -0.0), cols=[SPECIAL])[0]
    assert same_bits(e[0], edges_py(0.0, 0.0, 20)) and e[0, 0] == -0.5
    # a constant of magnitude 2^53 or more: lo - 0.5 == lo, the width stays 0, all edges are equal and every row is in the last bin
    x = np.full((3, 50, 1), 1e16)
    for rng in (None, (1e16, 1e16)):
        e, counts, under, over, nan = emulate(x, bins=8, rng=rng)
        assert np.all(e == 1e16) and counts[0].tolist() == [0] * 7 + [150] and under[0] == over[0] == nan[0] == 0
        check_1d(pooled(x), (e, counts, under, over, nan), 8, "a constant beyond 2^53", None if rng is None else [rng])


def test_collapsed_edges_need_a_walk_of_several_steps():
    """1e16 + 2 * integer over 64 bins: the 65 edges hold few distinct values, and from the uniform guess the defining bin is more than
    one step away for some value -- a single correction each way would miscount"""
    L = emulation()
    x = fixture(3, 700, 5, 11)
    e, counts = emulate(x, cols=[HUGE], bins=64)[:2]
    assert len(np.unique(e[0])) == 5 and counts[0].sum() == 2100
    guess, far = C.c_int(0), 0
    for v in np.unique(x[:, :, HUGE]):
        b = L.rhh_word_of(float(v), _capi.dptr(np.ascontiguousarray(e[0])), 64, C.byref(guess))
        far = max(far, abs(b - guess.value))
        assert b == 63 if v == e[0, 64] else e[0, b] <= v < e[0, b + 1]
    assert far >= 2, far


def test_chunking_is_not_part_of_the_result():
    """130 columns at 257 bins are 9 tiles of 16 columns, 8193 rows 3 splits (48.75 KiB of partials per tile): caps that hold all,
    four and one tile; 6 pairs at 64 x 64 (48 KiB each) likewise"""
    chains, kept = shape_for(8193)
    x = fixture(chains, kept, 130, 99)
    one = emulate(x, bins=257, chunks=True)
    p = plan(chains, kept, 1, 130, 257)
    assert one[5] == 1 and (p["cpt"], p["tiles"], p["S"], p["per_tile"]) == (16, 9, 3, 3 * 16 * 260 * 4)
    for cap, want in ((200 << 10, 3), (p["per_tile"], 9)):
        got = emulate(x, bins=257, cap=cap, chunks=True)
        assert got[5] == want and same_results(got, one), cap
    assert emulation().rhh_emulate(_capi.dptr(x), chains, kept, 130, 0, kept, 1, None, 130, 257, None, p["per_tile"] - 1, None, None, None, None, None) == -1
    pairs = [(0, 1), (2, 0), (3, 4), (5, 2), (4, 4), (129, 7)]
    one = emulate2d(x, pairs, bins=(64, 64), chunks=True)
    per = plan2d(chains, kept, 1, 6, 64, 64)["per_pair"]
    assert one[4] == 1 and per == 3 * 4097 * 4
    for cap, want in ((2 * per + 5, 3), (per, 6)):
        got = emulate2d(x, pairs, bins=(64, 64), cap=cap, chunks=True)
        assert got[4] == want and same_bits(got[0], one[0]) and same_bits(got[1], one[1]) and np.array_equal(got[2], one[2]) and np.array_equal(got[3], one[3])


@pytest.mark.parametrize("n", NS)
def test_host_emulation_pairs_equal_numpy(n):
    chains, kept = shape_for(n)
    for k, bins, thin in ((7, (32, 32), 1), (7, (1, 1), 3), (14, (64, 64), 3), (6, (7, 300), 1), (5, (4096, 1), 1), (3, (1, 4096), 3)):
        first, count, iters = window(kept, thin)
        x = fixture(chains, iters, k, 13 * n + k + thin)
        rows, pairs = pooled(x, first, count, thin), pairs_for(k)
        got = emulate2d(x, pairs, first, count, thin, bins=bins)
        check_2d(rows, pairs, got, bins[0], bins[1], (n, k, bins, thin))
        again = emulate2d(x, pairs[::-1], first, count, thin, bins=bins)                      # a second call, the list reversed
        assert np.array_equal(again[2][::-1], got[2]) and np.array_equal(again[3][::-1], got[3]) and same_bits(again[0][::-1], got[0])
        for p, (a, b) in enumerate(pairs):                                                      # a pair (a, a) is on the diagonal
            if a == b and bins[0] == bins[1]:
                assert got[2][p].sum() == np.trace(got[2][p])


def test_marginals_of_a_grid_over_given_bounds():
    """the marginal of a pair's grid equals the 1-D counts over the same bounds minus the rows the other axis rejects"""
    chains, kept = shape_for(4097)
    x = fixture(chains, kept, 7, 4)
    rows = pooled(x)
    for (a, b), (rx, ry) in (((NORMAL, SPECIAL), ((-1.0, 1.5), (0.0, 1.0))), ((QUARTERS, NORMAL), ((-2.0, 2.0), (-0.5, 3.0))), ((FAR, HUGE), ((1e6 - 1e-6, 1e6 + 2e-6), (1e16, 1e16 + 8.0)))):
        xe, ye, grid, outside = emulate2d(x, [(a, b)], bins=(16, 12), rng=[(rx, ry)])
        check_2d(rows, [(a, b)], (xe, ye, grid, outside), 16, 12, (a, b), [(rx, ry)])
        y_ok = (rows[:, b] >= ry[0]) & (rows[:, b] <= ry[1])
        x_ok = (rows[:, a] >= rx[0]) & (rows[:, a] <= rx[1])
        full_x = emulate(x, cols=[a], bins=16, rng=rx)
        assert same_bits(full_x[0][0], xe[0])
        rejected = np.histogram(rows[x_ok & ~y_ok, a], bins=xe[0])[0]
        assert np.array_equal(grid[0].sum(axis=1), full_x[1][0] - rejected)
        full_y = emulate(x, cols=[b], bins=12, rng=ry)
        rejected = np.histogram(rows[y_ok & ~x_ok, b], bins=ye[0])[0]
        assert np.array_equal(grid[0].sum(axis=0), full_y[1][0] - rejected)


def test_the_plan_is_arithmetic_over_the_headers_constants():
    # columns of a tile: the largest power of two, at most 64, whose edge tables (f64) and histograms (u32, + 3 tallies) fit 63 KiB
    for nbins in range(1, 1025):
        per = 8 * (nbins + 1) + 4 * (nbins + TALLIES)
        cpt = max(c for c in (1, 2, 4, 8, 16, 32, 64) if c * per <= LDS_BYTES)
        p = plan(3, 100, 1, 200, nbins)
        assert (p["cpt"], p["lds_bytes"]) == (cpt, cpt * per) and p["lds_bytes"] <= LDS_BYTES, nbins
    assert [plan(1, 1, 1, 1, b)["cpt"] for b in (20, 82, 83, 128, 257, 1024)] == [64, 64, 32, 32, 16, 4]
    for chains, count, thin, k, nbins in ((1024, 1000, 1, 5, 20), (3, 1365, 1, 65, 64), (3, 4100, 3, 1, 1), (256, 40, 2, 10004, 20), (4, 16384, 1, 2100, 1024)):
        kept = -(-count // thin)
        n = chains * kept
        s = -(-n // SPLIT)
        p = plan(chains, count, thin, k, nbins)
        per = s * p["cpt"] * (nbins + TALLIES) * 4
        want = dict(kept=kept, N=n, S=s, cpt=p["cpt"], tiles=-(-k // p["cpt"]), mtiles=-(-k // TC), lds_bytes=p["lds_bytes"], per_tile=per,
                    tc=max(1, min(CAP // per, -(-k // p["cpt"]))), over_cap=0)
        assert p == want, (chains, count, thin, k, nbins)
    # the GPU tier's shape that crosses the cap: 525 tiles of 256.75 KiB, 510 to a chunk
    p = plan(4, 16384, 1, 2100, 1024)
    assert (p["N"], p["S"], p["tiles"], p["per_tile"], p["tc"]) == (65536, 16, 525, 16 * 4 * 1027 * 4, 510) and p["tiles"] * p["per_tile"] > CAP
    # one tile alone beyond the cap
    assert plan(8168, 4096, 1, 2, 1024)["over_cap"] == 0 and plan(8169, 4096, 1, 2, 1024)["over_cap"] == 1
    for nbx, nby in ((1, 1), (32, 32), (64, 64), (4096, 1), (1, 4096), (7, 300)):
        p = plan2d(1024, 400, 1, 10, nbx, nby)
        assert p == dict(kept=400, N=409600, S=100, words=nbx * nby + 1, lds_bytes=8 * (nbx + nby + 2) + 4 * (nbx * nby + 1), per_pair=100 * (nbx * nby + 1) * 4,
                         pc=10, over_cap=0) and p["lds_bytes"] <= LDS_BYTES


# ---- 3. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    edges, counts, tally = np.zeros(4096), np.zeros(4096, dtype=np.int64), np.zeros(16, dtype=np.int64)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    i64 = lambda a: a.ctypes.data_as(lp)

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, thin=1, cols=None, ncols=None, nbins=20, rng=None, outs=True):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        nc = (len(sel) if sel is not None else 0) if ncols is None else ncols
        r = np.ascontiguousarray(rng, dtype=np.float64) if rng is not None else None
        return L.rh_histogram_device(ptr, 0, chains, iters, nvars, first, count, thin, sel.ctypes.data_as(ip) if sel is not None else None, nc, nbins,
                                     _capi.dptr(r) if r is not None else None, _capi.dptr(edges) if outs else None, i64(counts) if outs else None,
                                     i64(tally), None, None)

    def call2(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, thin=1, pairs=((0, 1),), npairs=None, nbx=8, nby=8, rng=None, outs=True):
        pr = np.array(pairs, dtype=np.int32).reshape(-1, 2) if pairs is not None else None
        r = np.ascontiguousarray(rng, dtype=np.float64) if rng is not None else None
        return L.rh_histogram2d_device(ptr, 0, chains, iters, nvars, first, count, thin, pr.ctypes.data_as(ip) if pr is not None else None,
                                       (len(pr) if pr is not None else 0) if npairs is None else npairs, nbx, nby, _capi.dptr(r) if r is not None else None,
                                       _capi.dptr(edges) if outs else None, _capi.dptr(edges), i64(counts), None)
    err = lambda: L.rh_last_error(None).decode()
    for f in (call, call2):
        assert f(ptr=None) == _capi.RH_E_INVALID and f(outs=False) == _capi.RH_E_INVALID
        for first, count, thin in ((0, 0, 1), (0, 11, 1), (5, 6, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):      # a broken window; N < 1
            assert f(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
            assert "window" in err()
        assert f(nvars=0) == _capi.RH_E_INVALID and f(chains=0) == _capi.RH_E_INVALID
    for cols in ([2], [-1], [0, 1, 7]):
        assert call(cols=cols) == _capi.RH_E_INVALID and "outside" in err(), cols
    assert call(cols=[0], ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(cols=[0], ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=1) == _capi.RH_E_INVALID and "ncols" in err()            # no list: 0 or nvars
    for nbins in (0, -1, 1025):
        assert call(nbins=nbins) == _capi.RH_E_INVALID and "nbins" in err(), nbins
    bad_bounds = ((1.0, 0.0), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 0.0), (0.0, np.inf), (-1e308, 1e308))
    for bad in bad_bounds:
        assert call(rng=[(0.0, 1.0), bad]) == _capi.RH_E_INVALID and "range" in err(), bad
        assert call2(rng=[[(0.0, 1.0), bad]]) == _capi.RH_E_INVALID and "range" in err(), bad
        assert call2(rng=[[bad, (np.nan, np.nan)]]) == _capi.RH_E_INVALID and "range" in err(), bad
    for pairs in (((0, 2),), ((-1, 0),), ((0, 1), (1, 5))):
        assert call2(pairs=pairs) == _capi.RH_E_INVALID and "pairs" in err(), pairs
    assert call2(pairs=None) == _capi.RH_E_INVALID
    assert call2(npairs=0) == _capi.RH_E_INVALID and "npairs" in err()
    for nbx, nby in ((0, 4), (4, 0), (-1, -1), (65, 64), (4097, 1), (1 << 16, 1 << 16)):
        assert call2(nbx=nbx, nby=nby) == _capi.RH_E_INVALID and "nbx" in err(), (nbx, nby)
    assert L.rh_sampler_histogram(None, 0, 10, 1, None, 0, 20, None, _capi.dptr(edges), i64(counts), None, None, None) == _capi.RH_E_INVALID
    assert L.rh_sampler_histogram2d(None, 0, 10, 1, None, 0, 8, 8, None, _capi.dptr(edges), _capi.dptr(edges), i64(counts), None) == _capi.RH_E_INVALID
    # one tile's partial counts beyond the workspace cap: refused from the shape, whatever the machine
    assert call(chains=8169, iters=4096, count=4096, nbins=1024) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    assert call2(chains=8192, iters=4096, count=4096, nbx=64, nby=64) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(ncols=2) == _capi.RH_E_DEVICE and call(cols=[1, 1, 0]) == _capi.RH_E_DEVICE      # valid requests
        assert call(chains=1, count=1, nbins=1024, rng=[(0.0, 0.0), (np.nan, np.nan)]) == _capi.RH_E_DEVICE
        assert call2() == _capi.RH_E_DEVICE and call2(pairs=((1, 1), (0, 1)), nbx=4096, nby=1) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.histogram_device(4096, 4, 10, 4)
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.histogram2d_device(4096, 4, 10, 4, [(0, 1)])


def test_python_surface():
    import inspect
    import re
    import rainier_amd as R
    hdr = open(os.path.join(ROOT, "include", "rainier_hip.h")).read()
    declared = set(re.findall(r"\bint (rh_[a-z0-9_]*histogram[a-z0-9_]*)\s*\(", hdr))
    assert declared == {"rh_sampler_histogram", "rh_histogram_device", "rh_histogram_lower_only"} | set(_capi.EXPORTS_2D)
    assert all(hasattr(_capi.lib(), name) for name in declared) and _capi.lib().rh_abi_version() == 6
    assert list(inspect.signature(R.Sampler.histogram).parameters) == ["self", "first", "count", "thin", "cols", "bins", "range"]
    assert list(inspect.signature(R.Sampler.histogram2d).parameters) == ["self", "pairs", "first", "count", "thin", "bins", "range"]
    assert list(inspect.signature(R.histogram_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "thin",
                                                                      "cols", "bins", "range"]
    assert list(inspect.signature(R.histogram2d_device).parameters) == ["ptr", "chains", "iterations", "nvars", "pairs", "device", "first", "count",
                                                                        "thin", "bins", "range"]
    sig = inspect.signature(R.Sampler.histogram).parameters
    assert sig["first"].default == 0 and sig["count"].default is None and sig["thin"].default == 1 and sig["cols"].default is None
    assert sig["bins"].default == 20 and sig["range"].default is None and inspect.signature(R.Sampler.histogram2d).parameters["bins"].default == (32, 32)
    assert R.Histogram._fields == ("cols", "edges", "counts", "under", "over", "nan") and R.Histogram2d._fields == ("pairs", "xedges", "yedges", "grid", "outside")
    assert "20 bins" in R.Sampler.histogram.__doc__ and "plotting library" in R.Sampler.histogram.__doc__
    # range: its nesting depth says whether it is one set of bounds for all entries or one per entry, never its length
    from rainier_amd.sampler import _range_arg
    nan = np.nan
    assert _range_arg(None, (3, 2), "h") is None and _range_arg((0, 1), (2, 2), "h").tolist() == [[0, 1], [0, 1]]
    assert _range_arg([(0, 1), (2, 3)], (2, 2), "h").tolist() == [[0, 1], [2, 3]]
    assert same_bits(_range_arg([(0, 1), None, (2, 3)], (3, 2), "h"), [[0, 1], [nan, nan], [2, 3]])
    assert _range_arg(((0, 1), (5, 6)), (2, 2, 2), "h").tolist() == [[[0, 1], [5, 6]]] * 2
    assert same_bits(_range_arg([((0, 1), (5, 6)), ((2, 3), None)], (2, 2, 2), "h"), [[[0, 1], [5, 6]], [[2, 3], [nan, nan]]])
    for bad, shape in (((0, 1, 2), (3, 2)), ([(0, 1)], (3, 2)), (5.0, (3, 2)), ([(0, 1)], (1, 2, 2)), ([[[(0, 1)]]], (1, 2))):
        with pytest.raises(ValueError):
            _range_arg(bad, shape, "h")
    # .density is np.histogram(..., density=True); a zero-width bin gives NaN
    rng = np.random.default_rng(3)
    v = rng.standard_normal(500)
    c, e = np.histogram(v, bins=12)
    h = R.Histogram((0,), e[None, :], c[None, :].astype(np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64))
    assert np.array_equal(h.density[0], c / (c.sum() * np.diff(e)))
    assert np.allclose(h.density[0], np.histogram(v, bins=12, density=True)[0], rtol=2.0 ** -51, atol=0)   # (numpy divides twice: two roundings apart)
    h = R.Histogram((0,), np.array([[0.0, 1.0, 1.0, 2.0]]), np.array([[3, 0, 5]]), *(np.zeros(1, np.int64) for _ in range(3)))
    assert np.isnan(h.density[0, 1]) and h.density[0, 0] == 3 / 8 and h.density[0, 2] == 5 / 8
    w = rng.standard_normal(500)
    g, xe, ye = np.histogram2d(v, w, bins=(6, 5))
    h2 = R.Histogram2d(((0, 1),), xe[None, :], ye[None, :], g[None, :, :].astype(np.int64), np.zeros(1, np.int64))
    assert np.allclose(h2.density[0], np.histogram2d(v, w, bins=(6, 5), density=True)[0], rtol=2.0 ** -50, atol=0)
