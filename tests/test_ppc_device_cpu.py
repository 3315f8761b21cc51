"""Posterior predictive checks on the device (csrc/device/rh_ppc.hip.h), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (ppc_plan of csrc/draws_plan.hpp) -- the emulation -- and compared
    with an independent numpy restatement of the contract in include/rainier_hip.h:
      - min, max, quantile, frac_le, t_obs of those kinds, which draws are NaN, and the three counts: exactly;
      - mean and sd at bounds that are derived, not tuned.  With u = 2^-53, n values v and longdouble references, n - 1 adds in any
        order and one division give
            |mean - ref| <= d,  d = (n + 2) u sum|v| / n
        and, as tests/test_loo_device_cpu.py derives it for p_waic (a subtraction and a product per term, n - 1 adds, a division, and
        the mean's error d, which enters squared because the deviations from the exact mean sum to zero),
            |var - ref| <= b,  b = ((n + 6) u sum (v - mean)^2 + 2 n d^2) / (n - 1);
        the square root of a value within b of var lies within b / sd of sd (both ways, whatever b), and is rounded once more:
            |sd - ref| <= b / sd + 2 u sd;
  * the contract's properties: a NaN, an infinity, a constant segment and a mix of zeros touch their own (draw, segment) only, the
    sum's order depends on the segment's length alone, duplicated and shuffled columns, the window; the plan's arithmetic; the C ABI's
    refusals, all without a device;
  * what the figures mean: rows of ten standard normals, whose mean and maximum have known distributions.

tests/test_gpu_ppc_device.py runs the same shapes through the kernels.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_ppc_stat_kernel", "rh_ppc_count_kernel")
CAP, MAX_STATS, MAX_OUT, BLOCK, STAGE, LDS_DOUBLES = 4096, 16, 4096, 256, 4096, 8192
LD = np.longdouble
U53 = 2.0 ** -53
MEAN, SD, MIN, MAX, QUANTILE, FRAC_LE = range(6)
EXACT = (MIN, MAX, QUANTILE, FRAC_LE)
RH_E_INVALID, RH_E_DEVICE, RH_E_UNSUPPORTED = 1, 3, 5

SIX = [(MEAN, 0.0), (SD, 0.0), (MIN, 0.0), (MAX, 0.0), (QUANTILE, 0.5), (FRAC_LE, 0.0)]
SIXTEEN = [(MEAN, 0.0), (SD, 0.0), (MIN, 0.0), (MAX, 0.0), (QUANTILE, 0.0), (QUANTILE, 1.0), (QUANTILE, 0.25), (QUANTILE, 0.5), (QUANTILE, 0.9),
           (QUANTILE, 0.999), (FRAC_LE, 0.0), (FRAC_LE, 1.0), (FRAC_LE, -0.5), (MEAN, 0.0), (MAX, 0.0), (QUANTILE, 0.1)]
KIDIQ_SEGS = (60, 50, 44, 43, 43, 42, 41, 40, 40, 31)


def five_segments():
    """nin = 40: 17 columns, one column, one column twice, 20 columns in a shuffled order, three far apart"""
    return [list(range(17)), [17], [18, 18], [int(c) for c in np.random.default_rng(5).permutation(np.arange(19, 39))], [5, 39, 30]]


def kidiq_segments():
    off = np.concatenate([[0], np.cumsum(KIDIQ_SEGS)])
    return [list(range(off[g], off[g + 1])) for g in range(len(KIDIQ_SEGS))]


def tile_rows(k):
    """the rows of a tile for one segment of k columns, as ppc_plan has them (test_the_plan checks this against the plan itself)"""
    stride = k if (k & 1) or k >= STAGE else k + 1
    rows = max(1, min(BLOCK, STAGE // stride))
    p = 1
    while p < k:
        p *= 2
    conc = BLOCK // max(1, min(BLOCK, p // 16))
    if rows > conc:
        rows -= rows % conc
    return rows


# (nin, cols, segments, stats, chains, iterations, first, count, thin).  One segment of every length at which the kernel takes another
# path -- n = 1, 2, 3; around one wave's worth of lanes, around the block, KidIQ's, the cap and one below -- each with S one below, at
# and one above its tile and at two tiles and one; then the tables, the segment lists, a shuffled selection and the windows.
CASES = []
for n_ in (1, 2, 3, 63, 64, 65, 255, 256, 257, 434, CAP - 1, CAP):
    t_ = tile_rows(n_)
    for s_ in sorted({t_ - 1, t_, t_ + 1, 2 * t_ + 1} - {0}):
        CASES.append((n_, None, None, SIX, 1, s_, 0, s_, 1))
CASES += [
    (40, None, five_segments(), SIX, 3, 40, 0, 40, 1),
    (40, None, five_segments(), SIXTEEN, 2, 31, 4, 26, 3),                      # first > 0, thin = 3 does not divide the count
    (40, None, five_segments(), [(QUANTILE, 0.5)], 2, 20, 0, 20, 1),
    (40, None, five_segments(), [(SD, 0.0)], 2, 20, 3, 17, 1),
    (434, None, kidiq_segments(), SIX, 2, 12, 1, 10, 3),
    (434, None, None, SIXTEEN, 2, 9, 0, 9, 1),
    (50, [int(c) for c in np.random.default_rng(11).permutation(50)], None, SIX, 2, 30, 2, 25, 2),
    (30, [7, 7, 3, 29, 0, 7], None, SIX, 4, 70, 0, 70, 1),                      # a duplicate in the column list
    (8, None, None, SIX, 5, 230, 0, 230, 1),                                    # the narrow shape: a lane per draw, several tiles
]


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def selection(nin, cols, segments):
    """-> (cols [K], seg_off [nseg + 1]) as rh_ppc_create completes them"""
    if segments is not None:
        return [c for seg in segments for c in seg], [0] + [int(v) for v in np.cumsum([len(seg) for seg in segments])]
    cc = list(range(nin)) if cols is None else list(cols)
    return cc, [0, len(cc)]


def base_buffer(nin, chains, iterations, seed):
    """even flat rows iid normal, odd flat rows Poisson-like integers with many ties and zeros"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((chains, iterations, nin))
    flat = x.reshape(chains * iterations, nin)
    flat[1::2] = rng.poisson(0.7, size=flat[1::2].shape)
    return x


def specials(x, cc, off, first, count, thin):
    """a copy of x with, in the kept draws r = 0 .. 3 (as far as there are that many): r = 0 the first segment constant, r = 1 the last
    segment a mix of -0.0 and +0.0, r = 2 one NaN in the first segment, r = 3 one +inf in the first segment.  -> (copy, [(r, segment)])"""
    x = x.copy()
    kept = -(-count // thin)
    S = x.shape[0] * kept
    touched = []
    nseg = len(off) - 1
    for r in range(min(4, S)):
        c, j = divmod(r, kept)
        row = x[c, first + j * thin]
        g = nseg - 1 if r == 1 else 0
        sel = cc[off[g]:off[g + 1]]
        if r == 0:
            row[sel] = 3.7
        elif r == 1:
            row[sel] = np.where(np.arange(len(sel)) % 3 == 1, -0.0, 0.0)
        elif r == 2:
            row[sel[len(sel) // 2]] = np.nan
        else:
            row[sel[0]] = np.inf
        # a column selected twice carries the value into every segment that names it
        hit = {g2 for g2 in range(nseg) if set(cc[off[g2]:off[g2 + 1]]) & set(sel)}
        touched += [(r, g2) for g2 in sorted(hit)]
    return x, touched


def case(i):
    """-> (x with the specials, base x, touched, cols, seg_off, stats, first, count, thin, y)"""
    nin, cols, segments, stats, chains, iterations, first, count, thin = CASES[i]
    cc, off = selection(nin, cols, segments)
    base = base_buffer(nin, chains, iterations, 300 + i)
    x, touched = specials(base, cc, off, first, count, thin)
    kept = -(-count // thin)
    S = chains * kept
    c, j = divmod(S - 1, kept)                                  # y: the last kept draw, so that n_eq >= 1 in every output
    y = x[c, first + j * thin].copy()
    return x, base, touched, cc, off, stats, first, count, thin, y


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
def to_keys(v):
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).copy()
    b[np.isnan(v)] = np.uint64(0x7ff8000000000000)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b ^ np.uint64(0x8000000000000000))


def from_keys(k):
    neg = ~(k >> np.uint64(63)).astype(bool)
    return np.where(neg, ~k, k ^ np.uint64(0x8000000000000000)).view(np.float64)


def kept_rows(x, first, count, thin):
    chains = x.shape[0]
    return np.ascontiguousarray(x[:, first:first + count:thin, :]).reshape(chains * -(-count // thin), x.shape[2])


def restate(rows, cc, off, stats):
    """rows [S][nin] -> (T [S][nout] in double -- exact for the exact kinds, the longdouble reference rounded for mean and sd --,
    mean bound [S][nout], sd bound [S][nout]; bounds 0 where the value must be met exactly)"""
    S = rows.shape[0]
    nseg, nstat = len(off) - 1, len(stats)
    T = np.full((S, nseg * nstat), -7.0)
    bound = np.zeros_like(T)
    for g in range(nseg):
        v = rows[:, cc[off[g]:off[g + 1]]]
        n = v.shape[1]
        keys = np.sort(to_keys(v), axis=1)
        has_nan = np.isnan(v).any(axis=1)
        alleq = keys[:, 0] == keys[:, -1]
        with np.errstate(all="ignore"):
            V = v.astype(LD)
            mean = V.sum(axis=1) / LD(n)
            d = (n + 2) * U53 * np.abs(V).sum(axis=1) / LD(n)
            mean = np.where(alleq, V[:, 0], mean)
            d = np.where(alleq, LD(0), d)
            # the double mean is what the contract's second pass subtracts; against the exact one the difference is inside b
            ssq = ((V - mean[:, None]) ** 2).sum(axis=1)
            var = ssq / LD(n - 1) if n > 1 else np.full(S, np.nan, dtype=LD)
            b = ((n + 6) * U53 * ssq + 2 * n * d * d) / LD(max(1, n - 1))
            sd = np.sqrt(var)
            bsd = np.where(ssq == 0, LD(0), b / sd + 2 * U53 * sd)
            sd = np.where(alleq & (n > 1), LD(0), sd)
            bsd = np.where(alleq, LD(0), bsd)
        for k, (kind, arg) in enumerate(stats):
            o = g * nstat + k
            if kind == MEAN:
                T[:, o], bound[:, o] = mean.astype(np.float64), d.astype(np.float64)
            elif kind == SD:
                T[:, o], bound[:, o] = sd.astype(np.float64), bsd.astype(np.float64)
            elif kind == MIN:
                T[:, o] = from_keys(keys[:, 0])
            elif kind == MAX:
                T[:, o] = from_keys(keys[:, -1])
            elif kind == QUANTILE:
                T[:, o] = from_keys(keys[:, min(n - 1, int(math.floor(float(n) * arg)))])
            else:
                T[:, o] = (v <= arg).sum(axis=1) / float(n)
            T[has_nan, o] = np.nan
    return T, bound


def restate_counts(T, t_obs):
    with np.errstate(invalid="ignore"):
        return (T > t_obs).sum(axis=0), (T == t_obs).sum(axis=0), np.isnan(T).sum(axis=0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def agrees(got, want, bound, stats, where=""):
    """got [S][nout] against restate()'s: the exact kinds in their bits, mean and sd inside their bounds, NaN where and only where"""
    nstat = len(stats)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    assert np.all(got[np.isnan(got)].view(np.uint64) == np.uint64(0x7ff8000000000000)), where     # the positive quiet NaN
    for o in range(got.shape[1]):
        kind = stats[o % nstat][0]
        g, w = got[:, o], want[:, o]
        ok = ~np.isnan(w)
        if kind in EXACT:
            assert same_bits(g[ok], w[ok]), (where, o, kind)
            continue
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), (where, o, kind)
        fin = ok & ~inf
        assert np.all(np.abs(g[fin] - w[fin]) <= bound[fin, o]), (where, o, kind, np.max(np.abs(g[fin] - w[fin]) - bound[fin, o]))
        exact = fin & (bound[:, o] == 0)                        # all keys equal: the value itself, sd 0
        assert np.array_equal(g[exact], w[exact]), (where, o, kind)


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// ppc_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp) and the kernels' index arithmetic, one workgroup after the
// other; the LDS is exactly the launch's, filled with a pattern before every workgroup and followed by guard words.  y may be NULL.
// Returns 0, -1 beyond a cap, -2 where a workgroup wrote behind its LDS.
static rh_plan::Ppc plan_of(long long chains, long long count, long long thin, const pp_stat *stats, int nstat, int K, const int *seg_off, int nseg) {
  std::vector<int> kinds(nstat);
  for (int k = 0; k < nstat; k++) kinds[k] = stats[k].kind;
  return rh_plan::ppc_plan(chains, count, thin, K, seg_off, nseg, kinds.data(), nstat);
}
extern "C" int pp_emulate(const double *in, int chains, long long iterations, long long nin, long long first, long long count, long long thin, const pp_stat *stats,
                          int nstat, const int *cols, int K, const int *seg_off, int nseg, const double *y, double *T, double *tobs, unsigned long long *counts) {
  const rh_plan::Ppc P = plan_of(chains, count, thin, stats, nstat, K, seg_off, nseg);
  if (P.over_k || P.over_nstat || P.over_nout) return -1;
  std::vector<int> qidx(P.nout, 0);
  for (int g = 0; g < nseg; g++)
    for (int k = 0; k < nstat; k++)
      if (stats[k].kind == PP_QUANTILE) qidx[g * nstat + k] = rh_plan::ppc_qidx(seg_off[g + 1] - seg_off[g], stats[k].arg);
  const size_t words = (size_t)(P.lds_bytes / 8), guard = 64;
  std::vector<rs_key> lds(words + guard);
  bool over = false;
  auto fresh = [&] { for (size_t i = 0; i < lds.size(); i++) lds[i] = 0xabababababababa0ull + i; };
  auto check = [&] { for (size_t i = words; i < lds.size(); i++) over = over || lds[i] != 0xabababababababa0ull + i; };
  if (y) {
    fresh();
    pp_tile_block(y, 1, nin, 1, 1, 0, 1, cols, K, seg_off, nseg, stats, nstat, qidx.data(), P.flags, P.stride, P.team_log2, P.sortp, lds.data(), tobs, PP_BLOCK);
    check();
  }
  for (long long t = 0; t < P.tiles; t++) {
    const long long r0 = t * P.rows;
    if (r0 >= P.S) continue;
    fresh();
    pp_tile_block(in + first * nin, iterations, nin, thin, P.kept, r0, (int)(P.S - r0 < P.rows ? P.S - r0 : P.rows), cols, K, seg_off, nseg, stats, nstat, qidx.data(),
                  P.flags, P.stride, P.team_log2, P.sortp, lds.data(), T, PP_BLOCK);
    check();
  }
  if (y) {
    std::vector<unsigned int> c32((size_t)(P.count_lds / 4) + guard);
    for (int o = 0; o < 3 * P.nout; o++) counts[o] = 0;
    for (long long b = 0; b < P.count_blocks; b++) {
      const long long r0 = b * P.count_rows;
      if (r0 >= P.S) continue;
      for (size_t i = 0; i < c32.size(); i++) c32[i] = 0xabab0000u + (unsigned)i;
      pp_count_block(T, r0, P.S - r0 < P.count_rows ? P.S : r0 + P.count_rows, P.nout, tobs, c32.data(), counts, PP_BLOCK);
      for (size_t i = (size_t)(P.count_lds / 4); i < c32.size(); i++) over = over || c32[i] != 0xabab0000u + (unsigned)i;
    }
  }
  return over ? -2 : 0;
}
extern "C" void pp_plan(long long chains, long long count, long long thin, const pp_stat *stats, int nstat, int K, const int *seg_off, int nseg, long long *out) {
  const rh_plan::Ppc P = plan_of(chains, count, thin, stats, nstat, K, seg_off, nseg);
  const long long v[20] = {P.kept, P.S, P.nout, P.nmax, P.flags, P.team, P.team_log2, P.conc, P.stride, P.rows, P.tiles, P.sortp, P.sort_stride, P.lds_bytes,
                           P.count_rows, P.count_blocks, P.count_lds, P.over_k ? 1 : 0, P.over_nstat ? 1 : 0, P.over_nout ? 1 : 0};
  for (int i = 0; i < 20; i++) out[i] = v[i];
}
extern "C" int pp_qidx(int n, double p) { return rh_plan::ppc_qidx(n, p); }
extern "C" int pp_width_of(int n) { return pp_width(n); }
extern "C" void pp_constants(long long *out) { const long long v[7] = {PP_BLOCK, PP_STAGE, PP_LDS_DOUBLES, PP_MAX_K, PP_MAX_STATS, PP_MAX_OUT, PP_COUNT_ELEMS}; for (int i = 0; i < 7; i++) out[i] = v[i]; }
'''
PLAN_FIELDS = ("kept", "S", "nout", "nmax", "flags", "team", "team_log2", "conc", "stride", "rows", "tiles", "sortp", "sort_stride", "lds_bytes", "count_rows",
               "count_blocks", "count_lds", "over_k", "over_nstat", "over_nout")
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h and rh_ppc.hip.h in host mode) + the driver above as a host shared library
    (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_ppc_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        # (the scratch is keys in one phase and doubles in the next through casts of one pointer, as LDS is: no type-based aliasing)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip, sp = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int), C.POINTER(_capi.PpcStat)
        L.pp_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, sp, C.c_int, ip, C.c_int, ip, C.c_int, dp, dp, dp, C.POINTER(C.c_ulonglong)]
        L.pp_plan.argtypes = [ll, ll, ll, sp, C.c_int, C.c_int, ip, C.c_int, C.POINTER(ll)]
        L.pp_plan.restype = None
        L.pp_qidx.argtypes = [C.c_int, C.c_double]
        L.pp_constants.argtypes = [C.POINTER(ll)]
        _emu = L
    return _emu


def table(stats):
    return (_capi.PpcStat * len(stats))(*[_capi.PpcStat(int(k), 0, float(a)) for k, a in stats])


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def plan(chains, count, thin, stats, off):
    out = (C.c_longlong * 20)()
    o = np.ascontiguousarray(off, dtype=np.int32)
    emulation().pp_plan(chains, count, thin, table(stats), len(stats), int(off[-1]), _ip(o), len(off) - 1, out)
    return dict(zip(PLAN_FIELDS, list(out)))


def emulate(x, cc, off, stats, y=None, first=0, count=None, thin=1):
    """the host emulation over x [chains][iterations][nin] -> dict t_rep [S][nout], and with y t_obs [nout], n_gt, n_eq, n_bad [nout]"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    chains, iterations, nin = x.shape
    count = iterations - first if count is None else count
    c, o = np.ascontiguousarray(cc, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int32)
    nout = (len(off) - 1) * len(stats)
    S = chains * -(-count // thin)
    T = np.full((S, nout), -7.0)
    tobs = np.full(nout, -7.0)
    counts = np.full(3 * nout, 77, dtype=np.uint64)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    rc = emulation().pp_emulate(_capi.dptr(x), chains, iterations, nin, first, count, thin, table(stats), len(stats), _ip(c), len(c), _ip(o), len(off) - 1,
                                None if yy is None else _capi.dptr(yy), _capi.dptr(T), _capi.dptr(tobs), counts.ctypes.data_as(C.POINTER(C.c_ulonglong)))
    assert rc == 0, rc
    out = dict(t_rep=T)
    if yy is not None:
        cnt = counts.astype(np.int64).reshape(3, nout)
        out.update(t_obs=tobs, n_gt=cnt[0], n_eq=cnt[1], n_bad=cnt[2])
    return out


_cases = {}


def emulated_case(i):
    """case(i) and the emulation's result, computed once and shared (the GPU tests compare with it)"""
    if i not in _cases:
        x, base, touched, cc, off, stats, first, count, thin, y = case(i)
        _cases[i] = (x, base, touched, cc, off, stats, first, count, thin, y, emulate(x, cc, off, stats, y, first, count, thin))
    return _cases[i]


# ---- lowering ------------------------------------------------------------------------------------------------------------------------
def test_the_code_object_lowers_for_gfx950_without_scratch_or_spills():
    code = _capi.ppc_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r        # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.ppc.co")))     # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.ppc_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before       # served by the kernel cache
    for other in (_capi.summary_lower_only, _capi.loo_lower_only):
        assert not any(k.encode() in other("gfx950") for k in KERNELS)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_the_plan():
    k = (C.c_longlong * 7)()
    emulation().pp_constants(k)
    assert list(k) == [BLOCK, STAGE, LDS_DOUBLES, CAP, MAX_STATS, MAX_OUT, 8192]
    width = lambda n: emulation().pp_width_of(n)
    assert [width(n) for n in (1, 16, 17, 32, 33, 434, 2048, 2049, 4096)] == [1, 1, 2, 2, 4, 32, 128, 256, 256]
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 434, CAP - 1, CAP):
        for stats in (SIX, [(MEAN, 0.0)]):
            p = plan(1, 1000, 1, stats, [0, n])
            assert p["rows"] == tile_rows(n) and p["tiles"] == -(-1000 // p["rows"]) and p["team"] == width(n) == 1 << p["team_log2"] and p["conc"] * p["team"] == BLOCK
            assert p["rows"] * p["stride"] <= STAGE and p["stride"] >= n and (p["stride"] % 2 == 1 or p["rows"] == 1)
            sort = stats is SIX
            assert p["flags"] == (7 if sort else 1) and p["sortp"] == (max(1, 1 << (n - 1).bit_length()) if sort else 0)
            assert p["conc"] * p["sort_stride"] <= LDS_DOUBLES - STAGE and p["sort_stride"] >= p["sortp"]
            assert p["lds_bytes"] == 8 * (p["rows"] * p["stride"] + max(2 * BLOCK + 3 * p["conc"], p["conc"] * p["sort_stride"])) <= 8 * LDS_DOUBLES
    # KidIQ's shapes and the narrow one: eight rows with a team of 32 lanes each; nine rows with teams of four; a lane per draw
    a = plan(1024, 200, 1, SIX, [0, 434])
    b = plan(1024, 200, 1, SIX, [0] + list(np.cumsum(KIDIQ_SEGS)))
    c = plan(1024, 1000, 1, SIX, [0, 8])
    assert (a["rows"], a["team"], a["tiles"], a["nout"]) == (8, 32, 25600, 6) and (b["rows"], b["team"], b["nout"]) == (9, 4, 60)
    assert (c["rows"], c["team"], c["tiles"], c["lds_bytes"]) == (256, 1, 4000, 8 * (256 * 9 + 256 * 9))
    assert plan(2, 26, 3, SIX, [0, 8])["kept"] == 9 and plan(2, 26, 3, SIX, [0, 8])["S"] == 18
    # the order statistic: precis' rule, in double
    q = emulation().pp_qidx
    assert [q(10, p) for p in (0.0, 0.05, 0.5, 0.999, 1.0)] == [0, 0, 5, 9, 9] and q(1, 0.7) == 0 and q(434, 0.5) == 217
    assert q(10, 0.3) == int(math.floor(10.0 * 0.3)) == 3 and q(10, 0.7) == int(math.floor(10.0 * 0.7)) == 7
    # the caps, from the shape alone
    assert plan(1, 1, 1, SIX, [0, CAP + 1])["over_k"] == 1 and plan(1, 1, 1, SIX, [0, CAP])["over_k"] == 0
    assert plan(1, 1, 1, SIXTEEN + [(MEAN, 0.0)], [0, 4])["over_nstat"] == 1
    assert plan(1, 1, 1, SIXTEEN, list(range(258)))["over_nout"] == 1 and plan(1, 1, 1, SIXTEEN, list(range(257)))["over_nout"] == 0


# ---- emulation against restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)))
def test_emulation_against_the_restatement(i):
    x, base, touched, cc, off, stats, first, count, thin, y, emu = emulated_case(i)
    rows = kept_rows(x, first, count, thin)
    want, bound = restate(rows, cc, off, stats)
    agrees(emu["t_rep"], want, bound, stats, CASES[i][:3])
    want_obs, bound_obs = restate(y[None, :], cc, off, stats)
    agrees(emu["t_obs"][None, :], want_obs, bound_obs, stats, "t_obs")
    # the counts: a restatement of the comparisons over the emulation's own T, and over the restated T for the exact kinds
    gt, eq, bad = restate_counts(emu["t_rep"], emu["t_obs"])
    assert np.array_equal(emu["n_gt"], gt) and np.array_equal(emu["n_eq"], eq) and np.array_equal(emu["n_bad"], bad)
    gt, eq, bad = restate_counts(want, want_obs[0])
    exact = [o for o in range(want.shape[1]) if stats[o % len(stats)][0] in EXACT]
    assert np.array_equal(emu["n_gt"][exact], gt[exact]) and np.array_equal(emu["n_eq"][exact], eq[exact])
    assert np.array_equal(emu["n_bad"], bad)
    S = rows.shape[0]
    nan_obs = np.isnan(emu["t_obs"])
    assert np.all(emu["n_eq"][~nan_obs] >= 1)                    # y is one of the draws
    assert np.all(emu["n_gt"][nan_obs] == 0) and np.all(emu["n_eq"][nan_obs] == 0)
    assert np.all(emu["n_gt"] + emu["n_eq"] + emu["n_bad"] <= S)
    # without y the statistics are the same and nothing else is asked for
    assert same_bits(emulate(x, cc, off, stats, None, first, count, thin)["t_rep"], emu["t_rep"])


@pytest.mark.parametrize("i", [j for j in range(len(CASES)) if CASES[j][1] is not None or CASES[j][2] is not None or CASES[j][0] in (3, 65, 434)])
def test_the_special_rows_touch_their_own_draw_and_segment_only(i):
    x, base, touched, cc, off, stats, first, count, thin, y, emu = emulated_case(i)
    plain = emulate(base, cc, off, stats, None, first, count, thin)["t_rep"]
    nstat = len(stats)
    same = np.ones(plain.shape, dtype=bool)
    for r, g in touched:
        same[r, g * nstat:(g + 1) * nstat] = False
    assert np.array_equal(plain.view(np.uint64)[same], emu["t_rep"].view(np.uint64)[same])
    kinds = np.array([k for k, _ in stats] * (len(off) - 1))
    single = np.repeat(np.diff(off) == 1, nstat)
    assert np.array_equal(np.isnan(plain), np.broadcast_to((kinds == SD) & single, plain.shape))      # NaN: the sd of one value, nothing else
    S = plain.shape[0]
    if S > 0:                                                   # r = 0: the constant segment
        t = emu["t_rep"][0, :nstat]
        for k, (kind, arg) in enumerate(stats):
            want = {MEAN: 3.7, SD: 0.0 if off[1] > 1 else np.nan, MIN: 3.7, MAX: 3.7, QUANTILE: 3.7, FRAC_LE: 1.0 if 3.7 <= arg else 0.0}[kind]
            assert same_bits(t[k], want), (k, kind, t[k])
    if S > 1:                                                   # r = 1: -0.0 sorts before +0.0
        g = len(off) - 2
        t = emu["t_rep"][1, g * nstat:(g + 1) * nstat]
        n = off[g + 1] - off[g]
        for k, (kind, arg) in enumerate(stats):
            if kind == MIN and n >= 2:
                assert same_bits(t[k], -0.0)
            if kind == MAX:
                assert same_bits(t[k], 0.0)
            if kind == FRAC_LE:
                assert t[k] == (1.0 if 0.0 <= arg else 0.0)
    if S > 2:                                                   # r = 2: a NaN gives NaN in every statistic of the segment
        assert np.all(np.isnan(emu["t_rep"][2, :nstat]))
    if S > 3 and off[1] > 1:                                    # r = 3: +inf follows IEEE arithmetic
        t = emu["t_rep"][3, :nstat]
        for k, (kind, arg) in enumerate(stats):
            if kind in (MEAN, MAX) or (kind == QUANTILE and arg == 1.0):
                assert t[k] == np.inf
            if kind == SD:
                assert np.isnan(t[k])
            if kind == MIN:
                assert np.isfinite(t[k])
    assert kinds.size == plain.shape[1]


def test_a_sum_depends_on_the_length_of_its_segment_alone():
    """the same 43 values as a segment of their own, as one of ten segments, in another place of a wider selection, under another table
    and in a window: the same bits in mean and sd"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 30, 434)) * 1e3 + 7.0
    cols43 = list(range(197, 240))
    alone = emulate(x[:, :, 197:240], list(range(43)), [0, 43], [(MEAN, 0.0), (SD, 0.0)])["t_rep"]
    cc, off = selection(434, None, kidiq_segments())
    ten = emulate(x, cc, off, SIX)["t_rep"]
    assert cc[off[4]:off[5]] == cols43
    assert same_bits(ten[:, 4 * 6:4 * 6 + 2], alone)
    moved = emulate(x, [0, 1, 2] + cols43 + list(range(300, 434)), [0, 3, 46, 180], SIXTEEN)["t_rep"]
    assert same_bits(moved[:, 16:18], alone) and same_bits(moved[:, 16 + 13], alone[:, 0])
    win = emulate(x, cols43, [0, 43], [(SD, 0.0)], None, 3, 20, 3)["t_rep"]
    assert same_bits(win[:, 0], alone.reshape(2, 30, 2)[:, 3:23:3, 1].reshape(-1))


def test_duplicates_and_reordered_segments_give_the_corresponding_outputs():
    x = base_buffer(40, 2, 25, 9)
    segs = five_segments()
    cc, off = selection(40, None, segs)
    a = emulate(x, cc, off, SIX)["t_rep"]
    order = [3, 0, 4, 2, 1, 3]
    cc2, off2 = selection(40, None, [segs[g] for g in order])
    b = emulate(x, cc2, off2, SIX)["t_rep"]
    for at, g in enumerate(order):
        assert same_bits(b[:, at * 6:(at + 1) * 6], a[:, g * 6:(g + 1) * 6])
    # a column twice: the statistics of the doubled values; min, max and the share are the single column's
    one = emulate(x, [18], [0, 1], [(MIN, 0.0), (MAX, 0.0), (FRAC_LE, 0.0)])["t_rep"]
    two = emulate(x, [18, 18], [0, 2], [(MIN, 0.0), (MAX, 0.0), (FRAC_LE, 0.0), (SD, 0.0), (MEAN, 0.0)])["t_rep"]
    assert same_bits(two[:, :3], one) and np.all(two[:, 3] == 0.0) and same_bits(two[:, 4], x.reshape(-1, 40)[:, 18])


# ---- what the figures mean -----------------------------------------------------------------------------------------------------------
def phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def test_what_the_figures_mean():
    """rows of n = 10 iid N(0, 1), S = 20000: P(mean >= 0.2) = 1 - Phi(0.2 sqrt(10)) and P(max >= 1.5) = 1 - Phi(1.5)^10, each within four
    binomial standard errors.  (The numpy restatement alone meets both with this seed: it is asserted first.)"""
    S, n = 20000, 10
    x = np.random.default_rng(1996).standard_normal((4, S // 4, n))
    y = np.array([1.5] + [(0.2 * n - 1.5) / (n - 1)] * (n - 1))
    stats = [(MEAN, 0.0), (MAX, 0.0)]
    p_mean, p_max = 1.0 - phi(0.2 * math.sqrt(n)), 1.0 - phi(1.5) ** n
    se = lambda p: math.sqrt(p * (1.0 - p) / S)
    rows = x.reshape(S, n)
    assert abs(np.mean(rows.mean(axis=1) >= y.mean()) - p_mean) <= 4 * se(p_mean) and abs(np.mean(rows.max(axis=1) >= 1.5) - p_max) <= 4 * se(p_max)
    emu = emulate(x, list(range(n)), [0, n], stats, y)
    assert abs(emu["t_obs"][0] - 0.2) <= 1e-15 and emu["t_obs"][1] == 1.5
    res = R.Ppc(emu["t_obs"].reshape(1, 2), emu["n_gt"].reshape(1, 2), emu["n_eq"].reshape(1, 2), emu["n_bad"].reshape(1, 2), None, 0, S)
    assert abs(res.p_ge[0, 0] - p_mean) <= 4 * se(p_mean) and abs(res.p_ge[0, 1] - p_max) <= 4 * se(p_max)
    assert np.all(res.n_bad == 0) and np.all(res.n_eq == 0) and np.array_equal(res.p_ge, res.p_gt)
    # y taken from one of the rows: at least that draw is equal, and for a statistic without ties the three p-values are apart
    emu = emulate(x, list(range(n)), [0, n], stats, rows[4321])
    res = R.Ppc(emu["t_obs"].reshape(1, 2), emu["n_gt"].reshape(1, 2), emu["n_eq"].reshape(1, 2), emu["n_bad"].reshape(1, 2), None, 0, S)
    assert np.all(res.n_eq >= 1) and np.all(res.p_gt < res.p_mid) and np.all(res.p_mid < res.p_ge)
    assert np.allclose(res.p_mid, (res.n_gt + 0.5 * res.n_eq) / S)
    # no draw is a number, or no y: NaN
    nanrow = R.Ppc(np.zeros((1, 1)), np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1), dtype=np.int64), np.full((1, 1), 5, dtype=np.int64), None, 0, 5)
    assert np.isnan(nanrow.p_ge[0, 0]) and np.isnan(nanrow.p_mid[0, 0]) and np.isnan(R.Ppc(None, None, None, None, None, 0, 5).p_ge)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def _create(stats, nin, cols=None, k=None, off=None, nseg=None):
    """rh_ppc_create -> (rc, message, handle)"""
    L = _capi.lib()
    h = C.c_void_p()
    keep = [np.ascontiguousarray(a, dtype=np.int32) for a in (cols, off) if a is not None]
    pc = None if cols is None else keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    po = None if off is None else keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.rh_ppc_create(table(stats) if stats else None, len(stats) if stats is not None else 0, pc, (0 if cols is None else len(cols)) if k is None else k, po,
                         (0 if off is None else len(off) - 1) if nseg is None else nseg, nin, -1, C.byref(h))
    return rc, (L.rh_last_error(None) or b"").decode(), h


def test_create_refuses_a_bad_table_and_names_the_entry():
    L = _capi.lib()
    bad = [
        (dict(stats=[(MEAN, 0.0), (9, 0.0)], nin=4), "statistic 1: unknown kind 9"),
        (dict(stats=[(MEAN, 0.0), (-1, 0.0)], nin=4), "statistic 1: unknown kind -1"),
        (dict(stats=[(QUANTILE, 1.5)], nin=4), "statistic 0 (QUANTILE): the probability"),
        (dict(stats=[(MEAN, 0.0), (QUANTILE, -0.1)], nin=4), "statistic 1 (QUANTILE)"),
        (dict(stats=[(QUANTILE, float("nan"))], nin=4), "statistic 0 (QUANTILE)"),
        (dict(stats=[(SD, 0.0), (MIN, 0.0), (FRAC_LE, float("inf"))], nin=4), "statistic 2 (FRAC_LE): the threshold"),
        (dict(stats=[(FRAC_LE, float("nan"))], nin=4), "statistic 0 (FRAC_LE)"),
        (dict(stats=[(MAX, 0.5)], nin=4), "statistic 0 (MAX): the kind takes no argument"),
        (dict(stats=SIX, nin=4, cols=[0, 4]), "cols[1] = 4 is outside 0 .. 3"),
        (dict(stats=SIX, nin=4, cols=[-1]), "cols[0] = -1"),
        (dict(stats=SIX, nin=4, k=3), "K must be"),
        (dict(stats=SIX, nin=4, cols=[1], k=0), "K must be"),
        (dict(stats=SIX, nin=0), "nin must be at least 1"),
        (dict(stats=SIX, nin=4, off=[1, 4]), "seg_off[0] = 1 must be 0"),
        (dict(stats=SIX, nin=4, off=[0, 2, 2, 4]), "seg_off[2] = 2 must be above seg_off[1] = 2"),
        (dict(stats=SIX, nin=4, off=[0, 3, 2, 4]), "seg_off[2] = 2"),
        (dict(stats=SIX, nin=4, off=[0, 2, 5]), "seg_off[2] = 5"),
        (dict(stats=SIX, nin=4, off=[0, 2, 3]), "seg_off[2] = 3 must be K = 4"),
        (dict(stats=SIX, nin=4, nseg=2), "nseg must be"),
    ]
    for kw, text in bad:
        rc, msg, h = _create(**kw)
        assert rc == RH_E_INVALID and text in msg and msg.startswith("rh_ppc_create: ") and not h, (kw, rc, msg)
    res = (C.c_int32 * 4)(MEAN, 1, 0, 0)                          # reserved != 0
    h = C.c_void_p()
    assert L.rh_ppc_create(C.cast(res, C.POINTER(_capi.PpcStat)), 1, None, 0, None, 0, 4, -1, C.byref(h)) == RH_E_INVALID
    assert b"statistic 0 (MEAN): reserved must be 0" in L.rh_last_error(None)
    assert L.rh_ppc_create(None, 1, None, 0, None, 0, 4, -1, C.byref(h)) == RH_E_INVALID and L.rh_ppc_create(table(SIX), 6, None, 0, None, 0, 4, -1, None) == RH_E_INVALID
    assert _create(stats=[], nin=4)[0] == RH_E_INVALID
    # the caps: refused from the shape alone
    for kw, text in [(dict(stats=SIX, nin=CAP + 1), "4097 selected columns"), (dict(stats=SIX, nin=3, cols=[0] * (CAP + 1)), "4097 selected columns"),
                     (dict(stats=SIXTEEN + [(MEAN, 0.0)], nin=4), "17 statistics"), (dict(stats=SIXTEEN, nin=300, off=list(range(257)) + [300]), "4112 outputs")]:
        rc, msg, h = _create(**kw)
        assert rc == RH_E_UNSUPPORTED and text in msg and not h, (kw, rc, msg)
    for kw, nout in [(dict(stats=SIX, nin=CAP), 6), (dict(stats=SIXTEEN, nin=300, off=list(range(256)) + [300]), 4096), (dict(stats=[(MIN, 0.0)], nin=3, cols=[2, 2, 0], off=[0, 1, 3]), 2)]:
        rc, msg, h = _create(**kw)
        assert rc == 0 and L.rh_ppc_nout(h) == nout, (kw, rc, msg)
        L.rh_ppc_destroy(h)
    assert L.rh_ppc_nout(None) == -1
    L.rh_ppc_destroy(None)


def test_the_calls_refuse_bad_arguments_and_do_not_compute_without_a_device():
    L = _capi.lib()
    chk = R.Check([R.ppc.mean(), R.ppc.sd(), R.ppc.min(), R.ppc.max(), R.ppc.quantile(0.5), R.ppc.frac_le(0.0)], 8, segments=[[0, 1, 2], [3, 4, 5, 6, 7]])
    assert (chk.nin, chk.nseg, chk.nstat, chk.nout) == (8, 2, 6, 12)
    fake = C.c_void_p(4096)
    y, t_obs = np.zeros(8), np.zeros(12)
    cnt = [np.zeros(12, dtype=np.int64) for _ in range(3)]
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    full = lambda **kw: L.rh_ppc_device(kw.get("h", chk._h), kw.get("ptr", fake), 0, kw.get("chains", 2), kw.get("iters", 10), kw.get("nin", 8), kw.get("first", 0),
                                        kw.get("count", 10), kw.get("thin", 1), kw.get("y", _capi.dptr(y)), kw.get("t_obs", _capi.dptr(t_obs)), lp(cnt[0]),
                                        kw.get("n_eq", lp(cnt[1])), lp(cnt[2]), None, None)
    msg = lambda: L.rh_last_error(None).decode()
    assert full(nin=9) == RH_E_INVALID and "the buffer has 9 columns, the check reads 8" in msg()
    for kw in (dict(first=-1), dict(first=5, count=6), dict(count=0), dict(thin=0), dict(chains=0)):
        assert full(**kw) == RH_E_INVALID and "window" in msg(), kw
    for kw in (dict(ptr=None), dict(h=None), dict(t_obs=None), dict(n_eq=None)):
        assert full(**kw) == RH_E_INVALID and "NULL" in msg(), kw
    # (the fake pointer is never dereferenced: every case above is refused before the first device call, and the ones below run only
    # where there is no device to hand it to)
    if L.rh_device_count() == 0:
        assert full(y=None, t_obs=None, n_eq=None) == RH_E_DEVICE   # without y the outputs may be NULL; and no device here
        assert full() == RH_E_DEVICE and "no CPU fallback" in msg()
        with pytest.raises(R.RainierHipError) as e:
            R.ppc_device(chk, 4096, 2, 10, 8)
        assert e.value.code == RH_E_DEVICE
    with pytest.raises(ValueError):
        R.ppc_device(chk, 4096, 2, 10, 8, y=np.zeros(7))
    with pytest.raises(ValueError):
        R.Check([R.ppc.mean()], 8, cols=[0], segments=[[0]])
    # the sampler form: a generator whose width is not the check's is refused before anything else is looked at; then the NULLs
    g = R.Generator([R.gen.Normal(R.gen.col(0), 1.0)] * 3, 1)
    sampler = lambda gh, hh: L.rh_sampler_ppc(None, None, gh, hh, 1, 0, 0, 10, 1, None, None, None, None, None, None, None)
    assert sampler(g._h, chk._h) == RH_E_INVALID and "the generator has 3 outputs, the check reads 8 columns" in msg()
    g8 = R.Generator([R.gen.Normal(R.gen.col(0), 1.0)] * 8, 1)
    assert sampler(g8._h, chk._h) == RH_E_INVALID and "NULL" in msg()
    assert sampler(None, chk._h) == RH_E_INVALID and sampler(g8._h, None) == RH_E_INVALID


def test_the_abi_and_the_python_surface():
    import inspect
    import re
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "rainier_hip.h")).read()
    names = {"rh_ppc_create", "rh_ppc_destroy", "rh_ppc_nout", "rh_ppc_device", "rh_sampler_ppc", "rh_ppc_lower_only"}
    assert set(re.findall(r"\b(rh_[a-z_]*ppc[a-z_]*)\s*\(", hdr)) == names
    for name in names:
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert C.sizeof(_capi.PpcStat) == 16
    assert R.Ppc._fields == ("t_obs", "n_gt", "n_eq", "n_bad", "t_rep", "dev_ptr", "S")
    assert list(inspect.signature(R.Check.__init__).parameters) == ["self", "stats", "nin", "cols", "segments", "device"]
    assert list(inspect.signature(R.ppc_device).parameters) == ["check", "ptr", "chains", "iterations", "nin", "y", "first", "count", "thin", "device", "to_host"]
    assert list(inspect.signature(R.Sampler.ppc).parameters) == ["self", "predictor", "generator", "check", "seed", "y", "first", "count", "thin", "to_host"]
    kinds = [s.kind for s in (R.ppc.mean(), R.ppc.sd(), R.ppc.min(), R.ppc.max(), R.ppc.quantile(0.25), R.ppc.frac_le(2.0))]
    assert kinds == [MEAN, SD, MIN, MAX, QUANTILE, FRAC_LE] and R.ppc.quantile(0.25).arg == 0.25 and R.ppc.frac_le(2.0).arg == 2.0 and R.ppc.sd().arg == 0.0
