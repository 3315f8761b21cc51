"""Posterior covariance and correlation on the device (csrc/device/rh_cov.hip.h: X^T X of the centred draws on the fp64 matrix
cores), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn and
    the MFMA a function that applies fma for k = 0, 1, 2, 3 at the instruction's lane maps, is driven over whole buffers exactly as
    the launches walk them (the workspace cap a parameter of the driver) and compared
      - bit for bit with an exact restatement of the contract written here (every fma through fractions.Fraction), at small N;
      - with an independent reference -- math.fsum for the mean, np.longdouble sums of the products of the centred values formed with
        the RETURNED mean -- at bounds that are derived, not tuned: with u = 2^-53,
            |mean - fsum / N| <= (N + 2) u sum|x| / N                       (N - 1 adds in any order, the division)
            |cov - ref|       <= (N + 4) u sum_r |d_ra d_rb| / (N - 1)      (the centring's rounding in either factor, N fused
                                                                             multiply-adds and S - 1 adds in any order, the division)
        A dropped or doubled row is off by about 1 / N of that sum: more than eight orders above the bound at these sizes;
  * the properties of the contract (bitwise symmetry, the bits of a sub-matrix for a shuffled column list with a duplicate, corr
    recomputed from the returned cov, a NaN column touching nothing else, chunking not being part of the result), the plan's
    arithmetic, the C ABI's argument errors and its refusal to compute without a device.

tests/test_gpu_covariance_device.py runs the same fixtures through the kernels.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_cov_mean_kernel", "rh_cov_tile_kernel", "rh_cov_finish_kernel")
SMALL_KERNELS = ("rh_cov_mean_finish_kernel", "rh_cov_corr_kernel")
SPLIT, TC, CAP = 4096, 64, 128 << 20
U53 = 2.0 ** -53
LD = np.longdouble


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
NKINDS = 4


def fixture(chains, iters, nvars, seed, nan_col=None):
    """[chains][iters][nvars]; column p is of kind p % 4: 0 a standard normal scaled by 1 + p / 7, 1 a standard normal moved by 1e6
    standard deviations, 2 the pair 0.9 * (column p - 2) + noise of sd 0.3, 3 the constant 2.0 (variance exactly 0).
    nan_col: that column holds one NaN"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((chains, iters, nvars))
    for p in range(nvars):
        kind = p % NKINDS
        if kind == 0:
            x[:, :, p] *= 1.0 + p / 7.0
        elif kind == 1:
            x[:, :, p] += 1e6
        elif kind == 2:
            x[:, :, p] = 0.9 * x[:, :, p - 2] + 0.3 * x[:, :, p]
        else:
            x[:, :, p] = 2.0
    if nan_col is not None:
        x[chains // 2, iters // 3, nan_col] = np.nan
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
    """(chains, kept) with chains * kept == n: three chains where 3 divides n (4095, 8193: splits straddle chain boundaries), else
    the smallest other odd divisor, else two chains"""
    for m in (3, 5, 7, 17, 241, 2):
        if n % m == 0 and n // m >= 1:
            return m, n // m
    return 1, n


# ---- the independent reference and the derived bounds ---------------------------------------------------------------------------------
def check_bounds(rows, mean, cov, what, entries=None):
    """rows [N][K] (the pooled, selected draws); entries: the (a, b) to check (None: all).  A column that holds a NaN: its mean and
    its row and column of cov must be NaN"""
    n, k = rows.shape
    bad = np.isnan(rows).any(axis=0)
    for p in range(k):
        if bad[p]:
            assert np.isnan(mean[p]), (what, "mean of a NaN column", p)
            continue
        col = rows[:, p].tolist()
        ref = math.fsum(col) / n
        bound = (n + 2) * U53 * math.fsum(map(abs, col)) / n
        assert abs(mean[p] - ref) <= bound, (what, "mean", p, mean[p], ref, bound)
    if cov is None:
        return
    if entries is None:
        good = np.where(~bad)[0]
        d = rows[:, good].astype(LD) - np.asarray(mean)[good].astype(LD)
        ref = (d.T @ d) / LD(n - 1)
        bound = LD((n + 4) * U53) * (np.abs(d).T @ np.abs(d)) / LD(n - 1)
        got = np.asarray(cov)[np.ix_(good, good)].astype(LD)
        err = np.abs(got - ref)
        assert np.all(err <= bound), (what, "cov", np.argwhere(~(err <= bound))[:4], float(np.max(err - bound)))
        assert np.all(np.isnan(np.asarray(cov)[bad, :])) and np.all(np.isnan(np.asarray(cov)[:, bad])), (what, "the NaN column's row and column")
        return
    for a, b in entries:
        if bad[a] or bad[b]:
            assert np.isnan(cov[a][b]), (what, a, b)
            continue
        da, db = rows[:, a].astype(LD) - LD(mean[a]), rows[:, b].astype(LD) - LD(mean[b])
        ref = np.sum(da * db) / LD(n - 1)
        bound = LD((n + 4) * U53) * np.sum(np.abs(da * db)) / LD(n - 1)
        assert abs(LD(cov[a][b]) - ref) <= bound, (what, "cov", a, b, cov[a][b], float(ref), float(bound))


def corr_of(cov, cols=None):
    """the contract's correlation from a finished covariance, in numpy: IEEE operations in the contract's order; an entry whose two
    columns are one parameter (the diagonal, a column that the list names twice) is a diagonal entry of the whole matrix"""
    cov = np.asarray(cov)
    cols = np.arange(len(cov)) if cols is None else np.asarray(cols)
    v = np.diag(cov).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(v)
        out = cov / (sd[:, None] * sd[None, :])
    same = cols[:, None] == cols[None, :]
    out[same] = np.broadcast_to(np.where(np.isfinite(v) & (v > 0.0), 1.0, np.nan)[:, None], out.shape)[same]
    return out


def same_bits(a, b):
    """NaN matches NaN, -0.0 does not match +0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)))


def check_properties(mean, cov, corr, what, cols=None):
    """what holds for every result: bitwise symmetry, corr from the returned cov bit for bit"""
    assert same_bits(cov, np.asarray(cov).T), (what, "cov is not bitwise symmetric")
    if corr is not None:
        assert same_bits(corr, np.asarray(corr).T), (what, "corr is not bitwise symmetric")
        assert same_bits(corr, corr_of(cov, cols)), (what, "corr is not the contract's function of the returned cov")


def check_constant_columns(rows, mean, cov, corr, what):
    """a constant column: mean exact, variance exactly 0, its corr row and diagonal NaN"""
    for p in range(rows.shape[1]):
        if np.all(rows[:, p] == rows[0, p]):
            assert mean[p] == rows[0, p] and cov[p][p] == 0.0 and not np.signbit(cov[p][p]), (what, p, mean[p], cov[p][p])
            assert np.all(np.asarray(cov)[p, ~np.isnan(np.asarray(cov)[p])] == 0.0)
            if corr is not None:
                assert np.all(np.isnan(np.asarray(corr)[p, :])) and np.all(np.isnan(np.asarray(corr)[:, p])), (what, p)


# ---- the contract restated exactly ---------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                                   # a NaN or an infinity: what IEEE arithmetic gives, fused or not
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding (an exact zero is +0.0 in round-to-nearest; acc is never -0.0)


def exact_contract(rows):
    """rows [N][K] -> mean, cov, corr by the contract, one IEEE operation at a time"""
    n, k = rows.shape
    splits = [range(s, min(s + SPLIT, n)) for s in range(0, n, SPLIT)]
    mean = np.zeros(k)
    for p in range(k):
        tot = 0.0
        for sp in splits:
            acc = 0.0
            for r in sp:
                acc = acc + float(rows[r, p])
            tot = tot + acc
        mean[p] = tot / float(n)
    d = rows - mean                                        # one rounding per element
    cov = np.zeros((k, k))
    for a in range(k):
        for b in range(k):
            tot = 0.0
            for sp in splits:
                acc = 0.0
                for r in sp:
                    acc = _fma(float(d[r, a]), float(d[r, b]), acc)
                tot = tot + acc
            cov[a, b] = tot / float(n - 1)
    return mean, cov, corr_of(cov)


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// covariance_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter) and the kernels' index arithmetic, one workgroup after the other
extern "C" int rc_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count,
                          long long thin, const int *cols, int K, long long cap, double *mean, double *cov, double *corr) {
  const rh_plan::Covariance P = rh_plan::covariance_plan(chains, count, thin, K, cap);
  if (P.over_cap) return -1;
  const double *base = draws + first * nvars;
  const long long tile = RC_TC * RC_TC;
  std::vector<double> part((size_t)(P.S * K)), ws((size_t)(P.pc * P.S * tile)), lds(RC_TILE_LDS);
  for (long long bid = 0; bid < P.S * P.ctiles; bid++) {
    const long long s = bid / P.ctiles, ct = bid - s * P.ctiles;
    rc_mean_split(base, iterations, nvars, thin, P.kept, P.N, cols, K, (int)ct * RC_TC, s, lds.data(), part.data(), RC_BLOCK);
  }
  for (int k = 0; k < K; k++) mean[k] = rc_mean_finish(part.data(), P.S, K, k, P.N);
  int chunks = 0;
  for (long long p0 = 0; p0 < P.pairs; p0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < P.pairs - p0 ? P.pc : P.pairs - p0;
    for (long long bid = 0; bid < p_cnt * P.S; bid++) {
      const long long pl = bid / P.S, s = bid - pl * P.S;
      int bi, bj;
      rc_pair_of(p0 + pl, (int)P.ctiles, &bi, &bj);
      rc_tile_split(base, iterations, nvars, thin, P.kept, P.N, cols, K, mean, bi, bj, s, lds.data(), ws.data() + (pl * P.S + s) * tile, RC_BLOCK);
    }
    for (long long pl = 0; pl < p_cnt; pl++) {
      int bi, bj;
      rc_pair_of(p0 + pl, (int)P.ctiles, &bi, &bj);
      rc_finish_pair(ws.data() + pl * P.S * tile, P.S, P.N, bi, bj, K, cov, RC_BLOCK);
    }
  }
  for (long long e = 0; e < (long long)K * K; e++) corr[e] = rc_corr_entry(cov, cols, K, e / K, e - e / K * K);
  return chunks;
}
// kept, N, S, ctiles, pairs, per_pair, pc, over_cap
extern "C" void rc_plan(long long chains, long long count, long long thin, long long K, long long cap, long long *out) {
  const rh_plan::Covariance P = cap ? rh_plan::covariance_plan(chains, count, thin, K, cap) : rh_plan::covariance_plan(chains, count, thin, K);
  const long long v[8] = {P.kept, P.N, P.S, P.ctiles, P.pairs, P.per_pair, P.pc, P.over_cap ? 1 : 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}
extern "C" void rc_pair(long long p, int T, int *out) { rc_pair_of(p, T, out, out + 1); }
// the slot rc_operand reads, through the device text's own function: a block that holds its own indices
extern "C" long long rc_operand_slot(int r0, int c0, int lane) {
  static std::vector<double> blk;
  if (blk.empty()) for (int i = 0; i < RC_TILE_LDS; i++) blk.push_back((double)i);
  return (long long)rc_operand(blk.data(), r0, c0, lane);
}
extern "C" void rc_constants(int *out) { const int v[6] = {RC_BLOCK, RC_SPLIT, RC_TC, RC_SLAB, RC_STRIDE, RC_TILE_LDS}; for (int i = 0; i < 6; i++) out[i] = v[i]; }
// one MFMA as the host mode takes it, over a block filled by the caller: acc [64 lanes][4]
extern "C" void rc_mfma_once(const double *blkA, int ca, const double *blkB, int cb, int r0, double *acc) {
  for (int lane = 0; lane < 64; lane++) {
    rc_d4 d;
    for (int e = 0; e < 4; e++) d[e] = acc[4 * lane + e];
    RC_MFMA(d, blkA, ca, blkB, cb, r0, lane);
    for (int e = 0; e < 4; e++) acc[4 * lane + e] = d[e];
  }
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_cov.hip.h in host mode) + the driver above as a host shared library (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_cov_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int)
        L.rc_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, ll, dp, dp, dp]
        L.rc_plan.argtypes = [ll, ll, ll, ll, ll, C.POINTER(ll)]
        L.rc_pair.argtypes = [ll, C.c_int, ip]
        L.rc_operand_slot.restype = ll
        L.rc_mfma_once.argtypes = [dp, C.c_int, dp, C.c_int, C.c_int, dp]
        _emu = L
    return _emu


def emulate(x, first=0, count=None, thin=1, cols=None, cap=CAP, chunks=False):
    """the host emulation over x [chains][iterations][nvars] -> mean [K], cov [K][K], corr [K][K] (and the number of chunks)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    k = len(sel)
    mean, cov, corr = np.full(k, -1.0), np.full((k, k), -1.0), np.full((k, k), -1.0)
    n = L.rc_emulate(_capi.dptr(x), m, iters, nv, first, count, thin, sel.ctypes.data_as(C.POINTER(C.c_int)), k, cap, _capi.dptr(mean),
                     _capi.dptr(cov), _capi.dptr(corr))
    assert n >= 1, "beyond the cap"
    return (mean, cov, corr, n) if chunks else (mean, cov, corr)


def same_results(a, b):
    return all(same_bits(u, v) for u, v in zip(a[:3], b[:3]))


def plan(chains, count, thin, k, cap=0):
    out = (C.c_longlong * 8)()
    emulation().rc_plan(chains, count, thin, k, cap, out)
    return dict(zip(("kept", "N", "S", "ctiles", "pairs", "per_pair", "pc", "over_cap"), list(out)))


def shuffled_with_duplicate(k, seed):
    """a column list for the sub-matrix property: a shuffle of about two thirds of the columns, one of them twice"""
    rng = np.random.default_rng(seed)
    pick = list(rng.permutation(k)[:max(1, (2 * k) // 3)])
    return [int(c) for c in pick + pick[:1]]


def check_submatrix(full, sub, cols, what):
    """entry (a, b) of the call over cols has the bits of entry (cols[a], cols[b]) of the call over all columns"""
    assert same_bits(sub[0], np.asarray(full[0])[cols]), (what, "mean")
    for q in (1, 2):
        if sub[q] is not None and full[q] is not None:
            assert same_bits(sub[q], np.asarray(full[q])[np.ix_(cols, cols)]), (what, ("cov", "corr")[q - 1])


def _lds_bytes(code, kernel):
    """.group_segment_fixed_size of a kernel: in the metadata's alphabetical order it precedes the kernel's .name"""
    mstr = lambda v: (bytes([0xa0 | len(v)]) if len(v) < 32 else bytes([0xd9, len(v)])) + v.encode()
    at = code.find(mstr(".name") + mstr(kernel))
    k = code.rfind(mstr(".group_segment_fixed_size"), 0, at)
    assert at >= 0 and k >= 0, kernel
    p = code[k + len(mstr(".group_segment_fixed_size")):]
    return p[0] if p[0] <= 0x7f else {0xcc: p[1], 0xcd: (p[1] << 8) | p[2], 0xce: int.from_bytes(p[1:5], "big")}[p[0]]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_covariance_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.covariance_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS + SMALL_KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "" and r["unproven"] == 0, r   # kernel_health: metadata + isacheck's walk
    # the tile kernel: two staged blocks of 32 rows at stride 80 -- 40 KiB, four workgroups in a CU's 160 KiB, within the family's 63 KiB
    assert _lds_bytes(code, "rh_cov_tile_kernel") == 8 * 2 * 32 * 80 <= 63 * 1024 and _lds_bytes(code, "rh_cov_mean_kernel") == 8 * 64 * 64
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.covariance.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.covariance_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_model_sources_do_not_carry_the_covariance_kernels():
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_cov" not in src


def test_lds_banks_of_the_operand_reads_and_the_staging_writes():
    """The LDS bank rule applied to the device text's own operand index: ds_read_b64 is served per 32-lane half over 64 four-byte
    banks, ds_write_b64 per 16 lanes over 32.  Every operand read of every k-group and column offset, and the staging write of a row
    (64 consecutive doubles), touch every bank at most once."""
    L = emulation()
    consts = (C.c_int * 6)()
    L.rc_constants(consts)
    block, split, tc, slab, stride, lds = list(consts)
    assert (block, split, tc, slab, stride, lds) == (256, SPLIT, TC, 32, 80, 2 * 32 * 80) and split % slab == 0 and slab % 4 == 0

    def worst(slots, group, banks):
        w = 1
        for g in range(0, 64, group):
            cnt = {}
            for sl in set(slots[g:g + group]):
                for dw in (2 * sl % banks, (2 * sl + 1) % banks):
                    cnt[dw] = cnt.get(dw, 0) + 1
            w = max(w, max(cnt.values()))
        return w
    for r0 in range(0, slab, 4):
        for c0 in range(0, tc, 16):
            sl = [L.rc_operand_slot(r0, c0, lane) for lane in range(64)]
            assert sl == [(r0 + (lane >> 4)) * stride + c0 + (lane & 15) for lane in range(64)] and max(sl) < slab * stride
            assert worst(sl, 32, 64) == 1, (r0, c0)
    for row in range(slab):
        assert worst([row * stride + c for c in range(64)], 16, 32) == 1


def test_the_host_mfma_is_an_fma_chain_over_k_at_the_instructions_lane_maps():
    """D[i][j] += sum_k A[i][k] B[k][j] with A[i][k] = blkA[r0 + k][ca + i], B[k][j] = blkB[r0 + k][cb + j], k ascending, one fma
    each; lane l holds D[(l >> 4) + 4 reg][l & 15].  Asymmetric integer data: a transposed or misplaced map gives other numbers."""
    L = emulation()
    rng = np.random.default_rng(5)
    stride = 80
    blk_a, blk_b = rng.integers(-9, 10, size=(32, stride)).astype(np.float64), rng.integers(-9, 10, size=(32, stride)).astype(np.float64)
    acc = rng.integers(-5, 6, size=(64, 4)).astype(np.float64)
    r0, ca, cb = 8, 16, 48
    want = np.empty((16, 16))
    for i in range(16):
        for j in range(16):
            lane, reg = (i % 4) * 16 + j, i // 4
            v = acc[lane, reg]
            for k in range(4):
                v = _fma(blk_a[r0 + k, ca + i], blk_b[r0 + k, cb + j], v)
            want[i, j] = v
    got = acc.copy()
    L.rc_mfma_once(_capi.dptr(blk_a), ca, _capi.dptr(blk_b), cb, r0, _capi.dptr(got))
    d = np.array([[got[(i % 4) * 16 + j, i // 4] for j in range(16)] for i in range(16)])
    assert np.array_equal(d, want) and not np.array_equal(d, d.T)
    # ... and the order of k shows in the last bit where the products do not add exactly
    blk_a[r0:r0 + 4, ca] = [1e16, 1.0, -1e16, 1.0]
    blk_b[r0:r0 + 4, cb] = [1.0, 1.0, 1.0, 1.0]
    got = np.zeros((64, 4))
    L.rc_mfma_once(_capi.dptr(blk_a), ca, _capi.dptr(blk_b), cb, r0, _capi.dptr(got))
    assert got[0, 0] == 1.0                                 # ((1e16 + 1) - 1e16) + 1 in double: the first 1 is lost, the last is not


# ---- 2. the device text, on the host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 9])
def test_host_emulation_is_the_contract_bit_for_bit(n):
    chains, kept = shape_for(n)
    for thin in (1, 3):
        first, count, iters = window(kept, thin)
        for k in (1, 2, 3, 5):
            x = fixture(chains, iters, k, 1000 * n + 10 * k + thin)
            got = emulate(x, first, count, thin)
            want = exact_contract(pooled(x, first, count, thin))
            assert same_results(got, want), (n, thin, k, got, want)
            check_properties(*got, (n, thin, k))
    # a NaN and an infinity: the restatement's IEEE arithmetic, entry by entry
    x = fixture(chains, kept, 5, n, nan_col=2)
    x[0, 0, 0] = np.inf
    with np.errstate(invalid="ignore"):
        assert same_results(emulate(x), exact_contract(pooled(x))), n


NS = (4095, 4096, 4097, 8193)
KS = (1, 2, 15, 16, 17, 63, 64, 65, 129)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_host_emulation_within_the_derived_bounds(n, k):
    chains, kept = shape_for(n)
    assert chains == 3 or n % 3
    for thin in (1, 3):
        first, count, iters = window(kept, thin)
        x = fixture(chains, iters, k, 7 * n + 31 * k + thin)
        got = emulate(x, first, count, thin)
        rows = pooled(x, first, count, thin)
        what = (n, k, thin)
        check_bounds(rows, got[0], got[1], what)
        check_properties(*got, what)
        check_constant_columns(rows, *got, what)
    # a window is its rows: the same bits as a (thinned) copy on its own
    assert same_results(emulate(np.ascontiguousarray(x[:, first:first + count:thin, :])), got)
    # the sub-matrix property for a shuffled column list with one duplicate
    cols = shuffled_with_duplicate(k, n + k)
    sub = emulate(x, first, count, thin, cols=cols)
    check_submatrix(got, sub, cols, what)
    check_properties(*sub, what, cols)


def test_a_nan_column_touches_nothing_else():
    for n, k, nan_col in ((4097, 17, 5), (4096, 65, 64), (9, 5, 0)):
        chains, kept = shape_for(n)
        x = fixture(chains, kept, k, n + k, nan_col=nan_col)
        got = emulate(x)
        rows = pooled(x)
        check_bounds(rows, got[0], got[1], ("nan", n, k))
        check_properties(*got, ("nan", n, k))
        others = [c for c in range(k) if c != nan_col]
        without = emulate(x, cols=others)
        check_submatrix(got, without, others, ("nan", n, k))
        assert not np.any(np.isnan(without[1])) and np.isnan(got[0][nan_col])
        assert np.all(np.isnan(got[1][nan_col, :])) and np.all(np.isnan(got[1][:, nan_col]))
        assert np.all(np.isnan(got[2][nan_col, :])) and np.all(np.isnan(got[2][:, nan_col]))


def test_chunking_is_not_part_of_the_result():
    """129 columns are 6 tile pairs and 8193 rows 3 splits (96 KiB of partials per pair): caps of 200 KiB and 96 KiB walk them in
    chunks of two and of one"""
    chains, kept = shape_for(8193)
    x = fixture(chains, kept, 129, 99)
    one = emulate(x, chunks=True)
    assert one[3] == 1
    for cap, want in ((200 << 10, 3), (96 << 10, 6)):
        got = emulate(x, cap=cap, chunks=True)
        assert got[3] == want and same_results(got, one), cap
    assert emulation().rc_emulate(_capi.dptr(x), chains, kept, 129, 0, kept, 1, None, 129, (96 << 10) - 1, None, None, None) == -1


def test_the_plan_is_arithmetic_over_the_headers_constants():
    L = emulation()
    for chains, count, thin, k in ((4, 5000, 1, 2600), (3, 1365, 1, 65), (3, 4100, 3, 1), (1, 2, 1, 129), (1024, 400, 1, 160), (256, 40, 2, 704)):
        kept = -(-count // thin)
        n = chains * kept
        s, t = -(-n // SPLIT), -(-k // TC)
        per = s * TC * TC * 8
        want = dict(kept=kept, N=n, S=s, ctiles=t, pairs=t * (t + 1) // 2, per_pair=per, pc=max(1, min(CAP // per, t * (t + 1) // 2)), over_cap=0)
        assert plan(chains, count, thin, k) == want, (chains, count, thin, k)
    # the GPU tier's shape that crosses the cap: 861 tile pairs of 160 KiB, 819 to a chunk
    p = plan(4, 5000, 1, 2600)
    assert (p["N"], p["S"], p["pairs"], p["per_pair"], p["pc"]) == (20000, 5, 861, 160 << 10, 819) and p["pairs"] * p["per_pair"] > CAP
    # one tile pair alone beyond the cap: more than 4096 splits
    assert plan(4096, 4096, 1, 2)["over_cap"] == 0 and plan(4097, 4096, 1, 2)["over_cap"] == 1 and plan(4097, 4096, 1, 2)["pc"] == 1
    # the pairs in order: (0,0) (0,1) .. (0,T-1) (1,1) ..
    for t in (1, 2, 3, 41):
        want = [(i, j) for i in range(t) for j in range(i, t)]
        out = (C.c_int * 2)()
        got = []
        for p_ in range(len(want)):
            L.rc_pair(p_, t, out)
            got.append((out[0], out[1]))
        assert got == want


# ---- 3. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    mean, cov, corr = np.zeros(8), np.zeros(64), np.zeros(64)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, thin=1, cols=None, ncols=None, outs=(True, True, True)):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        nc = (len(sel) if sel is not None else 0) if ncols is None else ncols
        return L.rh_covariance_device(ptr, 0, chains, iters, nvars, first, count, thin, sel.ctypes.data_as(ip) if sel is not None else None, nc,
                                      *[_capi.dptr(o) if on else None for o, on in zip((mean, cov, corr), outs)])
    err = lambda: L.rh_last_error(None).decode()
    assert call(ptr=None) == _capi.RH_E_INVALID
    assert call(outs=(False, False, False)) == _capi.RH_E_INVALID and "all NULL" in err()
    for first, count, thin in ((0, 0, 1), (0, 11, 1), (5, 6, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):
        assert call(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
        assert "window" in err()
    assert call(nvars=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    # N < 2: one chain and one kept draw, by count or by thinning
    assert call(chains=1, count=1) == _capi.RH_E_INVALID and "at least 2" in err()
    assert call(chains=1, count=10, thin=10) == _capi.RH_E_INVALID and "at least 2" in err()
    for cols in ([2], [-1], [0, 1, 7]):
        assert call(cols=cols) == _capi.RH_E_INVALID and "outside" in err(), cols
    assert call(cols=[0], ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(cols=[0], ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=1) == _capi.RH_E_INVALID and "ncols" in err()            # no list: 0 or nvars
    assert L.rh_sampler_covariance(None, 0, 10, 1, None, 0, _capi.dptr(mean), None, None) == _capi.RH_E_INVALID
    # one tile pair's partials beyond the workspace cap: refused from the shape, whatever the machine; not when only the mean is asked for
    assert call(chains=4097, iters=4096, count=4096) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    assert call(chains=4097, iters=4096, count=4096, outs=(False, False, True)) == _capi.RH_E_UNSUPPORTED
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(ncols=2) == _capi.RH_E_DEVICE and call(cols=[1, 1, 0]) == _capi.RH_E_DEVICE      # valid requests
        assert call(chains=1, count=2, outs=(True, False, False)) == _capi.RH_E_DEVICE
        assert call(chains=4097, iters=4096, count=4096, outs=(True, False, False)) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.covariance_device(4096, 4, 10, 4)


def test_python_surface():
    import inspect
    import rainier_amd as R
    assert list(inspect.signature(R.Sampler.covariance).parameters) == ["self", "first", "count", "thin", "cols", "corr"]
    assert list(inspect.signature(R.covariance_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "thin",
                                                                       "cols", "corr"]
    sig = inspect.signature(R.Sampler.covariance).parameters
    assert sig["first"].default == 0 and sig["count"].default is None and sig["thin"].default == 1 and sig["cols"].default is None
    assert sig["corr"].default is False and R.Covariance._fields == ("mean", "cov", "corr", "cols")
