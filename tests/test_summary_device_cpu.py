"""Posterior summaries on the device (csrc/device/rh_summary.hip.h: segmented sort, order statistics, hdpi, mean and sd), the part
that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the chunk size a parameter of the driver) and compared with a numpy
    restatement of the semantics written here: the key transform on uint64 with np.sort, hdpi as a scan for the first minimum,
    mean and sd with math.fsum.  Sorted keys, order statistics and hdpi: the same bits (NaN matches NaN, -0.0 is not +0.0); mean
    and sd within 1e-12 * (|mean| + sd), the bar the project holds between two summation orders of such moments
    (tests/test_oracle.py:178-179);
  * the C ABI's argument errors, its refusal to compute without a device, and format_precis.

tests/test_gpu_summary_device.py runs the same fixtures through the kernels and asks for the emulation's bits.
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
KERNELS = ("rh_summary_sort_kernel", "rh_summary_merge_kernel", "rh_summary_finish_kernel")
MOMENT_REL = 1e-12
PROBS, HDPI = (0.055, 0.945), 0.89
U = np.uint64
SIGN, ALL, ABS, INF_BITS, QNAN = U(1 << 63), U((1 << 64) - 1), U((1 << 63) - 1), U(0x7FF0000000000000), U(0x7FF8000000000000)


# ---- the semantics, in numpy ---------------------------------------------------------------------------------------------------------
def to_key(x):
    """java.lang.Double.compare's order as unsigned keys: every NaN the positive quiet NaN, negatives all bits flipped, the others
    the sign bit"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).copy()
    b[(b & ABS) > INF_BITS] = QNAN
    return np.where((b >> U(63)) == U(1), b ^ ALL, b ^ SIGN)


def from_key(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> U(63)) == U(1), k ^ SIGN, k ^ ALL).view(np.float64)


def pooled(x, first=0, count=None, thin=1):
    """[nvars][N]: column p = x[c][first + j * thin][p], chain-major, iteration ascending"""
    count = x.shape[1] - first if count is None else count
    sel = x[:, first:first + count:thin, :]
    return np.ascontiguousarray(sel.reshape(-1, x.shape[2]).T)


def hdpi_of_sorted(s, prob):
    """package.scala:327-342 on one sorted column; widths compare in Double.compare's order, the first minimum wins"""
    n = len(s)
    idx = int(math.ceil(prob * n))
    if np.isnan(s[-1]):
        return np.nan, np.nan
    if idx == n:
        return s[0], s[-1]
    with np.errstate(invalid="ignore"):
        w = to_key(s[idx:] - s[:n - idx])
    i = int(np.argmin(w))                                  # the first of the minima
    return s[i], s[i + idx]


def hdpi_loop(s, prob):
    """the same as a loop, for the test that the scan above is the loop"""
    n = len(s)
    idx = int(math.ceil(prob * n))
    if np.isnan(s[-1]):
        return np.nan, np.nan
    if idx == n:
        return s[0], s[-1]
    best, bi = None, None
    for i in range(n - idx):
        with np.errstate(invalid="ignore"):
            w = int(to_key(np.array([s[i + idx] - s[i]]))[0])
        if best is None or w < best:
            best, bi = w, i
    return s[bi], s[bi + idx]


def moments(col):
    """precis' computeParamStats with exact sums; a column that holds an infinity or a NaN: what IEEE arithmetic gives in any order"""
    n = len(col)
    if not np.all(np.isfinite(col)):
        with np.errstate(invalid="ignore"):
            return float(np.sum(col)) / n, np.nan
    mean = math.fsum(col) / n
    return mean, math.sqrt(math.fsum((col - mean) ** 2) / n)


class Reference:
    def __init__(self, x, first=0, count=None, thin=1, probs=PROBS, hdpi=HDPI):
        cols = pooled(x, first, count, thin)
        k, n = cols.shape
        self.keys = np.sort(to_key(cols), axis=1)
        s = from_key(self.keys)
        self.quantiles = s[:, [min(n - 1, int(math.floor(float(n) * q))) for q in probs]]
        self.hdpi = np.array([hdpi_of_sorted(s[p], hdpi) for p in range(k)]) if hdpi else None
        mo = [moments(cols[p]) for p in range(k)]
        self.mean, self.sd = np.array([m for m, _ in mo]), np.array([s_ for _, s_ in mo])


def same_bits(a, b):
    """equal as Double.compare sees them: NaN matches NaN, -0.0 does not match +0.0"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(to_key(a), to_key(b)) and np.array_equal(a[ok], b[ok]) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok])))


def check_against_reference(got, ref, what):
    mean, sd, quant, hdpi = got[:4]
    assert same_bits(quant, ref.quantiles), (what, "quantiles")
    if ref.hdpi is not None:
        assert same_bits(hdpi, ref.hdpi), (what, "hdpi")
    for p in range(len(ref.mean)):
        if np.isfinite(ref.mean[p]) and np.isfinite(ref.sd[p]):
            tol = MOMENT_REL * (abs(ref.mean[p]) + ref.sd[p])
            assert abs(mean[p] - ref.mean[p]) <= tol and abs(sd[p] - ref.sd[p]) <= tol, (what, p, mean[p], ref.mean[p], sd[p], ref.sd[p])
        else:
            assert same_bits(mean[p], ref.mean[p]) and np.isnan(sd[p]), (what, p, mean[p], ref.mean[p], sd[p])


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
NKINDS = 7
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-323, -1e-323, 1.0, -1.0, 2.5, -2.5, 0.0, -0.0])
NANS = np.array([0x7FF8000000000000, 0xFFF8000000000123, 0x7FF8000000000042, 0xFFFC000000000001], dtype=np.uint64).view(np.float64)


def fixture(chains, iters, nvars, seed, offset=0):
    """[chains][iters][nvars]; column p is of kind (p + offset) % 7:
    0 an AR(1) trace moved by 10 marginal sd, 1 an ascending and 2 a descending ramp over the pooled order, 3 a constant (every hdpi
    width is 0: the first minimum wins), 4 an AR(1) trace rounded to multiples of 0.25 (ties among keys and among widths), 5 signed
    zeros, infinities and the smallest subnormals among ordinary values, 6 an AR(1) trace with a few NaNs, two with the sign bit set"""
    rng = np.random.default_rng(seed)
    x = np.empty((chains, iters, nvars))
    ramp = np.arange(chains * iters, dtype=np.float64).reshape(chains, iters)
    phis = np.array([(0.0, 0.5, 0.9)[p % 3] for p in range(nvars)])
    ars = rng.normal(size=(chains, iters, nvars))
    ars[:, 0, :] /= np.sqrt(1 - phis * phis)
    for i in range(1, iters):
        ars[:, i, :] += phis * ars[:, i - 1, :]
    for p in range(nvars):
        kind, phi, ar = (p + offset) % NKINDS, phis[p], ars[:, :, p]
        if kind == 0:
            x[:, :, p] = ar + 10.0 / math.sqrt(1 - phi * phi)
        elif kind == 1:
            x[:, :, p] = ramp * 0.5 - 3.0
        elif kind == 2:
            x[:, :, p] = 1e6 - ramp
        elif kind == 3:
            x[:, :, p] = -7.125
        elif kind == 4:
            x[:, :, p] = np.round(ar * 4.0) / 4.0
        elif kind == 5:
            x[:, :, p] = SPECIALS[rng.integers(0, len(SPECIALS), size=(chains, iters))]
        else:
            col = ar.copy().reshape(-1)
            where = rng.choice(col.size, size=min(4, max(1, col.size // 8)), replace=False)
            col[where] = np.resize(NANS[[1, 3, 0, 2]], len(where))     # the two with the sign bit set first
            x[:, :, p] = col.reshape(chains, iters)
    return x


def tile():
    return emulation().rs_tile()


def n_cases():
    """(chains, kept): N = chains * kept in {1, 2, 63, 64, 65, T-1, T, T+1, 2T+1, 5T+3}; three chains wherever 3 divides N.
    5T+3: six runs -- three merge passes, an odd run count in the second, a ragged last run"""
    T = tile()
    out = []
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3):
        out.append((3, n // 3) if n % 3 == 0 else (1, n))
    # ... and three chains next to 5T+3 (N = 5T+4 at T = 4096): chain-major pooling across tile and run boundaries of a three-pass merge
    out.append((3, (5 * T + 3) // 3 + 1))
    return out


def window(kept, thin):
    """(first, count, iterations) for `kept` kept iterations: a real window at either thinning -- it starts late and ends early --
    and at thin 3 a count that is no multiple of thin"""
    count = kept if thin == 1 else (kept - 1) * thin + 2
    return 2, count, 2 + count + 3


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// summary_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; pc 0: the plan's chunk) and the kernels' index arithmetic, one workgroup after the other
extern "C" int rs_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count,
                          long long thin, long long pc, const double *probs, int nprobs, double hdpi_prob, double *mean, double *sd,
                          double *quant, double *hdpi, rs_key *sorted_out) {
  const rh_plan::Summary P = rh_plan::summary_plan(chains, count, thin, nvars, probs, nprobs, hdpi_prob);
  const long long kept = P.kept, N = P.N;
  if (pc == 0) pc = P.pc;
  std::vector<rs_key> ws((size_t)(2 * pc * N)), lds_sort(RS_TILE_SLOTS), lds_merge(RS_MERGE_LDS), lds_fin(3 * RS_BLOCK);
  for (long long p0 = 0; p0 < nvars; p0 += pc) {
    const int p_lo = (int)p0, p_cnt = (int)(pc < nvars - p0 ? pc : nvars - p0);
    rs_key *src = ws.data(), *dst = src + pc * N;
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
      const long long t = bid / p_cnt, g0 = t * RS_TILE;
      const int pl = (int)(bid - t * p_cnt);
      rs_tile_sort(draws + first * nvars + p_lo + pl, iterations, nvars, thin, kept, N, g0, lds_sort.data(), src + (long long)pl * N + g0, RS_BLOCK);
    }
    for (int k = 0; k < P.passes; k++) {
      const long long L = P.run(k);
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
        const long long t = bid / p_cnt, o0 = t * RS_MERGE_TILE;
        const int pl = (int)(bid - t * p_cnt);
        rs_merge_tile(src + (long long)pl * N, dst + (long long)pl * N, N, L, o0, lds_merge.data(), RS_BLOCK);
      }
      rs_key *t = src; src = dst; dst = t;
    }
    for (int pl = 0; pl < p_cnt; pl++) {
      const int p = p_lo + pl;
      rs_param_finish(src + (long long)pl * N, N, P.idx, nprobs, P.hidx, lds_fin.data(), mean + p, sd + p, quant + (long long)p * nprobs, hdpi + 2 * (long long)p, RS_BLOCK);
      if (sorted_out) for (long long i = 0; i < N; i++) sorted_out[(long long)p * N + i] = src[(long long)pl * N + i];
    }
  }
  return P.passes;
}
extern "C" int rs_tile(void) { return RS_TILE; }
extern "C" int rs_pair_lo_of(int i, int j) { return rs_pair_lo(i, j); }
extern "C" int rs_slot_of(int e) { return RS_SLOT(e); }
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h in host mode) + the driver above as a host shared library (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="rh_summary_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll = C.POINTER(C.c_double), C.c_longlong
        L.rs_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ll, dp, C.c_int, C.c_double, dp, dp, dp, dp, C.POINTER(C.c_uint64)]
        _emu = L
    return _emu


def emulate(x, first=0, count=None, thin=1, probs=PROBS, hdpi=HDPI, pc=0, passes=False):
    """the host emulation over x [chains][iterations][nvars] -> mean, sd, quantiles, hdpi, sorted keys [nvars][N];
    pc: parameters per chunk (0: the engine's)"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, k = x.shape
    count = iters - first if count is None else count
    n = m * (-(-count // thin))
    pr = np.array(probs, dtype=np.float64)
    mean, sd, quant, hd = np.full(k, -1.0), np.full(k, -1.0), np.full((k, len(pr)), -1.0), np.full((k, 2), -1.0)
    keys = np.zeros((k, n), dtype=np.uint64)
    np_ = L.rs_emulate(_capi.dptr(x), m, iters, k, first, count, thin, pc, _capi.dptr(pr), len(pr), float(hdpi or 0.0), _capi.dptr(mean),
                       _capi.dptr(sd), _capi.dptr(quant), _capi.dptr(hd), keys.ctypes.data_as(C.POINTER(C.c_uint64)))
    out = (mean, sd, quant, hd if hdpi else None, keys)
    return out + (np_,) if passes else out


def same_outputs(a, b):
    return all((u is None and v is None) or same_bits(u, v) for u, v in zip(a[:4], b[:4])) and np.array_equal(a[4], b[4])


def _lds_bytes(code, kernel):
    """.group_segment_fixed_size of a kernel: in the metadata's alphabetical order it precedes the kernel's .name"""
    mstr = lambda v: (bytes([0xa0 | len(v)]) if len(v) < 32 else bytes([0xd9, len(v)])) + v.encode()
    at = code.find(mstr(".name") + mstr(kernel))
    k = code.rfind(mstr(".group_segment_fixed_size"), 0, at)
    assert at >= 0 and k >= 0, kernel
    p = code[k + len(mstr(".group_segment_fixed_size")):]
    return p[0] if p[0] <= 0x7f else {0xcc: p[1], 0xcd: (p[1] << 8) | p[2], 0xce: int.from_bytes(p[1:5], "big")}[p[0]]


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_summary_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.summary_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "" and r["unproven"] == 0, r   # kernel_health: metadata + isacheck's walk
    # four sort workgroups fit a CU's 160 KiB of LDS
    assert [_lds_bytes(code, k) for k in KERNELS] == [8 * (tile() + tile() // 16), 8 * (2048 + 2048 + 2048 // 8 + 2), 8 * 3 * 256]
    assert 4 * _lds_bytes(code, KERNELS[0]) <= 160 * 1024
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.summary.co")))      # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.summary_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before       # served by the kernel cache


def test_lds_banks_of_every_step_of_the_tile_sort():
    """The LDS bank rule applied to the device text's own index functions (rs_pair_lo, RS_SLOT), every wave of every step:
    ds_read_b64 is served per 32-lane half over 64 four-byte banks, ds_write_b64 per 16 lanes over 32.  Conflict-free everywhere
    but the reads of stride 256 (one bank pair twice); the network has 42 register steps and 36 pairwise ones, 4 of them stride 256."""
    L, T = emulation(), tile()

    def worst(slots, group, banks):
        w = 1
        for g in range(0, 64, group):
            cnt = {}
            for sl in set(slots[g:g + group]):
                for dw in (2 * sl % banks, (2 * sl + 1) % banks):
                    cnt[dw] = cnt.get(dw, 0) + 1
            w = max(w, max(cnt.values()))
        return w
    for j in (16, 32, 64, 128, 256, 512, 1024, 2048):
        rd = wr = 1
        seen = set()
        for w0 in range(0, T // 2, 64):
            lo = [L.rs_pair_lo_of(w0 + lane, j) for lane in range(64)]
            seen.update(lo); seen.update(e + j for e in lo)
            for part in (lo, [e + j for e in lo]):
                sl = [L.rs_slot_of(e) for e in part]
                rd, wr = max(rd, worst(sl, 32, 64)), max(wr, worst(sl, 16, 32))
        assert seen == set(range(T)), j                                  # every element is in exactly one pair
        assert (rd, wr) == ((2, 1) if j == 256 else (1, 1)), (j, rd, wr)
    for i in range(16):                                                  # the register phase: thread t at slot 17 t + i
        sl = [L.rs_slot_of(16 * t + i) for t in range(64)]
        assert sl == [17 * t + i for t in range(64)] and worst(sl, 32, 64) == 1 and worst(sl, 16, 32) == 1
    stages = [k.bit_length() - 1 for k in (2 ** e for e in range(1, T.bit_length()))]
    assert sum(min(n, 4) for n in stages) == 42 and sum(max(n - 4, 0) for n in stages) == 36 and sum(1 for n in stages if n >= 9) == 4


def test_the_model_sources_do_not_carry_the_summary_kernels():
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_summary" not in src


# ---- 2. the device text, on the host, against numpy ----------------------------------------------------------------------------------
def test_the_reference_scan_is_the_loop_and_the_keys_are_double_compare():
    k = to_key(np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf, NANS[1], NANS[2]]))
    assert np.all(k[:-2][1:] > k[:-2][:-1]) and k[-1] == k[-2] > k[-3]
    assert same_bits(from_key(k[:8]), [-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf])
    x = fixture(1, 300, 7, 3)
    s = from_key(np.sort(to_key(pooled(x)), axis=1))
    for p in range(7):
        for prob in (0.5, 0.89, 0.999, 1.0):
            assert same_bits(hdpi_of_sorted(s[p], prob), hdpi_loop(s[p], prob)), (p, prob)


NCASES = 11            # len(n_cases())


@pytest.mark.parametrize("case", range(NCASES))
@pytest.mark.parametrize("thin", [1, 3])
def test_host_emulation_matches_numpy(case, thin):
    chains, kept = n_cases()[case]
    first, count, iters = window(kept, thin)
    T = tile()
    n = chains * kept
    jobs = [(1, off) for off in range(NKINDS)] + [(5, 0), (5, 5), (65, 0)]
    for nvars, off in jobs:
        x = fixture(chains, iters, nvars, 100 * case + 10 * nvars + off + thin, off)
        got = emulate(x, first, count, thin, passes=True)
        assert got[5] == (0 if n <= T else math.ceil(math.log2(math.ceil(n / T)))), (n, got[5])
        ref = Reference(x, first, count, thin)
        assert np.array_equal(got[4], ref.keys), (case, thin, nvars, off, "sorted keys")
        check_against_reference(got, ref, (case, thin, nvars, off))
        if nvars == 65 and case in (4, 7, 9, 10):
            # the chunking of the parameters is not part of the result: three chunks of 22, 22 and 21; chunks of one
            for pc in (22, 1):
                assert same_outputs(emulate(x, first, count, thin, pc=pc), got), (case, thin, pc)
    # a window is its rows: the same bits as a (thinned) copy summarised on its own
    own = emulate(np.ascontiguousarray(x[:, first:first + count:thin, :]))
    assert same_outputs(own, got)


def test_probability_edges():
    T = tile()
    # N = 1: every index is 0
    x = fixture(1, 1, NKINDS, 9)
    for hd in (0.89, 1.0, 1e-300):
        got = emulate(x, probs=(0.0, 1.0, 0.055), hdpi=hd)
        check_against_reference(got, Reference(x, probs=(0.0, 1.0, 0.055), hdpi=hd), ("N=1", hd))
        assert same_bits(got[2], np.repeat(x[0, 0, :, None], 3, axis=1)) and same_bits(got[3][:6], np.repeat(x[0, 0, :6, None], 2, axis=1))
        assert np.all(np.isnan(got[3][6]))
    # q = 0 and q = 1 are the extremes; sixteen probabilities; hdpi_prob = 1 is (min, max)
    probs16 = tuple(np.linspace(0.0, 1.0, 16))
    for chains, iters in ((3, 21), (1, T + 1)):
        x = fixture(chains, iters, NKINDS, 17)
        got = emulate(x, probs=probs16, hdpi=1.0)
        ref = Reference(x, probs=probs16, hdpi=1.0)
        check_against_reference(got, ref, ("sixteen", chains, iters))
        s = from_key(ref.keys)
        assert same_bits(got[2][:, 0], s[:, 0]) and same_bits(got[2][:, 15], s[:, -1])
        assert same_bits(got[3][:6], np.stack([s[:6, 0], s[:6, -1]], axis=1))
        assert emulate(x, hdpi=None)[3] is None
    # ceil(prob * N) == N only through rounding.  No decimal prob whose exact product is N - 1 gets there (the product's error is
    # below half an ulp of N - 1), so the case is the double next above (N - 1) / N: the product exceeds N - 1 by one ulp and ceil
    # makes it N, where prob = (N - 1) / N itself scans one candidate pair
    n = 64
    prob = float(np.nextafter((n - 1) / n, 1.0))
    assert prob * n > n - 1 and math.ceil(prob * n) == n and math.ceil((n - 1) / n * n) == n - 1
    x = fixture(1, n, NKINDS, 23)
    got = emulate(x, hdpi=prob)
    ref = Reference(x, hdpi=prob)
    check_against_reference(got, ref, ("rounded up to N", n))
    s = from_key(ref.keys)
    assert same_bits(got[3][:6], np.stack([s[:6, 0], s[:6, -1]], axis=1))
    check_against_reference(emulate(x, hdpi=(n - 1) / n), Reference(x, hdpi=(n - 1) / n), ("N - 1", n))
    # the reference's own rounding artefact: 0.55 * 100 is 55.00000000000001 in double, so idx is 56, not 55
    assert math.ceil(0.55 * 100) == 56
    x = fixture(1, 100, NKINDS, 29)
    got = emulate(x, hdpi=0.55)
    check_against_reference(got, Reference(x, hdpi=0.55), "0.55 * 100")
    s = from_key(got[4])
    assert got[3][1][1] - got[3][1][0] == s[1][56] - s[1][0]          # the ramp: a pair 56 apart


def test_constant_and_tied_columns_take_the_first_minimum():
    T = tile()
    x = fixture(3, (T + 3) // 3 + 1, 5, 31)
    got = emulate(x)
    n = x.shape[0] * x.shape[1]
    s = from_key(got[4])
    idx = math.ceil(HDPI * n)
    assert same_bits(got[3][3], [-7.125, -7.125]) and got[1][3] == 0.0 and got[0][3] == -7.125     # the constant column
    assert same_bits(got[3][1], [s[1][0], s[1][idx]])                                              # a ramp: every width equal, i = 0
    w = s[4][idx:] - s[4][:n - idx]
    assert np.sum(w == w.min()) > 1 and same_bits(got[3][4], [s[4][np.argmin(w)], s[4][np.argmin(w) + idx]])   # ties among widths


# ---- 3. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    out = [np.zeros(8) for _ in range(4)]
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, thin=1, probs=(0.055, 0.945), nprobs=None, hdpi=0.89):
        pr = np.array(probs, dtype=np.float64) if probs is not None else None
        return L.rh_summary_device(ptr, 0, chains, iters, nvars, first, count, thin, _capi.dptr(pr) if pr is not None else None,
                                   len(pr) if nprobs is None else nprobs, hdpi, *[_capi.dptr(o) for o in out])
    err = lambda: L.rh_last_error(None).decode()
    assert call(ptr=None) == _capi.RH_E_INVALID and call(probs=None, nprobs=2) == _capi.RH_E_INVALID
    for first, count, thin in ((0, 0, 1), (0, 11, 1), (5, 6, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):
        assert call(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
        assert "window" in err()
    assert call(nvars=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    assert call(nprobs=0) == _capi.RH_E_INVALID and "nprobs" in err()
    assert call(probs=tuple([0.5] * 17)) == _capi.RH_E_INVALID and "nprobs" in err()
    for bad in (-0.001, 1.0000001, float("nan")):
        assert call(probs=(0.5, bad)) == _capi.RH_E_INVALID and "probability" in err()
    for bad in (1.0000001, float("nan"), float("inf")):
        assert call(hdpi=bad) == _capi.RH_E_INVALID and "hdpi_prob" in err()
    pr = np.array(PROBS)
    assert L.rh_sampler_summary(None, 0, 10, 1, _capi.dptr(pr), 2, 0.89, None, None, None, None) == _capi.RH_E_INVALID
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(chains=1, count=1, hdpi=0.0, probs=(0.0,)) == _capi.RH_E_DEVICE        # one chain, one draw, no hdpi: a valid request
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.summary_device(4096, 4, 10, 4)


def test_python_surface_and_format_precis():
    import inspect
    import rainier_amd as R
    from rainier_amd import distributed
    assert list(inspect.signature(R.Sampler.summary).parameters) == ["self", "first", "count", "thin", "probs", "hdpi"]
    assert list(inspect.signature(R.summary_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "thin",
                                                                    "probs", "hdpi"]
    sig = inspect.signature(R.Sampler.summary).parameters
    assert sig["probs"].default == (0.055, 0.945) and sig["hdpi"].default == 0.89 and sig["thin"].default == 1
    assert callable(distributed.Comm.summary) and R.Summary._fields[:4] == ("mean", "sd", "quantiles", "hdpi")
    s = R.Summary(np.array([1.234, -10.0, 100.5]), np.array([0.5, 2.0, 3.333]), np.array([[0.1, 2.0], [-12.0, -8.0], [95.0, 106.049]]),
                  np.zeros((3, 2)))
    assert R.format_precis(["a", "beta[1]", "c"], s) == (
        "             Mean    StdDev      5.5%     94.5%\n"
        "a            1.23      0.50      0.10      2.00\n"
        "beta[1]    -10.00      2.00    -12.00     -8.00\n"
        "c          100.50      3.33     95.00    106.05")
    with pytest.raises(ValueError):
        R.format_precis(["a"], s)
