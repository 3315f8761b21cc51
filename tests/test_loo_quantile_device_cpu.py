"""Leave-one-out predictive quantiles, CRPS and spread on the device (csrc/device/rh_loo_quantile.hip.h), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck) and its kernels
    use no scratch and spill nothing;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) -- the emulation -- and
    compared with an independent numpy / longdouble restatement of the contract in include/rainier_hip.h: lexsort on (value, weight),
    cumsum, the contract's formulas;
  * identities that need no tolerance of their own, the brute-force double sum, NaN and infinity, the plan's arithmetic, chunking and
    pair order, the C ABI's refusals; a stand-alone sanitizer build of the driver;
  * what the figures mean: the conjugate normal model, whose leave-one-out predictive distribution is known.

How a quantile is compared.  The interpolation divides by one weight, so a difference relative to the value says nothing where the
distribution function is flat; the comparison goes through the quantile function: got must lie in [q_ref(p - delta), q_ref(p + delta)],
q_ref the longdouble restatement's, widened by 4 ulp of the largest knot between the two ends.  delta is derived, not measured from
the code under test.  Under the scan of rh_loo_quantile.hip.h C_j = off [t] + r_j: r_j is a running sum of at most L = ceil(S / 256)
weights (L - 1 additions), off [t] a running sum of at most 255 segment sums of L - 1 additions each (255 more), and one addition
joins them: no C_j is behind a chain longer than L + 255 additions of non-negative terms, so C_j (1 - e) <= computed C_j <= C_j (1 + e)
with e = (L + 255) 2^-53 over the weights as computed.  A weight as computed is within LOOX_MEASURED, relatively, of the restatement's
(tests/test_loo_expect_device_cpu.py measures exactly that, on these log-likelihood fixtures), and a relative error of every term is
one of every partial sum.  The computed j and fraction solve computed C = p computed C_S exactly up to the rounding of one product,
one quotient and two differences (4 * 2^-53 of p), and computed C / computed C_S is within 2 (e + LOOX_MEASURED) of C / C_S:
    delta = 2 ((L + 255 + 4) 2^-53 + LOOX_MEASURED).
In plain mode the weights are exact (LOOX_MEASURED drops out) and so is every C_j (integers below 2^53): delta = 8 * 2^-53.

Scores: the largest relative difference of crps and spread from the restatement over SHAPES is LOOQ_MEASURED (measured on the host
against the restatement, never against the device); they are tested at four times it, and where the restatement gives exactly 0 so
must the emulation.

tests/test_gpu_loo_quantile_device.py runs the same shapes through the kernels.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_capi_cpu import _kernel_meta
from tests.test_loo_device_cpu import NKINDS, SHAPES, conjugate, fixture, pooled, same_bits, tail_len, to_keys
from tests import test_loo_device_cpu as LOO
from tests import test_loo_expect_device_cpu as LOOX
from tests.test_loo_expect_device_cpu import CONST, LOOX_MEASURED, VKINDS, case_x, restate_weights, shuffled_with_duplicate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_loo_quantile_sort_kernel", "rh_loo_quantile_merge_kernel", "rh_loo_quantile_fit_kernel", "rh_loo_quantile_weight_kernel",
           "rh_loo_quantile_kvsort_kernel", "rh_loo_quantile_kvmerge_kernel", "rh_loo_quantile_scan_kernel")
CAP, TILE, MERGE_TILE, TAIL_MAX, BLOCK = 128 << 20, 4096, 2048, 8064, 256
LD = np.longdouble
U = 2.0 ** -53
PROBS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
SCORES = ("crps", "spread")
FIELDS = ("quantiles", "crps", "spread", "pareto_k", "tail_n")
# the largest relative difference of crps and spread from the longdouble restatement, measured over SHAPES in both modes
# (profiles/loo_quantile_device: on the host, never against the device).  As LOOX_MEASURED, all of it is the kind 1 columns', whose k
# is about 10: their few heavy tail weights carry the fit's difference (5.54e-12 in spread).  Every other column, and all of plain mode,
# stays below LOOQ_REGULAR_MEASURED (1.83e-14 in crps), and they are held to four times that.
LOOQ_MEASURED = 5.6e-12
LOOQ_REGULAR_MEASURED = 1.9e-14
# the conjugate fixture (seed 2017, S = 20000, y_rep from default_rng(7)): max |q - exact| over (0.05, 0.25, 0.5, 0.75, 0.95), max
# |crps - exact|, max relative spread error, max k (profiles/loo_quantile_device)
CONJ_Q_MEASURED, CONJ_CRPS_MEASURED, CONJ_SPREAD_MEASURED, CONJ_K_MEASURED = 0.044, 0.0052, 0.011, 0.22


def delta_for(S, plain):
    return 8 * U if plain else 2.0 * ((-(-S // BLOCK) + 255 + 4) * U + LOOX_MEASURED)


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
class Ecdf:
    """the contract's (b) - (e) on one pair in longdouble: v [S] in draw order, W [S] longdouble weights"""

    def __init__(self, v, W):
        v = np.asarray(v, dtype=np.float64)
        order = np.lexsort((np.asarray(W), to_keys(v)))          # the value's key first, then the weight
        self.x = v[order]
        self.w = np.asarray(W, dtype=LD)[order]
        self.C = np.cumsum(self.w)
        self.total = self.C[-1]

    def knot(self, p):
        """(j, t): the smallest 0-based j with C_j >= t = p C_S"""
        t = LD(min(max(p, 0.0), 1.0)) * self.total
        return int(np.searchsorted(self.C, t, "left")), t

    def quantile(self, p):
        j, t = self.knot(p)
        j = min(j, len(self.x) - 1)
        if j == 0:
            return LD(self.x[0])
        x0, x1 = LD(self.x[j - 1]), LD(self.x[j])
        return x0 + (x1 - x0) * (t - self.C[j - 1]) / (self.C[j] - self.C[j - 1])

    def scores(self, y=None):
        x = self.x.astype(LD)
        a, b, F = x[:-1], x[1:], (self.C / self.total)[:-1]
        G = (np.cumsum(self.w[::-1])[::-1] / self.total)[1:]    # 1 - F_j as the weight above x_(j): the subtraction cancels in longdouble too
        spread = 2 * ((b - a) * F * G).sum()
        if y is None or math.isnan(y):
            return math.nan, float(spread)
        m = np.minimum(np.maximum(LD(y), a), b)
        with np.errstate(invalid="ignore"):
            crps = ((m - a) * F * F + (b - m) * G * G).sum() + max(x[0] - LD(y), LD(0)) + max(LD(y) - x[-1], LD(0))
        return float(crps), float(spread)


def restate(l, v, plain):
    """-> Ecdf of one pair, or None where either window is not finite"""
    if not np.all(np.isfinite(v)):
        return None
    if plain:
        return Ecdf(v, np.ones(len(v), dtype=LD))
    got = restate_weights(l)
    return None if got is None else Ecdf(v, got[0])


def check_quantiles(got, ref, probs, delta, what):
    for g, p in zip(got, probs):
        jl, jh = min(ref.knot(p - delta)[0], len(ref.x) - 1), min(ref.knot(p + delta)[0], len(ref.x) - 1)
        lo, hi = float(ref.quantile(p - delta)), float(ref.quantile(p + delta))
        knots = ref.x[max(jl - 1, 0):jh + 1]
        slack = 4 * float(np.max(np.spacing(np.abs(knots))))
        assert lo - slack <= g <= hi + slack, (what, p, g, lo, hi, slack)


def rel_scores(got, want, what):
    """the relative differences of crps and spread (sums of non-negative terms); where the restatement is exactly 0, or not finite, the
    emulation says the same"""
    out = []
    for f in SCORES:
        g, w = float(got[f]), float(want[f])
        assert math.isnan(g) == math.isnan(w) and math.isinf(g) == math.isinf(w), (what, f, g, w)
        if math.isnan(w) or math.isinf(w):
            continue
        if w == 0.0:
            assert g == 0.0, (what, f, g)
            continue
        assert g >= 0.0
        out.append(abs(g - w) / w)
    return out


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
#include <cstring>
// a workgroup's LDS as the launch sizes it, with guard words behind it
template <class T> struct Lds {
  std::vector<T> v;
  size_t n;
  explicit Lds(size_t n_) : v(n_ + 8), n(n_) { std::memset(v.data() + n, 0x5a, 8 * sizeof(T)); }
  T *p() { return v.data(); }
  bool intact() const { const unsigned char *g = (const unsigned char *)(v.data() + n); for (size_t i = 0; i < 8 * sizeof(T); i++) if (g[i] != 0x5a) return false; return true; }
};
// loo_quantile_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter), its own use of the workspace
// and the kernels' index arithmetic, one workgroup after the other.  ll == NULL: plain mode.  x_out, w_out, cum_out [K][S] (the sorted
// values, their weights, the cumulative weights) and wd_out [K][S] (the weights in draw order) may be NULL.  Returns the number of
// chunks, -1 beyond the cap, -2 beyond the tail's LDS, -3 where a guard word behind an LDS was written.
extern "C" int lq_emulate(const double *ll, long long nll, const double *val, long long nval, int chains, long long iterations, long long first, long long count,
                          long long thin, const int *lcols, const int *vcols, int K, const double *y, const double *probs, int nprobs, long long cap, double *quant,
                          double *crps, double *spread, double *pareto_k, int *tail_n, double *x_out, double *w_out, double *cum_out, double *wd_out) {
  const rh_plan::LooQuantile P = rh_plan::loo_quantile_plan(chains, count, thin, K, cap);
  if (P.over_cap) return -1;
  if (P.over_lds) return -2;
  const long long S = P.S;
  const size_t words = (size_t)(P.pc * S);
  std::vector<rs_key> ak(words), aw(words), bk(words), bw(words);
  std::vector<double> tw((size_t)(P.pc * P.M));
  Lds<rs_key> l_sort(RS_TILE_SLOTS), l_merge(RS_MERGE_LDS), l_kvsort(LQ_SORT_LDS), l_kvmerge(LQ_MERGE_LDS);
  Lds<double> l_fit(LL_LDS_DOUBLES), l_scan(LQ_SCAN_LDS_DOUBLES);
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0;
    const double *w = nullptr;
    if (ll) {
      rs_key *src = bk.data(), *dst = bw.data();
      for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE;
        if (g0 >= S) continue;
        rs_tile_sort(ll + first * nll + lcols[k0 + pl], iterations, nll, thin, P.kept, S, g0, l_sort.p(), src + pl * S + g0, LL_BLOCK);
      }
      for (int k = 0; k < P.passes; k++) {
        for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
          const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
          if (o0 >= S) continue;
          rs_merge_tile(src + pl * S, dst + pl * S, S, P.run(k), o0, l_merge.p(), LL_BLOCK);
        }
        std::swap(src, dst);
      }
      for (size_t i = 0; i < tw.size(); i++) tw[i] = -7.0;    // a weight that was not written shows
      for (long long pl = 0; pl < p_cnt; pl++) lx_fit_block(src + pl * S, S, P.M, l_fit.p(), tw.data() + pl * P.M, pareto_k + k0 + pl, tail_n + k0 + pl, LL_BLOCK);
      double *wd = (double *)dst;
      for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE, k = k0 + pl;
        if (g0 >= S) continue;
        lq_weight_block(src + pl * S, S, tw.data() + pl * P.M, pareto_k[k], tail_n[k], ll + first * nll + lcols[k], nll, iterations, thin, P.kept, g0, wd + pl * S, LL_BLOCK);
      }
      if (wd_out) for (long long pl = 0; pl < p_cnt; pl++) for (long long s = 0; s < S; s++) wd_out[(k0 + pl) * S + s] = wd[pl * S + s];
      w = wd;
    }
    rs_key *sk = ak.data(), *sw = aw.data(), *tk = bk.data(), *tww = bw.data();
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
      const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * LQ_TILE;
      if (g0 >= S) continue;
      lq_tile_sort(val + first * nval + vcols[k0 + pl], iterations, nval, thin, P.kept, S, g0, w ? w + pl * S : nullptr, l_kvsort.p(), sk + pl * S + g0, sw + pl * S + g0, LL_BLOCK);
    }
    for (int k = 0; k < P.passes; k++) {
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
        if (o0 >= S) continue;
        lq_merge_tile(sk + pl * S, sw + pl * S, tk + pl * S, tww + pl * S, S, P.run(k), o0, l_kvmerge.p(), LL_BLOCK);
      }
      std::swap(sk, tk);
      std::swap(sw, tww);
    }
    double *cum = (double *)tk;
    for (long long pl = 0; pl < p_cnt; pl++) {
      const long long k = k0 + pl;
      const bool ll_bad = ll != nullptr && rs_to_key(pareto_k[k]) == RS_KEY_NAN;
      for (long long s = 0; s < S; s++) cum[pl * S + s] = -7.0;
      lq_scan_block(sk + pl * S, sw + pl * S, S, ll_bad, y != nullptr, y ? y[k] : 0.0, probs, nprobs, cum + pl * S, l_scan.p(), quant + k * nprobs, crps ? crps + k : nullptr,
                    spread ? spread + k : nullptr, LL_BLOCK);
      for (long long s = 0; s < S; s++) {
        if (x_out) x_out[k * S + s] = rs_from_key(sk[pl * S + s]);
        if (w_out) w_out[k * S + s] = lq_weight_of(sw[pl * S + s]);
        if (cum_out) cum_out[k * S + s] = cum[pl * S + s];
      }
    }
  }
  if (!(l_sort.intact() && l_merge.intact() && l_kvsort.intact() && l_kvmerge.intact() && l_fit.intact() && l_scan.intact())) return -3;
  return chunks;
}
// kept, S, M, per_pair, pc, over_cap, over_lds, tiles, mtiles, passes, seg
extern "C" void lq_plan(long long chains, long long count, long long thin, long long K, long long cap, long long *out) {
  const rh_plan::LooQuantile P = cap ? rh_plan::loo_quantile_plan(chains, count, thin, K, cap) : rh_plan::loo_quantile_plan(chains, count, thin, K);
  const long long v[11] = {P.kept, P.S, P.M, P.per_pair, P.pc, P.over_cap ? 1 : 0, P.over_lds ? 1 : 0, P.tiles, P.mtiles, P.passes, P.seg};
  for (int i = 0; i < 11; i++) out[i] = v[i];
}
extern "C" void lq_constants(long long *out) {
  const long long v[7] = {LL_BLOCK, LQ_TILE, LQ_SORT_LDS, LQ_MERGE_LDS, LQ_SCAN_LDS_DOUBLES, LQ_WS_CAP_BYTES, RS_MAX_PROBS};
  for (int i = 0; i < 7; i++) out[i] = v[i];
}
'''
# the sanitizer tier's program: the driver above over draws it makes itself, S = 2, 4097 and 8194 (one tile; two; three tiles and two
# merge passes), both modes, several chunks
_MAIN = r'''
#include <cstdio>
int main() {
  const int shapes[3][3] = {{1, 2, 1}, {1, 4097, 1}, {2, 8194, 2}};
  for (int i = 0; i < 3; i++) {
    const int chains = shapes[i][0], thin = shapes[i][2];
    const long long count = shapes[i][1], iters = count + 3, first = 2, nll = 3, nval = 2;
    std::vector<double> ll((size_t)(chains * iters * nll)), val((size_t)(chains * iters * nval));
    unsigned long long st = 88172645463325252ull + i;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) / 9007199254740992.0; };
    for (auto &v : ll) { const double t = 6.0 * next() - 3.0; v = -0.5 * t * t; }
    for (auto &v : val) v = (double)(long long)(40.0 * next()) / 8.0;      // ties
    const int lcols[4] = {0, 2, 1, 0}, vcols[4] = {1, 0, 1, 0};
    const double y[4] = {0.5, -1.0, 7.0, 2.25}, probs[3] = {0.0, 0.5, 1.0};
    const long long kept = (count + thin - 1) / thin, S = chains * kept;
    for (int plain = 0; plain < 2; plain++) {
      double q[12], crps[4], spread[4], pk[4];
      int tn[4];
      std::vector<double> cum((size_t)(4 * S));
      const rh_plan::LooQuantile P = rh_plan::loo_quantile_plan(chains, count, thin, 4);
      const int n = lq_emulate(plain ? nullptr : ll.data(), nll, val.data(), nval, chains, iters, first, count, thin, lcols, vcols, 4, y, probs, 3, 3 * P.per_pair, q, crps,
                               spread, pk, tn, nullptr, nullptr, cum.data(), nullptr);
      if (n != 2) { std::printf("shape %d: %d chunks\n", i, n); return 1; }
      for (int k = 0; k < 4; k++) {
        for (long long s = 1; s < S; s++) if (!(cum[k * S + s] >= cum[k * S + s - 1])) { std::printf("C not monotone\n"); return 1; }
        if (!(crps[k] >= 0.0 && spread[k] >= 0.0 && q[3 * k] <= q[3 * k + 1] && q[3 * k + 1] <= q[3 * k + 2])) { std::printf("figures\n"); return 1; }
      }
    }
  }
  std::printf("ok\n");
  return 0;
}
'''
_emu = None
HDR = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
GXX = ["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function"]


def emulation():
    """draws_plan.hpp (which brings the four headers in host mode) + the driver above as a host shared library (g++ -O2
    -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_looq_emu")
        src, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(src, "w").write('#include "%s"\n%s' % (HDR, _DRIVER))
        subprocess.check_call(GXX + ["-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int)
        L.lq_emulate.argtypes = [dp, ll, dp, ll, C.c_int, ll, ll, ll, ll, ip, ip, C.c_int, dp, dp, C.c_int, ll, dp, dp, dp, dp, ip, dp, dp, dp, dp]
        L.lq_plan.argtypes = [ll, ll, ll, ll, ll, C.POINTER(ll)]
        L.lq_plan.restype = None
        L.lq_constants.argtypes = [C.POINTER(ll)]
        _emu = L
    return _emu


PLAN_FIELDS = ("kept", "S", "M", "per_pair", "pc", "over_cap", "over_lds", "tiles", "mtiles", "passes", "seg")


def plan(chains, count, thin, k, cap=0):
    out = (C.c_longlong * 11)()
    emulation().lq_plan(chains, count, thin, k, cap, out)
    return dict(zip(PLAN_FIELDS, list(out)))


def emulate(x, v, ll_cols, val_cols, y=None, probs=PROBS, first=0, count=None, thin=1, cap=CAP, dump=False, want_crps=True, want_spread=True):
    """the host emulation over x [chains][iterations][nll] (None: plain mode) and v [chains][iterations][nval] -> dict of "quantiles"
    [K][nprobs], "crps" (None without y), "spread", "pareto_k", "tail_n" (None in plain mode), "chunks", and with dump "x", "w", "cum"
    [K][S] (sorted) and "wd" [K][S] (the weights in draw order; None in plain mode)"""
    L = emulation()
    v = np.ascontiguousarray(v, dtype=np.float64)
    m, iters, nval = v.shape
    plain = x is None
    if not plain:
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape[:2] == (m, iters)
    count = iters - first if count is None else count
    vc = np.ascontiguousarray(val_cols, dtype=np.int32)
    k = len(vc)
    lc = np.zeros(k, dtype=np.int32) if plain else np.ascontiguousarray(ll_cols, dtype=np.int32)
    assert len(lc) == k
    p = plan(m, count, thin, k, cap)
    pp = np.ascontiguousarray(probs, dtype=np.float64)
    out = dict(quantiles=np.full((k, len(pp)), -1.0), crps=np.full(k, -1.0), spread=np.full(k, -1.0), pareto_k=np.full(k, -1.0), tail_n=np.full(k, -1, dtype=np.int32))
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    dumps = {f: np.zeros((k, p["S"])) for f in ("x", "w", "cum", "wd")} if dump else {}
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dq = lambda f: _capi.dptr(dumps[f]) if dump else None
    n = L.lq_emulate(None if plain else _capi.dptr(x), 0 if plain else x.shape[2], _capi.dptr(v), nval, m, iters, first, count, thin, ip(lc), ip(vc), k,
                     _capi.dptr(yy) if yy is not None else None, _capi.dptr(pp), len(pp), cap, _capi.dptr(out["quantiles"]),
                     _capi.dptr(out["crps"]) if yy is not None and want_crps else None, _capi.dptr(out["spread"]) if want_spread else None,
                     _capi.dptr(out["pareto_k"]), ip(out["tail_n"]), dq("x"), dq("w"), dq("cum"), dq("wd"))
    assert n >= 1, "refused: %d" % n
    if yy is None or not want_crps:
        assert np.all(out["crps"] == -1.0)                    # not written
        out["crps"] = None
    if not want_spread:
        assert np.all(out["spread"] == -1.0)
        out["spread"] = None
    if plain:
        assert np.all(out["pareto_k"] == -1.0) and np.all(out["tail_n"] == -1)
        out["pareto_k"] = out["tail_n"] = None
        dumps.pop("wd", None)
    out["chunks"] = n
    out.update(dumps)
    return out


_cases = {}


def emulated_case(i, plain=False, bad=np.nan):
    """(ll, val, first, count, thin, ll_cols, val_cols, y, the emulation's result with its dumps) of shape i, computed once and shared
    (the GPU tests compare with it)"""
    key = (i, plain, "nan" if np.isnan(bad) else "inf")
    if key not in _cases:
        x, v, first, count, thin, lc, vc, y = case_x(i, bad)
        _cases[key] = (x, v, first, count, thin, lc, vc, y, emulate(None if plain else x, v, lc, vc, y, PROBS, first, count, thin, dump=True))
    return _cases[key]


def same_results(a, b, pick=None):
    """entry k of a has the bits of entry pick[k] of b (where both have the figure)"""
    ix = slice(None) if pick is None else list(pick)
    for f in FIELDS:
        if a[f] is None or b[f] is None:
            continue
        if not same_bits(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64)[ix]):
            return False
    return True


def _lds_bytes(code, kernel):
    """.group_segment_fixed_size of a kernel: the key sorts before .name, so it is the last one in front of the kernel's name"""
    mstr = lambda v: (bytes([0xa0 | len(v)]) if len(v) < 32 else bytes([0xd9, len(v)])) + v.encode()
    at = code.find(mstr(".name") + mstr(kernel))
    k = code.rfind(mstr(".group_segment_fixed_size"), 0, at)
    assert at >= 0 and k >= 0, kernel
    p = code[k + len(mstr(".group_segment_fixed_size")):]
    return p[0] if p[0] <= 0x7f else int.from_bytes(p[1:1 + {0xcc: 1, 0xcd: 2, 0xce: 4, 0xcf: 8}[p[0]]], "big")


# ---- 1. the code object and the public surface ---------------------------------------------------------------------------------------
def test_loo_quantile_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.loo_quantile_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r   # kernel_health: metadata + isacheck's walk
        print(k, "vgprs", r["vgprs"], "sgprs", r["sgprs"], "lds", _lds_bytes(code, k))
    assert _lds_bytes(code, "rh_loo_quantile_kvsort_kernel") == 8 * 2 * (TILE + TILE // 16)          # 68 KiB: two workgroups per CU
    assert _lds_bytes(code, "rh_loo_quantile_kvmerge_kernel") == 8 * (2 * (MERGE_TILE + MERGE_TILE + MERGE_TILE // 8) + 2)
    assert _lds_bytes(code, "rh_loo_quantile_scan_kernel") == 8 * (5 * BLOCK + 2) and _lds_bytes(code, "rh_loo_quantile_weight_kernel") == 0
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.loo_quantile.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.loo_quantile_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_other_code_objects_do_not_carry_the_loo_quantile_kernels():
    assert b"rh_loo_quantile_scan_kernel" in _capi.loo_quantile_lower_only("gfx950")          # the name does show where the kernels are
    for other in (_capi.loo_expect_lower_only, _capi.loo_lower_only, _capi.summary_lower_only, _capi.rank_lower_only, _capi.ppc_lower_only):
        assert b"rh_loo_quantile" not in other("gfx950")


def test_exports_and_python_surface():
    import inspect
    import rainier_amd as R
    L = _capi.lib()
    for name in ("rh_loo_quantile_device", "rh_sampler_loo_quantile", "rh_loo_quantile_lower_only"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert R.LooQuantile._fields == ("probs", "quantiles", "crps", "spread", "pareto_k", "tail_n", "ll_cols", "val_cols")
    assert list(inspect.signature(R.loo_quantile_device).parameters) == ["ll_ptr", "val_ptr", "chains", "iterations", "nll", "nval", "ll_cols", "val_cols", "probs", "y",
                                                                         "device", "first", "count", "thin"]
    sig = inspect.signature(R.Sampler.loo_quantile).parameters
    assert list(sig)[:4] == ["self", "ll_predictor", "predictor", "probs"] and list(sig)[-3:] == ["y", "generator", "seed"]
    assert sig["probs"].default == (0.05, 0.5, 0.95) and all(sig[n].default is None for n in ("y", "generator", "seed", "ll_cols", "val_cols", "count"))
    r = R.LooQuantile((0.5,), np.array([[1.0], [2.0]]), np.array([0.5, 1.0]), np.array([1.0, 4.0]), None, None, (), (0, 1))
    assert np.array_equal(r.abs_err, [1.0, 3.0]) and np.allclose(r.scrps, [-1.0, -0.75 - 0.5 * math.log(4.0)], rtol=1e-15)
    assert r._replace(crps=None).abs_err is None and r._replace(crps=None).scrps is None
    with pytest.raises(ValueError, match="pair up"):
        R.loo_quantile_device(4096, 4096, 4, 10, 2, 2, [0, 1], [0])
    with pytest.raises(ValueError, match="y has"):
        R.loo_quantile_device(4096, 4096, 4, 10, 2, 2, [0, 1], [0, 1], y=[0.5])


# ---- 2. the emulation against the longdouble restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_figures_against_the_longdouble_restatement(i, plain):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, plain)
    pl, pv = pooled(x, first, count, thin, lc), pooled(v, first, count, thin, vc)
    S = pl.shape[1]
    assert S == SHAPES[i][0] * -(-count // thin) == emu["x"].shape[1]
    delta = delta_for(S, plain)
    loo, lx = LOO.emulated_case(i)[4], LOOX.emulated_case(i)[8]
    worst = 0.0
    for k in range(len(lc)):
        got = {f: emu[f][k] for f in FIELDS if emu[f] is not None}
        if not plain:
            # the tail fit is rh_loo's and the draws' weights are rh_loo_expect's, bit for bit
            assert same_bits(got["pareto_k"], loo["pareto_k"][lc[k]]) and got["tail_n"] == loo["tail_n"][lc[k]], (SHAPES[i], k)
        if lc[k] % NKINDS == 5:                                # a NaN in the log-likelihood window -- and, the value being of the same theta or exp(l), in kind 1's
            if not plain:
                assert np.all(np.isnan(got["quantiles"])) and np.isnan(got["crps"]) and np.isnan(got["spread"]) and got["tail_n"] == 0 and np.isnan(got["pareto_k"])
                continue
        elif not plain:
            assert same_bits(emu["wd"][k], lx["w"][k]), (SHAPES[i], k)
        ref = restate(pl[k], pv[k], plain)
        if ref is None:
            assert np.all(np.isnan(got["quantiles"])) and np.isnan(got["crps"]) and np.isnan(got["spread"]), (SHAPES[i], k)
            continue
        # the sorted sequence is the multiset's: the keys ascending, the weights ascending inside a key
        assert np.array_equal(to_keys(emu["x"][k]), to_keys(ref.x)) and np.all(np.diff(emu["cum"][k]) >= 0.0), (SHAPES[i], k)
        check_quantiles(got["quantiles"], ref, PROBS, delta, (SHAPES[i], k))
        assert np.all(np.diff(got["quantiles"]) >= 0.0)
        crps, spread = ref.scores(float(y[k]))
        d = rel_scores(got, dict(crps=crps, spread=spread), (SHAPES[i], k))
        assert all(e <= 4 * LOOQ_MEASURED for e in d), (SHAPES[i], k, d, got, crps, spread)
        if plain or lc[k] % NKINDS != 1:
            assert all(e <= 4 * LOOQ_REGULAR_MEASURED for e in d), (SHAPES[i], k, d, got, crps, spread)
        worst = max([worst] + d)
    print("largest relative difference of crps / spread from the restatement: %.3g" % worst)
    assert worst <= LOOQ_MEASURED


# ---- 3. identities that need no tolerance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_identities(i, plain):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, plain)
    k = len(lc)
    xx = None if plain else x
    hi = emulate(xx, v, lc, vc, np.full(k, np.inf), PROBS, first, count, thin)
    lo = emulate(xx, v, lc, vc, np.full(k, -np.inf), PROBS, first, count, thin)
    none = emulate(xx, v, lc, vc, None, PROBS, first, count, thin)
    only_q = emulate(xx, v, lc, vc, y, PROBS, first, count, thin, want_crps=False, want_spread=False)
    assert none["crps"] is None and same_results(none, emu) and only_q["spread"] is None and same_results(only_q, emu)
    for j in range(k):
        if np.isnan(emu["spread"][j]):
            assert np.isnan(hi["crps"][j]) and np.isnan(lo["crps"][j])
            continue
        xs, ws, cum = emu["x"][j], emu["w"][j], emu["cum"][j]
        # probs 0 and 1: x_(1) and the largest value of positive weight, with their own bits -- the largest whose weight still moves C:
        # behind a draw that carries nearly all the weight (kind 1, k about 10) an addition absorbs the others'
        last = int(np.max(np.flatnonzero(ws > 0.0)))
        assert same_bits(emu["quantiles"][j][0], xs[0]) and same_bits(emu["quantiles"][j][-1], xs[np.searchsorted(cum, cum[-1], "left")]), (SHAPES[i], j)
        if np.all(np.diff(cum)[ws[1:] > 0.0] > 0.0):
            assert same_bits(emu["quantiles"][j][-1], xs[last])
        else:
            assert not plain and lc[j] % NKINDS == 1
        # C is non-decreasing as computed and ends in the total; the y = +-inf edge terms
        assert np.all(np.diff(cum) >= 0.0) and cum[0] == ws[0] and hi["crps"][j] == math.inf and lo["crps"][j] == math.inf
        assert same_bits(hi["spread"][j], emu["spread"][j]) and same_bits(hi["quantiles"][j], emu["quantiles"][j])
        if vc[j] % VKINDS == 2:                                # the constant: every quantile is the value, spread 0, crps |c - y|
            assert np.all(emu["quantiles"][j] == CONST) and emu["spread"][j] == 0.0 and emu["crps"][j] == abs(CONST - y[j])
        if plain:
            assert np.array_equal(ws, np.ones_like(ws)) and np.array_equal(cum, np.arange(1, len(ws) + 1))
        elif lc[j] % NKINDS == 4:                              # a constant log-likelihood: every weight is 1, the plain figures
            plain_emu = emulated_case(i, True)[8]
            assert all(same_bits(emu[f][j], plain_emu[f][j]) for f in ("quantiles", "crps", "spread"))


def test_plain_mode_puts_knot_j_at_j_over_s():
    rng = np.random.default_rng(31)
    for chains, iters in ((4, 16), (2, 4096)):               # S a power of two: j / S and (j / S) S are exact
        S = chains * iters
        v = rng.permutation(S).astype(np.float64).reshape(chains, iters, 1) * 0.37 - 11.0
        probs = [j / S for j in (1, 2, 3, S // 2, S - 1, S)] + [1.5 / S, (S - 0.25) / S]
        emu = emulate(None, v, [0], [0], None, probs)
        xs = np.sort(v.reshape(-1))
        want = [xs[j - 1] for j in (1, 2, 3, S // 2, S - 1, S)]
        assert same_bits(emu["quantiles"][0][:6], want)
        assert emu["quantiles"][0][6] == xs[0] + (xs[1] - xs[0]) * 0.5 and emu["quantiles"][0][7] == xs[S - 2] + (xs[S - 1] - xs[S - 2]) * 0.75


def test_signed_zeros_and_a_constant_column():
    v = np.zeros((2, 6, 2))
    v[:, ::2, 0] = -0.0
    v[:, :, 1] = -2.5
    x = fixture(2, 6, 2, 3)
    for xx in (None, x):
        emu = emulate(xx, v, [0, 0], [0, 1], [0.25, 1.0], dump=True)
        assert np.array_equal(np.signbit(emu["x"][0]), [True] * 6 + [False] * 6)       # -0.0 before +0.0
        assert np.all(emu["quantiles"][0] == 0.0) and emu["spread"][0] == 0.0 and emu["crps"][0] == 0.25
        assert np.all(emu["quantiles"][1] == -2.5) and emu["spread"][1] == 0.0 and emu["crps"][1] == 3.5
        assert not np.signbit(emu["spread"][0]) and np.signbit(emu["quantiles"][0][0])   # x_(1) is -0.0 itself


@pytest.mark.parametrize("i", (2, 5, 7, 8))
def test_shuffled_draws_give_the_same_bits_and_duplicated_draws_the_same_figures(i):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i)
    chains = x.shape[0]
    cut = lambda a: np.ascontiguousarray(a[:, first:first + count:thin, :])
    cx, cv = cut(x), cut(v)
    kept = cx.shape[1]
    flat = lambda a: a.reshape(chains * kept, -1)
    perm = np.random.default_rng(50 + i).permutation(chains * kept)
    sx, sv = flat(cx)[perm].reshape(cx.shape), flat(cv)[perm].reshape(cv.shape)
    # the lexicographic order makes the sorted pairs a function of the multiset: no figure depends on the draws' order
    assert same_results(emulate(sx, sv, lc, vc, y), emu) and same_results(emulate(None, sv, lc, vc, y), emulated_case(i, True)[8]), SHAPES[i]
    # every draw twice (plain mode: the fit of a longer column is another fit): the same distribution function, so the same scores.  The
    # quantile's interpolation is not a functional of the distribution function alone: between the original's knots j - 1 and j the
    # doubled column interpolates over the first half of the step and is flat over the second.  In plain mode every C is an exact
    # integer and the divisor is 1, so that piecewise rule, written out in double, is asked for bit by bit
    dv = np.repeat(cv, 2, axis=1)
    plain2, plain1 = emulate(None, dv, lc, vc, y), emulated_case(i, True)[8]
    pv = pooled(v, first, count, thin, vc)
    delta = delta_for(2 * chains * kept, True)
    for k in range(len(lc)):
        if np.isnan(plain1["spread"][k]):
            continue
        ref = restate(None, pv[k], True)
        for q, p in zip(plain2["quantiles"][k], PROBS):
            jl, jh = min(ref.knot(p - delta)[0], len(ref.x) - 1), min(ref.knot(p + delta)[0], len(ref.x) - 1)
            assert ref.x[max(jl - 1, 0)] <= q <= ref.x[jh], (SHAPES[i], k, p)
            t2 = np.float64(p) * np.float64(2 * len(ref.x))       # the doubled column's target; its knot j2 (1-based) holds x_(ceil(j2 / 2))
            j2 = max(int(math.ceil(t2)), 1)
            want = ref.x[(j2 + 1) // 2 - 1]
            if j2 > 1 and t2 != j2:
                below = ref.x[j2 // 2 - 1]                        # knot j2 - 1: the same value (flat) where j2 is even
                want = below + (want - below) * ((t2 - np.float64(j2 - 1)) / np.float64(1.0))
            assert same_bits(q, want), (SHAPES[i], k, p, q, want)
        for f in SCORES:
            assert abs(plain2[f][k] - plain1[f][k]) <= 4 * LOOQ_MEASURED * plain1[f][k], (SHAPES[i], k, f)


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_properties_of_the_contract(i, plain):
    x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, plain)
    chains, k = SHAPES[i][0], len(lc)
    xx = None if plain else x
    # a second call gives the same bits
    assert same_results(emulate(xx, v, lc, vc, y, PROBS, first, count, thin), emu), SHAPES[i]
    # a window (first > 0) gives the bits of its copy (thinned on the host)
    assert first > 0
    cut = lambda a: np.ascontiguousarray(a[:, first:first + count:thin, :])
    assert same_results(emulate(None if plain else cut(x), cut(v), lc, vc, y), emu), SHAPES[i]
    # a shuffled pair list with a duplicate gives the bits of the full call's entries
    pick = shuffled_with_duplicate(k, i)
    assert same_results(emulate(xx, v, [lc[j] for j in pick], [vc[j] for j in pick], y[pick], PROBS, first, count, thin), emu, pick), SHAPES[i]
    # forcing several chunks gives the same bits
    p = plan(chains, count, thin, k)
    small = emulate(xx, v, lc, vc, y, PROBS, first, count, thin, cap=3 * p["per_pair"])
    assert small["chunks"] == -(-k // 3) and emu["chunks"] == 1 and same_results(small, emu), SHAPES[i]
    # another list of probabilities: each quantile is its own
    one = emulate(xx, v, lc, vc, y, (PROBS[3],), first, count, thin)
    assert same_bits(one["quantiles"][:, 0], emu["quantiles"][:, 3]) and same_bits(one["crps"], emu["crps"])


# ---- 4. brute force ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", (0, 1, 2, 3, 4))
def test_crps_is_the_energy_form_by_brute_force(i):
    """crps = sum w |v - y| - 1/2 sum sum w w' |v - v'| over the normalised weights, the O(S^2) double sum in longdouble (S <= 1500: these
    shapes, and 1300 draws of the conjugate fixture below)"""
    for plain in (False, True):
        x, v, first, count, thin, lc, vc, y, emu = emulated_case(i, plain)
        pl, pv = pooled(x, first, count, thin, lc), pooled(v, first, count, thin, vc)
        for k in range(len(lc)):
            if np.isnan(emu["spread"][k]):
                continue
            W = np.ones(pv.shape[1], dtype=LD) if plain else restate_weights(pl[k])[0]
            energy_check(emu["crps"][k], emu["spread"][k], pv[k], W, float(y[k]), (SHAPES[i], plain, k))


def energy_check(crps, spread, v, W, y, what):
    w = W / W.sum()
    V = v.astype(LD)
    e1 = (w * np.abs(V - LD(y))).sum()
    e2 = (w[:, None] * w[None, :] * np.abs(V[:, None] - V[None, :])).sum()
    scale = float(e1 + e2)                                   # what the difference e1 - e2 / 2 is the rounding of
    assert abs(spread - float(e2)) <= 4 * LOOQ_MEASURED * scale and abs(crps - float(e1 - e2 / 2)) <= 4 * LOOQ_MEASURED * scale, (what, crps, spread, float(e1), float(e2))


def test_crps_by_brute_force_on_the_conjugate_fixture():
    ll, _ = conjugate()
    x = np.ascontiguousarray(ll[:2, :650, :3])
    rng = np.random.default_rng(2017)
    yobs = rng.standard_normal(10) + 0.7
    v = np.ascontiguousarray(np.random.default_rng(7).standard_normal((2, 650, 3)) + yobs.mean())
    emu = emulate(x, v, [0, 1, 2], [0, 1, 2], yobs[:3])
    pl, pv = pooled(x), pooled(v)
    for k in range(3):
        energy_check(emu["crps"][k], emu["spread"][k], pv[k], restate_weights(pl[k])[0], float(yobs[k]), k)


# ---- 5. NaN and infinity -------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_in_either_window_and_in_y_touch_their_own_outputs_only():
    x, v, first, count, thin, lc, vc, y = case_x(5)         # 5 chains, count 819, 13 log-likelihood columns; 5 and 11 hold a NaN already
    clean = emulate(x, v, lc, vc, y, PROBS, first, count, thin)
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
    yy[4 * 10 + 3] = np.nan
    got = emulate(bx, bv, lc, vc, yy, PROBS, first, count, thin)
    pos_nan = np.array([np.nan]).view(np.uint64)[0] & np.uint64(0x7fffffffffffffff) | np.uint64(0x7ff8000000000000)
    canonical = lambda a: np.all(np.atleast_1d(np.asarray(a, dtype=np.float64)).view(np.uint64) == np.uint64(0x7ff8000000000000))
    assert pos_nan == np.uint64(0x7ff8000000000000)
    for k in range(len(lc)):
        if lc[k] in (0, 6, 9, 5, 11):
            assert all(canonical(got[f][k]) for f in ("quantiles", "crps", "spread", "pareto_k")) and got["tail_n"][k] == 0, k
        elif vc[k] in (4 * 3, 4 * 4 + 3, 4 * 7 + 2):
            assert all(canonical(got[f][k]) for f in ("quantiles", "crps", "spread")), k
            assert same_bits(got["pareto_k"][k], clean["pareto_k"][k]) and got["tail_n"][k] == clean["tail_n"][k], k
        elif k == 4 * 10 + 3:
            assert canonical(got["crps"][k]) and all(same_bits(got[f][k], clean[f][k]) for f in ("quantiles", "spread", "pareto_k", "tail_n")), k
        else:
            assert all(same_bits(got[f][k], clean[f][k]) for f in FIELDS), k
            assert np.all(np.isfinite(got["quantiles"][k])) and np.isfinite(got["crps"][k])
    # plain mode: the log-likelihoods are not read
    pgot, pclean = emulate(None, bv, lc, vc, yy, PROBS, first, count, thin), emulate(None, v, lc, vc, y, PROBS, first, count, thin)
    for k in range(len(lc)):
        if vc[k] in (4 * 3, 4 * 4 + 3, 4 * 7 + 2) or vc[k] % VKINDS == 1 and lc[k] in (5, 11):
            assert all(canonical(pgot[f][k]) for f in ("quantiles", "crps", "spread")), k
        elif k == 4 * 10 + 3:
            assert canonical(pgot["crps"][k]) and same_bits(pgot["quantiles"][k], pclean["quantiles"][k]) and same_bits(pgot["spread"][k], pclean["spread"][k])
        else:
            assert all(same_bits(pgot[f][k], pclean[f][k]) for f in ("quantiles", "crps", "spread")), k
    # thinning steps over a bad value
    x2, v2, first, count, thin, lc, vc, y = case_x(8)
    assert thin == 2
    x2[0, first + 1, 0] = np.nan
    v2[1, first + 3, 1] = -np.inf
    assert same_results(emulate(x2, v2, lc, vc, y, PROBS, first, count, thin), emulated_case(8)[8])


# ---- 6. the plan and the C ABI without a device --------------------------------------------------------------------------------------
def test_the_plan_is_arithmetic_over_the_headers_constants():
    consts = (C.c_longlong * 7)()
    emulation().lq_constants(consts)
    assert list(consts) == [BLOCK, TILE, 2 * (TILE + TILE // 16), 2 * (MERGE_TILE + MERGE_TILE + MERGE_TILE // 8) + 2, 5 * BLOCK + 2, CAP, 16]
    for chains, count, thin, k in ((1, 2, 1, 1), (4, 5, 1, 6), (2, 8194, 2, 6), (16, 1250, 1, 13), (1024, 200, 1, 434), (64, 2000, 1, 70), (3, 100, 7, 5)):
        kept = -(-count // thin)
        S = chains * kept
        M = tail_len(S)
        tiles, passes = -(-S // TILE), 0
        while TILE << passes < S:
            passes += 1
        per = 32 * S + 8 * M
        want = dict(kept=kept, S=S, M=M, per_pair=per, pc=max(1, min(CAP // per, k)), over_cap=0, over_lds=0, tiles=tiles, mtiles=-(-S // MERGE_TILE), passes=passes,
                    seg=-(-S // BLOCK))
        assert plan(chains, count, thin, k) == want, (chains, count, thin, k)
        q = LOOX.plan(chains, count, thin, k)
        assert all(want[f] == q[f] for f in ("kept", "S", "M", "tiles", "mtiles", "passes"))      # the sort plan is the summary's, the tail rh_loo's
    assert plan(1024, 200, 1, 434)["pc"] == 20
    # refused from the shape alone: M beyond the tail's LDS, one pair beyond the cap
    assert plan(1, 4190000, 1, 1)["over_cap"] == 0 and plan(1, 1 << 22, 1, 1)["over_cap"] == 1 and plan(1, 1 << 22, 1, 1)["pc"] == 1
    assert plan(1, 7225345, 1, 1)["over_lds"] == 1 and plan(1, 7225344, 1, 1)["over_lds"] == 0
    x = fixture(2, 40, 3, 1)
    sel = (C.c_int * 3)(0, 1, 2)
    pr = (C.c_double * 1)(0.5)
    assert emulation().lq_emulate(_capi.dptr(x), 3, _capi.dptr(x), 3, 2, 40, 0, 40, 1, sel, sel, 3, None, pr, 1, plan(2, 40, 1, 3)["per_pair"] - 1, *[None] * 9) == -1


def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    q, crps, spread, pk = np.zeros(64), np.zeros(8), np.zeros(8), np.zeros(8)
    tn = np.zeros(8, dtype=np.int32)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ll=fake, val=fake, chains=4, iters=10, nll=2, nval=3, first=0, count=10, thin=1, lc=(0, 1), vc=(2, 0), ncols=None, y=None, probs=(0.05, 0.5), nprobs=None,
             null=(), no_lc=False, no_vc=False, no_probs=False):
        a, b = np.array(lc, dtype=np.int32), np.array(vc, dtype=np.int32)
        yy = None if y is None else np.array(y, dtype=np.float64)
        pp = np.array(probs, dtype=np.float64)
        o = [_capi.dptr(q), _capi.dptr(crps) if yy is not None else None, _capi.dptr(spread), _capi.dptr(pk), tn.ctypes.data_as(ip)]
        for i in null:
            o[i] = None
        return L.rh_loo_quantile_device(ll, nll, val, nval, 0, chains, iters, first, count, thin, None if no_lc else a.ctypes.data_as(ip),
                                        None if no_vc else b.ctypes.data_as(ip), len(b) if ncols is None else ncols, _capi.dptr(yy) if yy is not None else None,
                                        None if no_probs else _capi.dptr(pp), len(pp) if nprobs is None else nprobs, *o)
    err = lambda: L.rh_last_error(None).decode()
    assert call(val=None) == _capi.RH_E_INVALID and "NULL" in err()
    assert call(no_lc=True) == _capi.RH_E_INVALID and "NULL" in err() and call(no_vc=True) == _capi.RH_E_INVALID and call(no_probs=True) == _capi.RH_E_INVALID
    for null in (0, 3, 4):
        assert call(null=[null]) == _capi.RH_E_INVALID and "NULL" in err()
    o = [_capi.dptr(q), _capi.dptr(crps), _capi.dptr(spread), _capi.dptr(pk), tn.ctypes.data_as(ip)]
    sel = np.zeros(2, dtype=np.int32)
    pp = np.array([0.5])
    # crps needs y
    assert L.rh_loo_quantile_device(fake, 2, fake, 3, 0, 4, 10, 0, 10, 1, sel.ctypes.data_as(ip), sel.ctypes.data_as(ip), 2, None, _capi.dptr(pp), 1, *o) == _capi.RH_E_INVALID
    for first, count, thin in ((0, 0, 1), (0, 11, 1), (7, 4, 1), (-1, 5, 1), (10, 1, 1), (0, 10, 0), (0, 10, -2)):
        assert call(first=first, count=count, thin=thin) == _capi.RH_E_INVALID, (first, count, thin)
        assert "window" in err()
    assert call(nll=0) == _capi.RH_E_INVALID and call(nval=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    assert call(chains=1, count=1) == _capi.RH_E_INVALID and "at least 2" in err()
    assert call(chains=1, count=10, thin=10) == _capi.RH_E_INVALID and "at least 2" in err()
    for lc, vc in (((2, 0), (0, 0)), ((-1, 0), (0, 0)), ((0, 1), (3, 0)), ((0, 1), (0, -1))):
        assert call(lc=lc, vc=vc) == _capi.RH_E_INVALID and "outside" in err(), (lc, vc)
    assert call(ncols=0) == _capi.RH_E_INVALID and "ncols" in err() and call(ncols=-3) == _capi.RH_E_INVALID
    for probs in ((-0.1,), (1.0000001,), (0.5, np.nan), (np.inf,)):
        assert call(probs=probs) == _capi.RH_E_INVALID and "[0, 1]" in err(), probs
    assert call(nprobs=0) == _capi.RH_E_INVALID and "nprobs" in err() and call(probs=[0.5] * 17) == _capi.RH_E_INVALID and "nprobs" in err()
    assert L.rh_sampler_loo_quantile(None, None, None, None, 0, 0, 10, 1, sel.ctypes.data_as(ip), sel.ctypes.data_as(ip), 2, None, _capi.dptr(pp), 1, *o) == _capi.RH_E_INVALID
    # one pair beyond the workspace cap, and one whose tail is beyond the LDS: refused from the shape, whatever the machine
    assert call(chains=2049, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    # (a tail beyond the LDS needs S above 7.2 million, which 32 S bytes of workspace refuse first: the plan reports it, the ABI cannot reach it)
    assert call(ll=None, no_lc=True, null=[3, 4], chains=2049, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED     # plain mode is planned the same way
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(y=[0.5, np.nan]) == _capi.RH_E_DEVICE and call(null=[2]) == _capi.RH_E_DEVICE and call(probs=[0.0, 1.0] * 8) == _capi.RH_E_DEVICE
        assert call(ll=None, no_lc=True, null=[3, 4]) == _capi.RH_E_DEVICE                                             # plain mode: no lists, no tail outputs
        assert call(lc=(1, 1, 0), vc=(0, 0, 2)) == _capi.RH_E_DEVICE and call(chains=1, count=2) == _capi.RH_E_DEVICE and call(thin=3) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.loo_quantile_device(4096, 4096, 4, 10, 4, 4, [0], [1])
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.loo_quantile_device(None, 4096, 4, 10, 0, 4, None, [1, 2], y=[0.0, 1.0])


# ---- 7. what the figures mean --------------------------------------------------------------------------------------------------------
def test_conjugate_normal_model_against_the_analytic_leave_one_out_predictive_distribution():
    from statistics import NormalDist
    n = 10
    ll, _ = conjugate()
    rng = np.random.default_rng(2017)                          # conjugate()'s own draws
    yobs = rng.standard_normal(n) + 0.7
    theta = yobs.mean() + rng.standard_normal((16, 1250)) / math.sqrt(n)
    yrep = np.ascontiguousarray((theta + np.random.default_rng(7).standard_normal((16, 1250)))[:, :, None])
    probs = (0.05, 0.25, 0.5, 0.75, 0.95)
    emu = emulate(ll, yrep, list(range(n)), [0] * n, yobs, probs)
    others, sigma = (yobs.sum() - yobs) / (n - 1), math.sqrt(1.0 + 1.0 / (n - 1))
    N = NormalDist()
    q_exact = np.array([[others[i] + sigma * N.inv_cdf(p) for p in probs] for i in range(n)])
    z = (yobs - others) / sigma
    crps_exact = np.array([sigma * (zi * (2.0 * N.cdf(zi) - 1.0) + 2.0 * N.pdf(zi) - 1.0 / math.sqrt(math.pi)) for zi in z])
    d_q = float(np.max(np.abs(emu["quantiles"] - q_exact)))
    d_crps = float(np.max(np.abs(emu["crps"] - crps_exact)))
    d_spread = float(np.max(np.abs(emu["spread"] / (2.0 * sigma / math.sqrt(math.pi)) - 1.0)))
    k = float(np.max(emu["pareto_k"]))
    print("conjugate fixture: max |q - exact| %.4f, max |crps - exact| %.4f, max relative spread error %.4f, max k %.3f" % (d_q, d_crps, d_spread, k))
    assert d_q <= CONJ_Q_MEASURED and d_crps <= CONJ_CRPS_MEASURED and d_spread <= CONJ_SPREAD_MEASURED and k <= CONJ_K_MEASURED   # the README's figures are what is measured
    assert d_q <= 2 * CONJ_Q_MEASURED and d_crps <= 2 * CONJ_CRPS_MEASURED and d_spread <= 2 * CONJ_SPREAD_MEASURED and k < 0.7        # the bound: twice them
    assert np.all(emu["tail_n"] == tail_len(20000)) and np.all(emu["crps"] > 0.0)


# ---- 8. the driver under AddressSanitizer and UBSan ----------------------------------------------------------------------------------
def test_the_emulation_driver_runs_clean_under_the_sanitizers():
    """a stand-alone host program (its own main, a child process): nothing is loaded into python under a sanitizer"""
    d = tempfile.mkdtemp(prefix="rh_looq_san")
    probe, src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "san.cpp"), os.path.join(d, "san")
    open(probe, "w").write("int main() { return 0; }\n")
    # (shift-base off: fdlibm's exponent arithmetic in rh_loo.hip.h shifts a negative int left, which both compilers define)
    san = ["-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    if subprocess.run(["g++"] + san + [probe, "-o", os.path.join(d, "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    open(src, "w").write('#include "%s"\n%s\n%s' % (HDR, _DRIVER, _MAIN))
    subprocess.check_call(GXX[:1] + ["-O1"] + GXX[2:] + san + [src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
