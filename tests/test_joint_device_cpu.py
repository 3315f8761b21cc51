"""Multivariate ESS and MPSRF on the device (csrc/device/rh_joint.hip.h), the part that needs no GPU: the device text compiled with
the host g++ (RH_JOINT_HOST: every "thread" of a phase in turn, the MFMA a chain of fma over k = 0, 1, 2, 3 at the instruction's lane
maps) and driven over whole buffers as joint_run's launches walk them, with the host finish the library itself uses, against a plain
np.longdouble restatement of the contract.

Bounds, derived (u = 2^-53): a Gram entry sum_r d_ra d_rb is computed from rows and centres that are themselves rounded sums -- a
mean of t terms is off by at most (t + 2) u sum|x| / t -- so with eta_ra that bound for row r's value plus its centre's and
D = |d| + eta, the entry is off by at most sum_r (D_ra D_rb - |d_ra d_rb|) + (R + 8) u sum_r D_ra D_rb (R fused multiply-adds, the
adds of the splits, the centring's rounding in either factor, the divisor, the scale), times the entry's scale.  A dropped or doubled
row is off by about 1 / R of the sum.  mess and mpsrf: relative 1e-9 (K cond u = 65 * 1e4 * 1.1e-16 = 7e-11, one order of margin),
where cond(Sigma) and cond(W) of the reference are at most 1e4, which is asserted."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_covariance_device_cpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, LD, CAP = 2.0 ** -53, np.longdouble, 128 << 20
CASES = [(2, 4), (3, 10), (3, 33), (5, 900), (1, 64)]     # (C, count) at the default batch: b = 2, 3, 5, 30, 8
KS = [1, 5, 64, 65]
MATS = ("within", "between", "sigma", "mcse_cov")


def fixture(chains, iters, k, seed=11, stuck=0.0, nan_col=None):
    """independent AR(1) columns (coefficients 0.1 .. 0.5, unit variance) mixed by a fixed well-conditioned matrix, a per-chain offset
    of sd 0.1 (chain 0's moved by `stuck` in column 0), column k // 2 shifted by 1e6"""
    rng = np.random.default_rng(seed + 1000 * chains + iters + 7 * k)
    rho = 0.1 + 0.4 * np.arange(k) / max(k - 1, 1)
    z = rng.standard_normal((chains, iters, k))
    for t in range(1, iters):
        z[:, t] = rho * z[:, t - 1] + np.sqrt(1.0 - rho * rho) * z[:, t]
    x = z @ (np.eye(k) + 0.1 * np.random.default_rng(7).standard_normal((k, k)) / math.sqrt(k)).T + 0.1 * rng.standard_normal((chains, 1, k))
    x[0, :, 0] += stuck
    x[:, :, k // 2] += 1e6
    if nan_col is not None:
        x[chains // 2, iters // 3, nan_col] = np.nan
    return x


def reference(x, first=0, count=None, batch=0, cols=None):
    """the contract in np.longdouble -> dict of the figures, and of the matrices' and ess_bm's error bounds under "bound" """
    c, iters, nv = x.shape
    count = iters - first if count is None else count
    cols = list(range(nv)) if cols is None else list(cols)
    k, b = len(cols), batch or math.isqrt(count)
    a = count // b
    n, big = a * b, c * a * b
    u = x[:, first + count - n:first + count, :][:, :, cols].astype(LD)
    m, mu, y = u.sum(1) / n, u.sum((0, 1)) / big, u.reshape(c, a, b, k).sum(2) / b
    au = np.abs(u)
    em, emu, ey = (n + 2) * U * au.sum(1) / n, (big + 2) * U * au.sum((0, 1)) / big, (b + 2) * U * au.reshape(c, a, b, k).sum(2) / b

    def gram(d, eta):
        dd, ad = d.reshape(-1, k), np.abs(d).reshape(-1, k)
        full = ad + np.broadcast_to(eta, d.shape).reshape(-1, k)
        return dd.T @ dd, (full.T @ full - ad.T @ ad) + (len(dd) + 8) * U * (full.T @ full)
    gw, bw = gram(u - m[:, None, :], em[:, None, :])
    gs, bs = gram(y - mu, ey + emu)
    gb, bb = gram(m - mu, em + emu)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = dict(mean=mu, within=gw / (c * (n - 1)), between=gb / LD(c - 1), sigma=b * gs / (c * a - 1), batch=b, batches=a, dropped=count - n, N=big)
        lam = (gw + n * gb) / (big - 1)
        bl = (bw + n * bb) / (big - 1) + 4 * U * np.abs(lam)
        r["mcse_cov"] = r["sigma"] / big
        r["ess_bm"] = big * np.diag(lam) / np.diag(r["sigma"])
        bsig = b * bs / (c * a - 1)
        r["bound"] = dict(mean=emu, within=bw / (c * (n - 1)), between=bb / LD(c - 1), sigma=bsig, mcse_cov=bsig / big,
                          ess_bm=r["ess_bm"] * (np.diag(bl) / np.diag(lam) + np.diag(bsig) / np.diag(r["sigma"]) + 4 * U))
    w64, b64, s64 = (np.asarray(r[q], dtype=np.float64) for q in ("within", "between", "sigma"))
    r["mess"] = r["mpsrf"] = math.nan
    r["conds"] = []
    if c * a - 1 >= k:
        r["mess"] = big * math.exp((np.linalg.slogdet(np.asarray(lam, dtype=np.float64))[1] - np.linalg.slogdet(s64)[1]) / k)
        r["conds"].append(np.linalg.cond(s64))
    if c >= 2 and c * (n - 1) >= k and np.all(np.isfinite(w64)):
        li = np.linalg.inv(np.linalg.cholesky(w64))
        r["mpsrf"] = math.sqrt((n - 1) / n + (c + 1) / c * np.linalg.eigvalsh(li @ b64 @ li.T)[-1])
        r["conds"].append(np.linalg.cond(w64))
    return r


_DRIVER = r'''
#include <cstring>
// joint_run's launches (csrc/draws.cpp) by its own plan (the cap a parameter), one workgroup after the other, and its host finish
extern "C" int rj_emulate(const double *draws, int C, long long iterations, long long nvars, long long first, long long count, long long batch,
                          const int *cols, int K, long long cap, double *scal, double *ess, double *mu, double *mats, long long *plan) {
  const rh_plan::Joint P = rh_plan::joint_plan(C, count, batch, K, cap);
  const long long v[10] = {P.b, P.a, P.dropped, P.S[0], P.S[1], P.S[2], P.pairs, P.pc, P.chunks, P.over_cap};
  std::memcpy(plan, v, sizeof v);
  if (P.over_cap || P.a < 2 || !draws) return -1;
  const size_t kk = (size_t)K * K, tile = RC_TC * RC_TC;
  std::vector<double> ybar((size_t)C * P.a * K), m((size_t)C * K), ts((size_t)C * K), ws((size_t)P.pc * (P.S[0] + P.S[1] + P.S[2]) * tile), lds(RC_TILE_LDS), M(4 * kk);
  const double *base = draws + (first + P.dropped) * nvars;
  for (long long bid = 0; bid < C * P.ctiles; bid++)
    rj_batch_chain(base, iterations, nvars, cols, K, (int)(bid % P.ctiles) * RC_TC, bid / P.ctiles, P.b, P.a, lds.data(), ybar.data(), m.data(), ts.data(), RC_BLOCK);
  for (int k = 0; k < K; k++) mu[k] = rj_mean(ts.data(), C, K, k, P.N);
  const rj_src src[3] = {{base, P.np, iterations * nvars, nvars, cols, m.data(), K}, {ybar.data(), P.R[1], 0, K, nullptr, mu, 0}, {m.data(), P.R[2], 0, K, nullptr, mu, 0}};
  double *w[3] = {ws.data(), ws.data() + P.pc * P.S[0] * tile, ws.data() + P.pc * (P.S[0] + P.S[1]) * tile};
  for (long long p0 = 0; p0 < P.pairs; p0 += P.pc) {
    const long long p_cnt = P.pc < P.pairs - p0 ? P.pc : P.pairs - p0;
    int bi, bj;
    for (int g = 0; g < 3; g++)
      for (long long bid = 0; bid < p_cnt * P.S[g]; bid++) {
        rc_pair_of(p0 + bid / P.S[g], (int)P.ctiles, &bi, &bj);
        rj_gram_split(src[g], P.R[g], K, bi, bj, bid % P.S[g], lds.data(), w[g] + bid * tile, RC_BLOCK);
      }
    for (long long pl = 0; pl < p_cnt; pl++) {
      rc_pair_of(p0 + pl, (int)P.ctiles, &bi, &bj);
      rj_finish_pair(w[0] + pl * P.S[0] * tile, w[1] + pl * P.S[1] * tile, w[2] + pl * P.S[2] * tile, P.S[0], P.S[1], P.S[2], C, P.a, P.b, bi, bj, K,
                     M.data(), M.data() + kk, M.data() + 2 * kk, M.data() + 3 * kk, RC_BLOCK);
    }
  }
  bool repeated = false;
  for (int i = 0; i < K; i++) for (int j = 0; j < i; j++) repeated |= cols[i] == cols[j];
  rh_plan::joint_figures(P, C, K, repeated, M.data(), M.data() + kk, M.data() + 2 * kk, M.data() + 3 * kk, m.data(), mu, scal, scal + 1, ess, mats + 3 * kk);
  std::memcpy(mats, M.data(), 3 * kk * sizeof(double));
  return (int)P.chunks;
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_cov.hip.h and rh_joint.hip.h in host mode) + the driver above as a host shared library"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_joint_emu")
        open(os.path.join(d, "emu.cpp"), "w").write('#include "%s"\n%s' % (os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp"), _DRIVER))
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", os.path.join(d, "emu.cpp"),
                               "-o", os.path.join(d, "emu.so")])
        _emu = C.CDLL(os.path.join(d, "emu.so"))
        dp, ll = C.POINTER(C.c_double), C.c_longlong
        _emu.rj_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, C.POINTER(C.c_int), C.c_int, ll, dp, dp, dp, dp, C.POINTER(ll)]
    return _emu


def emulate(x, first=0, count=None, batch=0, cols=None, cap=CAP):
    """the host emulation over x [chains][iterations][nvars] -> a dict shaped like JointDiagnostics (and "chunks")"""
    c, iters, nv = x.shape
    x = np.ascontiguousarray(x, dtype=np.float64)
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    k = len(sel)
    scal, ess, mu, mats, plan = np.zeros(2), np.zeros(k), np.zeros(k), np.zeros((4, k, k)), (C.c_longlong * 10)()
    n = emulation().rj_emulate(_capi.dptr(x), c, iters, nv, first, iters - first if count is None else count, batch,
                        sel.ctypes.data_as(C.POINTER(C.c_int)), k, cap, _capi.dptr(scal), _capi.dptr(ess), _capi.dptr(mu), _capi.dptr(mats), plan)
    return dict(mess=scal[0], mpsrf=scal[1], ess_bm=ess, mean=mu, within=mats[0], between=mats[1], sigma=mats[2], mcse_cov=mats[3],
                batch=plan[0], batches=plan[1], dropped=plan[2], chunks=n)


def check(got, ref, what, scalars=True):
    """got: a dict or a JointDiagnostics.  Every matrix, mean and ess_bm within the derived bounds of the reference (NaN where it is
    NaN), bitwise symmetric; ess_bm exactly N Lambda_ii / Sigma_ii of the returned matrices; the scalars NaN by shape or within 1e-9"""
    g = got if isinstance(got, dict) else got._asdict()
    assert (g["batch"], g["batches"], g["dropped"]) == (ref["batch"], ref["batches"], ref["dropped"]), what
    for q in ("mean", "ess_bm") + MATS:
        v, r, bound = np.asarray(g[q]).astype(LD), ref[q], ref["bound"][q]
        assert np.array_equal(np.isnan(v), np.isnan(r)), (what, q, "NaN pattern")
        ok = ~np.isnan(r)
        assert np.all(np.abs(v - r)[ok] <= bound[ok]), (what, q, float(np.max((np.abs(v - r) - bound)[ok])))
        assert q not in MATS or same_bits(g[q], np.asarray(g[q]).T), (what, q, "not bitwise symmetric")
    n, c, big = ref["batch"] * ref["batches"], ref["N"] // (ref["batch"] * ref["batches"]), float(ref["N"])
    with np.errstate(invalid="ignore", divide="ignore"):
        w, bn = np.diag(g["within"]), np.diag(g["between"])
        lam = w if c == 1 else (float(c * (n - 1)) * w + float(n * (c - 1)) * bn) / float(big - 1)
        assert same_bits(g["ess_bm"], big * lam / np.diag(g["sigma"])), (what, "ess_bm is not N Lambda_ii / Sigma_ii")
    for q in ("mess", "mpsrf"):
        print(what, q, g[q], ref[q])
        assert math.isnan(g[q]) == math.isnan(ref[q]), (what, q, g[q], ref[q])
        assert not scalars or math.isnan(ref[q]) or abs(g[q] - ref[q]) <= 1e-9 * abs(ref[q]), (what, q, g[q], ref[q])
    assert not scalars or all(cd <= 1e4 for cd in ref["conds"]), (what, ref["conds"])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("chains,count", CASES)
def test_host_emulation_against_the_reference(chains, count, k):
    x = fixture(chains, count, k)
    got, ref = emulate(x), reference(x)
    check(got, ref, (chains, count, k))
    assert math.isnan(got["mess"]) == (chains * ref["batches"] - 1 < k) and math.isnan(got["mpsrf"]) == (chains < 2 or chains * (ref["batch"] * ref["batches"] - 1) < k)
    if k == 1 and chains > 1:       # the scalar form of the MPSRF, from the returned figures
        n = ref["batch"] * ref["batches"]
        want = (n - 1) / n + (chains + 1) / chains * (got["between"][0, 0] / got["within"][0, 0])
        assert abs(got["mpsrf"] ** 2 - want) <= 4 * np.spacing(want)


@pytest.mark.parametrize("k", [5, 65])
def test_windows_batches_column_lists_and_chunks(k):
    x = fixture(3, 120, k)
    full = emulate(x, 7, 100, 9)                                        # first > 0, an explicit batch that does not divide count
    check(full, reference(x, 7, 100, 9), ("window", k))
    copy = emulate(np.ascontiguousarray(x[:, 7:107]), batch=9)
    cols = [int(c) for c in np.random.default_rng(k).permutation(k)[:max(2, (2 * k) // 3)]]
    sub, one = emulate(x, 7, 100, 9, cols=cols), emulate(x, 7, 100, 9, cap=3 * 32768)      # ... and one tile pair per chunk
    assert one["chunks"] == (1 if k == 5 else 3) and full["chunks"] == 1
    for q in ("mean", "ess_bm") + MATS:
        assert same_bits(full[q], copy[q]) and same_bits(full[q], one[q]), q
        assert same_bits(sub[q], full[q][cols] if full[q].ndim == 1 else full[q][np.ix_(cols, cols)]), q
    check(sub, reference(x, 7, 100, 9, cols), ("cols", k))
    twice = emulate(x, 7, 100, 9, cols=cols + cols[:1])                  # singular by construction
    assert math.isnan(twice["mess"]) and math.isnan(twice["mpsrf"]) and same_bits(twice["within"][:-1, :-1], sub["within"])


def test_scaling_and_a_chain_that_sits_elsewhere():
    x = fixture(8, 400, 5)                # more chains than columns: the finish takes the K x K eigenproblem
    base, ref = emulate(x), reference(x)
    scaled = emulate(x * 2.0 ** np.array([3, -2, 0, 7, -5]))
    moved = fixture(8, 400, 5, stuck=10.0)
    got, mref = emulate(moved), reference(moved)
    check(got, mref, "moved")
    assert all(abs(scaled[q] - base[q]) <= 1e-12 * base[q] for q in ("mess", "mpsrf"))
    assert got["mess"] < base["mess"] and got["mpsrf"] > 1.1 and got["mpsrf"] > base["mpsrf"] and abs(base["mess"] - ref["mess"]) <= 1e-9 * ref["mess"]


def test_a_nan_column_touches_nothing_else():
    x = fixture(3, 33, 65, nan_col=64)
    got, clean = emulate(x), emulate(x, cols=list(range(64)))
    check(got, reference(x), "nan", scalars=False)
    assert math.isnan(got["mess"]) and math.isnan(got["mpsrf"]) and math.isnan(got["mean"][64]) and not math.isnan(clean["mpsrf"])
    for q in MATS:
        assert np.all(np.isnan(got[q][64])) and np.all(np.isnan(got[q][:, 64])) and same_bits(got[q][:64, :64], clean[q])


def test_the_code_object_the_plan_and_what_is_refused():
    assert len(_capi.joint_lower_only()) > 1000
    L, ip, fake = _capi.lib(), C.POINTER(C.c_int32), C.c_void_p(4096)    # never dereferenced: refused before the first device call
    out = (C.c_longlong * 10)()     # b, a, dropped, the three Grams' splits, pairs, pairs per chunk, chunks, over the cap
    for (c, n, b, k, cap), want in (((1, 4096, 1, 1, CAP), [1, 4096, 0, 1, 1, 1, 1, 1, 1, 0]), ((1, 4097, 1, 65, CAP), [1, 4097, 0, 2, 2, 1, 3, 3, 1, 0]),
                                    ((5, 900, 0, 256, 4 * 32768), [30, 30, 0, 2, 1, 1, 10, 1, 10, 0]), ((5, 901, 0, 1, 4 * 32768 - 1), [30, 30, 1, 2, 1, 1, 1, 1, 1, 1])):
        emulation().rj_emulate(None, c, n, 1, 0, n, b, None, k, cap, None, None, None, None, out)
        assert list(out) == want, (c, n, b, k, list(out))

    def call(ptr=fake, chains=4, iters=100, nvars=2, first=0, count=100, batch=0, cols=None):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        return L.rh_joint_diagnostics_device(ptr, 0, chains, iters, nvars, first, count, batch, sel.ctypes.data_as(ip) if cols is not None else None,
                                             len(cols) if cols is not None else 0, *([None] * 9))
    for kw in (dict(ptr=None), dict(count=3), dict(count=101), dict(first=-1), dict(batch=-1), dict(batch=51), dict(cols=[2]), dict(cols=[0, -1]), dict(chains=0)):
        assert call(**kw) == _capi.RH_E_INVALID, kw
    assert call(nvars=257) == _capi.RH_E_UNSUPPORTED and "256" in L.rh_last_error(None).decode()
    assert call(chains=4097, iters=4096, count=4096, batch=1) == _capi.RH_E_UNSUPPORTED and "workspace" in L.rh_last_error(None).decode()
    assert L.rh_sampler_joint_diagnostics(None, 0, 100, 0, None, 0, *([None] * 9)) == _capi.RH_E_INVALID
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and call(nvars=256, cols=[1, 0]) == _capi.RH_E_DEVICE
    import rainier_amd as R
    assert R.JointDiagnostics._fields == ("mess", "mpsrf", "ess_bm", "mean") + MATS + ("batch", "batches", "dropped", "cols")
