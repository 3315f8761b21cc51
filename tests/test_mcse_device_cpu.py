"""Monte Carlo standard errors and ESS of the reported figures on the device (csrc/device/rh_mcse.hip.h; Vehtari, Gelman, Simpson,
Carpenter, Buerkner 2021, section 4), the part that needs no GPU:

  * the device source cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck), its kernels use
    no scratch and spill nothing, and the code objects of the other families do not carry it;
  * the very text of its block routines, compiled with the host g++ (contraction off) with every "thread" of a phase run in turn, is
    driven over whole buffers exactly as the launches walk them (the workspace cap a parameter of the driver) -- the emulation -- and
    compared with an independent numpy / np.longdouble restatement:
      - m_q and g_q(t) of every series (3 + nprobs per column, remade here from y, the emulation's pooled mean and its thresholds --
        the device never writes them) at the rank diagnostics' derived bounds, (h + 2) u and (h + 4) u;
      - every other figure with the restatement fed with those series: every comparison of the estimator's scan and every floor /
        ceil of the quantiles' brackets is first shown to be decided by more than 1e-6, then flags and indices are equal and the
        figures within four times the largest relative difference measured here (profiles/mcse_device/README.md);
  * csrc/qbeta.hpp as a stand-alone host program (tools/qbeta_check.cpp, also under AddressSanitizer and UBSan) against mpmath at 40
    digits, scipy.special.betaincinv as a cross-check;
  * the pin to merged code: with probs = (0.05, 0.95) the smaller ess_quantile is rank_diagnostics' ess_tail, bit for bit;
  * the properties of the contract, the plan's arithmetic, the C ABI's argument errors and its refusal to compute without a device;
  * what the figures mean, on fixed seeds.

tests/test_gpu_mcse_device.py runs the same shapes through the kernels.
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
from tests.test_rank_diagnostics_device_cpu import (CAP, LD, MAXLAG, MERGE_TILE, NKINDS, SHAPES, TILE, ar1, case, check_sums, estimator, fixture, same_bits,
                                                    shuffled_with_duplicate, split, to_keys)
from tests import test_rank_diagnostics_device_cpu as RK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rh_mcse_stage_kernel", "rh_mcse_sort_kernel", "rh_mcse_merge_kernel", "rh_mcse_moment_kernel", "rh_mcse_chain_kernel",
           "rh_mcse_finish_kernel", "rh_mcse_pick_kernel", "rh_mcse_combine_kernel")
P16, P84 = 0.15865525393145707, 0.8413447460685429
# the largest relative difference of a figure (absolute, for the autocorrelations) from the longdouble restatement measured over SHAPES
# (profiles/mcse_device/README.md); the tolerance is four times it
FIGURE_MEASURED = 3.1e-11
# the largest |qbeta - mpmath's root at 40 digits| measured over qbeta_grid() (profiles/mcse_device/README.md); the bound is four times it
QBETA_MEASURED = 6.1e-16
QBETA_SMAX = 4.2e6       # the largest S the issue's workspace figure admits: 128 MiB / 32 B
DOUBLES = ("mean", "sd", "ess_mean", "ess_sd", "mcse_mean", "mcse_sd", "quantile", "ess_quantile", "mcse_quantile", "acf")
FIELDS = DOUBLES + ("truncated",)
PROBS = (0.05, 0.5, 0.95)
NLAGS = (0, 7, 255)


def params(i):
    """the probabilities and lags of shape i: the tails' and the median's; nlags 0, 7 and 255 (beyond L where h <= 255) in turn"""
    return PROBS, NLAGS[i % 3]


# ---- the device text on the host -----------------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <vector>
// mcse_run's launches (csrc/draws.cpp) by its own plan (csrc/draws_plan.hpp; the cap a parameter) and the kernels' index arithmetic, one
// workgroup after the other.  Outputs as the C ABI's (none NULL here); ws_out [K][nseries][M][sl], fin_out [K][nseries][3], mom_out [K][3],
// pick_out [K][nprobs][3] and sorted_out [K][S] (doubles) may be NULL.  Returns the number of chunks, -1 beyond the cap.
extern "C" int mk_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, const int *cols, int K,
                          const double *probs, int nprobs, int nlags, long long cap, double *mean, double *sd, double *ess_mean, double *ess_sd, double *mcse_mean,
                          double *mcse_sd, double *quantile, double *ess_quantile, double *mcse_quantile, double *acf, int *truncated, double *ws_out,
                          double *fin_out, double *mom_out, long long *pick_out, double *sorted_out) {
  const rh_plan::Mcse P = rh_plan::mcse_plan(chains, count, K, probs, nprobs, cap);
  if (P.over_cap) return -1;
  const long long S = P.S, M = P.M;
  const int h = (int)P.h, ns = P.nseries;
  std::vector<double> y((size_t)(P.pc * S)), ws((size_t)(P.pc * ns * M * P.sl)), fin((size_t)K * ns * RK_NFIN), mom((size_t)K * MK_NMOM), lds(RK_LDS_DOUBLES);
  std::vector<rs_key> ka((size_t)(P.pc * S)), kb((size_t)(P.pc * S)), klds(RS_TILE_SLOTS > RS_MERGE_LDS ? RS_TILE_SLOTS : RS_MERGE_LDS);
  std::vector<long long> pick((size_t)(P.pc * (nprobs ? nprobs : 1) * MK_NPICK));
  std::vector<double> clds((size_t)(P.chain_lds / 8) + 64, -7.0);   // the chain launch's dynamic LDS, and a margin that must stay as it is
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0, ctiles = (p_cnt + RK_TP - 1) / RK_TP;
    for (long long bid = 0; bid < P.stiles * ctiles; bid++) {
      const long long rt = bid / ctiles, pl = (bid - rt * ctiles) * RK_TP, s0 = rt * RK_ROWS;
      if (s0 >= S || pl >= p_cnt) continue;
      rk_stage_tile(draws, iterations, nvars, first, count, P.h, S, cols + k0 + pl, (int)(p_cnt - pl < RK_TP ? p_cnt - pl : RK_TP), s0, lds.data(), y.data() + pl * S, MK_BLOCK);
    }
    rs_key *src = ka.data(), *dst = kb.data();
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++) {
      const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, g0 = tile * RS_TILE;
      if (g0 >= S) continue;
      rs_tile_sort(y.data() + pl * S, S, 1, 1, S, S, g0, klds.data(), src + pl * S + g0, MK_BLOCK);
    }
    for (int k = 0; k < P.passes; k++) {
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++) {
        const long long tile = bid / p_cnt, pl = bid - tile * p_cnt, o0 = tile * RS_MERGE_TILE;
        if (o0 >= S) continue;
        rs_merge_tile(src + pl * S, dst + pl * S, S, P.run(k), o0, klds.data(), MK_BLOCK);
      }
      std::swap(src, dst);
    }
    const rs_key *sy = src;
    for (long long pl = 0; pl < p_cnt; pl++) mk_moment_block(y.data() + pl * S, sy + pl * S, S, lds.data(), mom.data() + (k0 + pl) * MK_NMOM, MK_BLOCK);
    for (long long bid = 0; bid < p_cnt * ns * M; bid++) {
      const long long cs = bid / M, q = bid - cs * M, pl = cs / ns;
      const int kind = (int)(cs - pl * ns);
      const rs_key thr = kind >= MK_NFIXED ? sy[pl * S + P.idx[kind - MK_NFIXED]] : 0ull;
      mk_chain_block(y.data() + pl * S + q * h, kind, mom[(k0 + pl) * MK_NMOM], thr, h, P.L, clds.data(), ws.data() + bid * P.sl, MK_BLOCK);
    }
    for (size_t e = (size_t)(P.chain_lds / 8); e < clds.size(); e++)
      if (clds[e] != -7.0) return -2;               // a write beyond the launch's dynamic LDS
    for (long long bid = 0; bid < p_cnt * ns; bid++) {
      const long long pl = bid / ns;
      const int kind = (int)(bid - pl * ns);
      const double *w = ws.data() + bid * M * P.sl;
      double *f = fin.data() + ((k0 + pl) * ns + kind) * RK_NFIN;
      rk_series_finish(w, sy + pl * S, S, (int)M, h, P.L, P.sl, P.tau_min, lds.data(), f, MK_BLOCK);
      if (kind == 0) mk_acf(w, lds.data(), f, (int)M, h, P.L, P.sl, nlags, acf + (k0 + pl) * (nlags + 1), MK_BLOCK);
    }
    for (long long e = 0; e < p_cnt * nprobs; e++) {
      const long long pl = e / nprobs, k = e - pl * nprobs;
      rh_plan::mcse_pick(S, P.idx[k], probs[k], fin[((k0 + pl) * ns + MK_NFIXED + k) * RK_NFIN + 1], &pick[e * MK_NPICK]);
    }
    for (long long e = 0; e < p_cnt * nprobs; e++) {
      const long long pl = e / nprobs, o = k0 * nprobs + e;
      mk_pick(sy + pl * S, S, &pick[e * MK_NPICK], quantile + o, mcse_quantile + o);
      if (pick_out) for (int j = 0; j < MK_NPICK; j++) pick_out[o * MK_NPICK + j] = pick[e * MK_NPICK + j];
    }
    if (ws_out) for (long long e = 0; e < p_cnt * ns * M * P.sl; e++) ws_out[k0 * ns * M * P.sl + e] = ws[e];
    if (sorted_out) for (long long e = 0; e < p_cnt * S; e++) sorted_out[k0 * S + e] = rs_from_key(sy[e]);
  }
  for (int k = 0; k < K; k++)
    mk_combine(mom.data() + (size_t)k * MK_NMOM, fin.data() + (size_t)k * ns * RK_NFIN, S, nprobs, mean + k, sd + k, ess_mean + k, ess_sd + k, mcse_mean + k,
               mcse_sd + k, ess_quantile + (size_t)k * nprobs, truncated + k);
  if (fin_out) for (size_t i = 0; i < fin.size(); i++) fin_out[i] = fin[i];
  if (mom_out) for (size_t i = 0; i < mom.size(); i++) mom_out[i] = mom[i];
  return chunks;
}
// h, M, S, L, sl, nprobs, nseries, per_col, pc, over_cap, tiles, mtiles, passes, stiles, chain_lds, then idx [16]
extern "C" double mk_plan(long long chains, long long count, long long K, const double *probs, int nprobs, long long cap, long long *out) {
  const rh_plan::Mcse P = cap ? rh_plan::mcse_plan(chains, count, K, probs, nprobs, cap) : rh_plan::mcse_plan(chains, count, K, probs, nprobs);
  const long long v[15] = {P.h, P.M, P.S, P.L, P.sl, P.nprobs, P.nseries, P.per_col, P.pc, P.over_cap ? 1 : 0, P.tiles, P.mtiles, P.passes, P.stiles, P.chain_lds};
  for (int i = 0; i < 15; i++) out[i] = v[i];
  for (int i = 0; i < MK_MAXPROBS; i++) out[15 + i] = P.idx[i];
  return P.tau_min;
}
extern "C" void mk_constants(long long *out) { const long long v[6] = {MK_BLOCK, MK_MAXPROBS, MK_NFIXED, MK_NMOM, MK_NPICK, MK_WS_CAP_BYTES}; for (int i = 0; i < 6; i++) out[i] = v[i]; }
extern "C" void mk_pick_host(long long S, long long j, double p, double e, long long *pick) { rh_plan::mcse_pick(S, j, p, e, pick); }
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h, rh_rank.hip.h, rh_mcse.hip.h in host mode and qbeta.hpp) + the driver above as a
    host shared library (g++ -O2 -ffp-contract=off, as hiprtc is told for the device)"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_mcse_emu")
        src = os.path.join(d, "emu.cpp")
        hdr = os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp")
        open(src, "w").write('#include "%s"\n%s' % (hdr, _DRIVER))
        so = os.path.join(d, "emu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        dp, ll, ip, lp = C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
        L.mk_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ip, C.c_int, dp, C.c_int, C.c_int, ll] + [dp] * 10 + [ip, dp, dp, dp, lp, dp]
        L.mk_plan.argtypes = [ll, ll, ll, dp, C.c_int, ll, lp]
        L.mk_plan.restype = C.c_double
        L.mk_constants.argtypes = [lp]
        L.mk_pick_host.argtypes = [ll, ll, C.c_double, C.c_double, lp]
        _emu = L
    return _emu


PLAN_FIELDS = ("h", "M", "S", "L", "sl", "nprobs", "nseries", "per_col", "pc", "over_cap", "tiles", "mtiles", "passes", "stiles", "chain_lds")


def plan(chains, count, k, probs=PROBS, cap=0):
    out = (C.c_longlong * 31)()
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    tau_min = emulation().mk_plan(chains, count, k, _capi.dptr(pr) if len(pr) else None, len(pr), cap, out)
    return dict(zip(PLAN_FIELDS, list(out)[:15]), idx=list(out)[15:15 + len(pr)], tau_min=tau_min)


def emulate(x, first=0, count=None, cols=None, probs=PROBS, nlags=0, cap=CAP, dump=False):
    """the host emulation over x [chains][iterations][nvars] -> dict of the eleven outputs, "chunks", and with dump ws [K][nseries][M][sl],
    fin [K][nseries][3], mom [K][3], pick [K][nprobs][3] and sorted [K][S]"""
    L = emulation()
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, nv = x.shape
    count = iters - first if count is None else count
    sel = np.ascontiguousarray(range(nv) if cols is None else cols, dtype=np.int32)
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    k, npr = len(sel), len(pr)
    p = plan(m, count, k, probs, cap)
    out = {f: np.full(k, -1.0) for f in DOUBLES[:6]}
    out.update({f: np.full((k, npr), -1.0) for f in DOUBLES[6:9]})
    out["acf"] = np.full((k, nlags + 1), -1.0)
    out["truncated"] = np.full(k, -1, dtype=np.int32)
    dumps = {}
    if dump:
        dumps = dict(ws=np.zeros((k, p["nseries"], p["M"], p["sl"])), fin=np.zeros((k, p["nseries"], 3)), mom=np.zeros((k, 3)),
                     pick=np.zeros((k, npr, 3), dtype=np.int64), sorted=np.zeros((k, p["S"])))
    dptr = lambda name: _capi.dptr(dumps[name]) if dump else None
    n = L.mk_emulate(_capi.dptr(x), m, iters, nv, first, count, sel.ctypes.data_as(C.POINTER(C.c_int)), k, _capi.dptr(pr) if npr else None, npr, nlags, cap,
                     *[_capi.dptr(out[f]) for f in DOUBLES], out["truncated"].ctypes.data_as(C.POINTER(C.c_int)), dptr("ws"), dptr("fin"), dptr("mom"),
                     dumps["pick"].ctypes.data_as(C.POINTER(C.c_longlong)) if dump else None, dptr("sorted"))
    assert n != -2, "the chain routine wrote beyond the launch's dynamic LDS"
    assert n >= 1, "beyond the cap"
    out.update(dumps, chunks=n)
    return out


_cases = {}


def emulated_case(i):
    """(x, first, count, the emulation's result with its dumps) of shape i with params(i), computed once and shared (the GPU tests compare with it)"""
    if i not in _cases:
        x, first, count = case(i)
        probs, nlags = params(i)
        _cases[i] = (x, first, count, emulate(x, first, count, probs=probs, nlags=nlags, dump=True))
    return _cases[i]


def same_results(a, b, cols=None):
    """entry k of a has the bits of entry cols[k] of b, in all eleven outputs"""
    ix = slice(None) if cols is None else list(cols)
    return all(same_bits(np.asarray(a[f], dtype=np.float64), np.asarray(b[f], dtype=np.float64)[ix]) for f in FIELDS)


# ---- the independent restatement -----------------------------------------------------------------------------------------------------
def series_of(y, m, sk, idx):
    """y [M][h], the pooled mean the device used, the sorted keys and the order statistics -> the 3 + nprobs series in float64 (each one
    operation on y, so numpy gives the device's bits)"""
    d = y - m
    return [y, np.abs(d), d * d] + [(to_keys(y) <= sk[j]).astype(np.float64) for j in idx]


def rel(got, want):
    if math.isnan(want) or math.isnan(got):
        assert math.isnan(want) and math.isnan(got), (got, want)
        return 0.0
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def restate_column(y, probs, nlags, m_used=None):
    """One finite column y [M][h] in longdouble (the series made in float64 from m_used, the emulation's pooled mean, or from the
    restatement's own) -> dict of the figures, "margin" (the least by which a comparison or a floor / ceil was decided) and "pick"."""
    from scipy.special import betaincinv
    M, h = y.shape
    S = M * h
    flat = y.ravel()
    fl = flat.astype(LD)
    m = fl.sum() / LD(S)
    mu = float(m) if m_used is None else m_used
    d = fl - LD(mu)
    e2, e4 = (d * d).sum() / LD(S), ((d * d) * (d * d)).sum() / LD(S)
    sd = np.sqrt(LD(S) * e2 / LD(S - 1))
    order = np.argsort(to_keys(flat), kind="stable")
    sv, sk = flat[order], to_keys(flat)[order]
    idx = [min(S - 1, int(math.floor(float(S) * p))) for p in probs]
    ser = series_of(y, mu, sk, idx)
    est = [estimator(u, dtype=LD) for u in ser]          # rhat, ess, truncated, stop, margin, m, g
    margin = min(e[4] for e in est if not math.isnan(e[1])) if any(not math.isnan(e[1]) for e in est) else math.inf
    ess = [LD(e[1]) for e in est]
    out = dict(mean=m, sd=sd, ess_mean=ess[0], ess_sd=ess[1], mcse_mean=sd / np.sqrt(ess[0]),
               mcse_sd=np.sqrt((e4 - e2 * e2) / ess[2] / e2 / LD(4)), e2=e2, e4=e4, quantile=[sv[j] for j in idx], ess_quantile=ess[3:],
               truncated=sum(e[2] << b for b, e in enumerate(est)), series=ser)
    picks, mq = [], []
    for k, p in enumerate(probs):
        e = float(ess[3 + k])
        if math.isnan(e):
            picks.append((idx[k], -1, -1)); mq.append(float("nan"))
            continue
        a, b = betaincinv(e * p + 1.0, e * (1.0 - p) + 1.0, P16) * S, betaincinv(e * p + 1.0, e * (1.0 - p) + 1.0, P84) * S
        margin = min(margin, abs(a - round(a)), abs(b - round(b)))
        i1, i2 = max(int(math.floor(a)), 1) - 1, min(int(math.ceil(b)), S) - 1
        picks.append((idx[k], i1, i2)); mq.append((sv[i2] - sv[i1]) / 2.0)
    out.update(pick=picks, mcse_quantile=mq, margin=margin)
    # the autocorrelations of series A from the estimator's own longdouble sums
    L = min(h - 1, MAXLAG)
    mq_, g = est[0][5], est[0][6]
    gm = g.sum(axis=1) / LD(M)
    W = gm[0] * LD(h) / LD(h - 1)
    B = ((mq_ - mq_.sum() / LD(M)) ** 2).sum() / LD(M - 1)
    V = LD(h - 1) / LD(h) * W + B
    acf = np.full(nlags + 1, np.nan, dtype=LD)
    if not math.isnan(float(ess[0])):
        n = min(nlags, L)
        acf[:n + 1] = LD(1) - (W - gm[:n + 1]) / V
        acf[0] = LD(1)
    out["acf"] = acf
    return out


# ---- 1. the code object --------------------------------------------------------------------------------------------------------------
def test_mcse_kernels_cross_compile_without_spills_or_scratch():
    code = _capi.mcse_lower_only("gfx950")
    rep = _capi.code_object_report(code)
    for k in KERNELS:
        assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
        assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
        r = rep[("object", k)]
        assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r   # kernel_health: metadata + isacheck's walk
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.mcse.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.mcse_lower_only("gfx950") == code and _capi.lib().rh_compile_count() == before      # served by the kernel cache


def test_the_other_code_objects_do_not_carry_the_mcse_kernels():
    """the existing families' translation units are what they were: none holds a word of this one, and each is still served by the
    kernel cache under its own key (their bytes against the parent commit's: profiles/mcse_device/README.md)"""
    from rainier_amd import models
    src, _ = _capi.lower_only(models.funnel(10).rir, compile=False)
    assert "rh_mcse" not in src
    for lower in (_capi.trace_lower_only, _capi.summary_lower_only, _capi.rank_lower_only, _capi.covariance_lower_only, _capi.histogram_lower_only,
                  _capi.loo_lower_only, _capi.loo_expect_lower_only, _capi.loo_quantile_lower_only, _capi.ppc_lower_only, _capi.generate_lower_only,
                  _capi.generate_ext_lower_only):
        code = lower("gfx950")
        assert b"rh_mcse" not in code, lower.__name__
        before = _capi.lib().rh_compile_count()
        assert lower("gfx950") == code and _capi.lib().rh_compile_count() == before
    assert b"rh_mcse_chain_kernel" in _capi.mcse_lower_only("gfx950")


def test_exports_and_python_surface():
    import inspect
    import rainier_amd as R
    L = _capi.lib()
    for name in ("rh_sampler_mcse", "rh_mcse_device", "rh_mcse_lower_only"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    assert L.rh_abi_version() == 6
    assert R.Mcse._fields == FIELDS + ("cols", "probs")
    assert list(inspect.signature(R.Sampler.mcse).parameters) == ["self", "first", "count", "cols", "probs", "nlags"]
    assert list(inspect.signature(R.mcse_device).parameters) == ["ptr", "chains", "iterations", "nvars", "device", "first", "count", "cols", "probs", "nlags"]
    sig = inspect.signature(R.Sampler.mcse).parameters
    assert sig["first"].default == 0 and sig["count"].default is None and sig["cols"].default is None and sig["nlags"].default == 0


# ---- 2. the device text, on the host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_sums_and_figures_against_the_longdouble_restatement(i):
    x, first, count, emu = emulated_case(i)
    probs, nlags = params(i)
    h = count // 2
    L = min(h - 1, MAXLAG)
    tol = 4 * FIGURE_MEASURED
    worst = 0.0
    ys = split(x, first, count)
    for k in range(min(x.shape[2], NKINDS)):                # every kind of column
        y = ys[k]
        ref = restate_column(y, probs, nlags, m_used=float(emu["mom"][k, 0]))
        # the sorted column and the quantiles: order statistics, exact
        assert np.array_equal(emu["sorted"][k], np.sort(y.ravel())) and same_bits(emu["quantile"][k], ref["quantile"])
        # the sums of every series at the derived bounds
        for s, u in enumerate(ref["series"]):
            check_sums(u, emu["ws"][k, s], L, (SHAPES[i], k, s))
        # every comparison of the scans and every floor / ceil is decided clearly under the restatement (else the fixture's seed is changed) ...
        assert ref["margin"] > 1e-6, (SHAPES[i], k, ref["margin"])
        # ... so flags and indices are equal, the bracket's figure has the restatement's bits, and the other figures are close
        assert emu["truncated"][k] == ref["truncated"], (SHAPES[i], k)
        assert [tuple(r) for r in emu["pick"][k]] == ref["pick"], (SHAPES[i], k, emu["pick"][k], ref["pick"])
        assert same_bits(emu["mcse_quantile"][k], ref["mcse_quantile"])
        figs = [(float(emu[f][k]), float(ref[f])) for f in ("mean", "sd", "ess_mean", "ess_sd", "mcse_mean", "mcse_sd")]
        figs += [(float(emu["mom"][k, 1]), float(ref["e2"])), (float(emu["mom"][k, 2]), float(ref["e4"]))]
        figs += [(float(a), float(b)) for a, b in zip(emu["ess_quantile"][k], ref["ess_quantile"])]
        for got, want in figs:
            r = rel(got, want)
            assert r <= tol, (SHAPES[i], k, got, want)
            worst = max(worst, r)
        assert np.array_equal(np.isnan(emu["acf"][k]), np.isnan(ref["acf"].astype(np.float64))), (SHAPES[i], k)
        ok = ~np.isnan(emu["acf"][k])
        if ok.any():
            a = float(np.max(np.abs(emu["acf"][k][ok].astype(LD) - ref["acf"][ok])))
            assert a <= tol and emu["acf"][k, 0] == 1.0, (SHAPES[i], k, a)
            worst = max(worst, a)
        assert np.all(np.isnan(emu["acf"][k, L + 1:]))      # beyond L
    print("largest relative difference of a figure from the longdouble restatement: %.3g" % worst)
    assert worst <= FIGURE_MEASURED


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_tail_quantiles_pin_to_the_rank_diagnostics(i):
    """with probs = (0.05, 0.95) the indicator series are the rank diagnostics' tails: the same values through the same arithmetic"""
    x, first, count = case(i)
    rank = RK.emulated_case(i)[3]
    got = emulate(x, first, count, probs=(0.05, 0.95))
    lo, hi = got["ess_quantile"][:, 0], got["ess_quantile"][:, 1]
    with np.errstate(invalid="ignore"):
        tail = np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.minimum(lo, hi))
    assert same_bits(tail, rank["ess_tail"]), SHAPES[i]
    assert np.array_equal((got["truncated"] >> 3) & 3, (rank["truncated"] >> 1) & 3), SHAPES[i]
    # ... and the shared case's tails are those too
    emu = emulated_case(i)[3]
    assert same_bits(emu["ess_quantile"][:, [0, 2]], got["ess_quantile"])


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_properties_of_the_contract(i):
    x, first, count, emu = emulated_case(i)
    probs, nlags = params(i)
    chains, _ = SHAPES[i]
    nv = x.shape[2]
    kw = dict(probs=probs, nlags=nlags)
    # a window gives the bits of its copy
    assert same_results(emulate(np.ascontiguousarray(x[:, first:first + count, :]), **kw), emu), SHAPES[i]
    # a shuffled column list with a duplicate gives the bits of the full call's entries
    cols = shuffled_with_duplicate(nv, i)
    assert same_results(emulate(x, first, count, cols=cols, **kw), emu, cols), SHAPES[i]
    # forcing several chunks gives the same bits
    if nv > 1:
        p = plan(chains, count, nv, probs)
        small = emulate(x, first, count, cap=2 * p["per_col"], **kw)
        assert small["chunks"] == -(-nv // 2) and emu["chunks"] == 1 and same_results(small, emu), SHAPES[i]
    # no probabilities, sixteen of them, no lags, all lags: the shared figures keep their bits
    none = emulate(x, first, count, probs=(), nlags=255 - nlags)
    many = tuple(np.linspace(0.03, 0.97, 16))
    full = emulate(x, first, count, probs=many, nlags=0)
    for f in DOUBLES[:6]:
        assert same_bits(none[f], emu[f]) and same_bits(full[f], emu[f]), (SHAPES[i], f)
    assert none["quantile"].shape == (nv, 0) and np.array_equal(none["truncated"], emu["truncated"] & 7) and np.array_equal(full["truncated"] & 7, emu["truncated"] & 7)
    n = min(nlags, 255 - nlags)
    assert same_bits(none["acf"][:, :n + 1], emu["acf"][:, :n + 1]) and same_bits(full["acf"][:, 0], emu["acf"][:, 0])
    S, L = 2 * chains * (count // 2), min(count // 2 - 1, MAXLAG)
    assert np.array_equal(full["quantile"], np.sort(split(x, first, count).reshape(nv, -1), axis=1)[:, [min(S - 1, int(math.floor(S * p))) for p in many]])
    # a constant column keeps its mean and sd and has no ess; the others are finite
    for k in range(nv):
        if k % NKINDS == 4:
            assert emu["mean"][k] == 2.0 and emu["sd"][k] == 0.0 and np.all(emu["quantile"][k] == 2.0) and emu["truncated"][k] == 0
            assert all(np.all(np.isnan(emu[f][k])) for f in ("ess_mean", "ess_sd", "mcse_mean", "mcse_sd", "ess_quantile", "mcse_quantile", "acf"))
        else:
            assert all(np.isfinite(emu[f][k]) for f in DOUBLES[:6]), (SHAPES[i], k)
            assert np.all(np.isfinite(emu["acf"][k, :min(nlags, L) + 1])) and np.isfinite(emu["ess_quantile"][k, 1]) and np.isfinite(emu["mcse_quantile"][k, 1])


def test_nan_and_inf_columns_are_nan_and_touch_nothing_else():
    x, first, count = case(5)                               # 5 chains, count 819, 17 columns
    clean = emulate(x, first, count, nlags=5)
    bad = x.copy()
    bad[2, first + 100, 0] = np.nan
    bad[4, first + 7, 6] = np.inf
    bad[0, first + count - 1, 9] = -np.inf
    bad[1, first + count // 2, 3] = np.nan                  # count is odd: the middle draw is left out, the column stays clean
    bad[0, first - 1, 1] = np.nan                           # outside the window
    got = emulate(bad, first, count, nlags=5)
    for k in range(x.shape[2]):
        if k in (0, 6, 9):
            assert all(np.all(np.isnan(got[f][k])) for f in DOUBLES) and got["truncated"][k] == 0, k
        else:
            assert all(same_bits(got[f][k], clean[f][k]) for f in FIELDS), k


def test_the_plan_is_arithmetic_over_the_headers_constants():
    consts = (C.c_longlong * 6)()
    emulation().mk_constants(consts)
    assert list(consts) == [256, 16, 3, 3, 3, CAP]
    for chains, count, k, probs in ((1, 4, 1, ()), (2, 9, 5, PROBS), (3, 513, 17, (0.5,)), (1, 16131, 3, tuple(np.linspace(0.03, 0.97, 16))),
                                    (1024, 200, 5, PROBS), (64, 2000, 40, PROBS)):
        h, M = count // 2, 2 * chains
        S, L, ns = M * h, min(h - 1, MAXLAG), 3 + len(probs)
        per = 24 * S + 8 * ns * M * (L + 2)                 # y and two key buffers; no series buffer
        tiles, passes = -(-S // TILE), 0
        while TILE << passes < S:
            passes += 1
        want = dict(h=h, M=M, S=S, L=L, sl=L + 2, nprobs=len(probs), nseries=ns, per_col=per, pc=max(1, min(CAP // per, k)), over_cap=0, tiles=tiles,
                    mtiles=-(-S // MERGE_TILE), passes=passes, stiles=-(-S // 256), chain_lds=8 * min(max(h, 256), 8064), idx=[min(S - 1, int(math.floor(S * p))) for p in probs], tau_min=1.0 / math.log10(S))
        assert plan(chains, count, k, probs) == want, (chains, count, k)
    # the GPU tier's buffer that crosses the cap: the smallest number of columns of 64 chains x 2000 that does
    p = plan(64, 2000, 40, PROBS)
    assert p["per_col"] == 24 * 128000 + 8 * 6 * 128 * 257 and p["pc"] == CAP // p["per_col"] == 28 and 29 * p["per_col"] > CAP
    # a single column beyond the cap, from the shape alone; more probabilities need more
    per = lambda chains, ns: 2 * chains * (24 * 1024 + 8 * ns * 257)
    assert per(2182, 3) <= CAP < per(2183, 3) and per(1054, 19) <= CAP < per(1055, 19)
    assert plan(2182, 2048, 1, ())["over_cap"] == 0 and plan(2183, 2048, 1, ())["over_cap"] == 1 and plan(2183, 2048, 1, ())["pc"] == 1
    many = tuple(np.linspace(0.03, 0.97, 16))
    assert plan(1054, 2048, 1, many)["over_cap"] == 0 and plan(1055, 2048, 1, many)["over_cap"] == 1
    x = fixture(2, 40, 3, 1)
    pr = np.array(PROBS)
    assert emulation().mk_emulate(_capi.dptr(x), 2, 40, 3, 0, 40, None, 3, _capi.dptr(pr), 3, 0, plan(2, 40, 3)["per_col"] - 1, *[None] * 16) == -1


def test_the_brackets_of_a_quantile():
    """mcse_pick: the order statistics at the 16 % and 84 % points of Beta(e p + 1, e (1 - p) + 1), clipped to the column; no ess, no bracket"""
    from scipy.special import betaincinv
    pick = (C.c_longlong * 3)()
    for S, p, e in ((4000, 0.5, 4000.0), (4000, 0.05, 812.5), (128000, 0.95, 3.7), (16, 0.5, 1e-3), (16, 0.99, 40.0), (4200000, 0.5, 4.2e6 * 6.6)):
        j = min(S - 1, int(math.floor(S * p)))
        emulation().mk_pick_host(S, j, p, e, pick)
        a, b = betaincinv(e * p + 1, e * (1 - p) + 1, [P16, P84]) * S
        assert min(abs(a - round(a)), abs(b - round(b))) > 1e-6
        assert list(pick) == [j, max(int(math.floor(a)), 1) - 1, min(int(math.ceil(b)), S) - 1] and 0 <= pick[1] <= pick[2] <= S - 1, (S, p, e)
    for e in (float("nan"), 0.0, -1.0, float("inf")):
        emulation().mk_pick_host(100, 50, 0.5, e, pick)
        assert list(pick) == [50, -1, -1]


# ---- 3. qbeta as a stand-alone host program --------------------------------------------------------------------------------------------
def qbeta_grid():
    """(p, a, b): the two probabilities at shapes e q + 1, e (1 - q) + 1 from 1.05 up to 4.2e6, and the corners"""
    grid = []
    for e in (5.0, 1.0, 7.3, 100.0, 4000.0, 1.2e5, QBETA_SMAX):
        for q in (0.01, 0.05, 0.5, 0.95, 0.99):
            a, b = e * q + 1, e * (1 - q) + 1
            if min(a, b) >= 1.05 and max(a, b) <= QBETA_SMAX + 1:
                grid += [(P16, a, b), (P84, a, b)]
    for a, b in ((1.05, 1.05), (1.05, QBETA_SMAX), (QBETA_SMAX, 1.05), (QBETA_SMAX, QBETA_SMAX)):
        grid += [(P16, a, b), (P84, a, b)]
    return grid


def build_qbeta_check(flags=()):
    d = tempfile.mkdtemp(prefix="rh_qbeta")
    exe = os.path.join(d, "qbeta_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tools", "qbeta_check.cpp"), "-o", exe])
    return exe


def run_qbeta_check(exe, grid):
    inp = "".join("%.17g %.17g %.17g\n" % g for g in grid)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True)
    assert out.stderr == "", out.stderr
    return [float(s) for s in out.stdout.split()]


def mp_root(p, a, b, x0):
    """the root of I_x(a, b) = p at 40 digits by Newton steps from x0 (within 1e-12 of it).  mpmath's betainc sums a hypergeometric
    series that does not converge for shapes in the thousands and beyond; there the distribution function is the integral of the
    density over pieces of two standard deviations on the shorter side of x (the two agree to 1e-37 where both work)."""
    import mpmath as mp
    A, B, P = mp.mpf(a), mp.mpf(b), mp.mpf(p)
    c = mp.loggamma(A + B) - mp.loggamma(A) - mp.loggamma(B)
    f = lambda x: mp.exp((A - 1) * mp.log(x) + (B - 1) * mp.log(1 - x) + c)
    sd = mp.sqrt(A * B / ((A + B) ** 2 * (A + B + 1)))
    mode = (A - 1) / (A + B - 2)

    def cdf_quad(x):
        lower = x < mode
        pts = [x]
        while len(pts) < 40:
            nxt = pts[-1] - 2 * sd if lower else pts[-1] + 2 * sd
            if nxt <= 0 or nxt >= 1:
                break
            pts.append(nxt)
        pts.append(mp.mpf(0) if lower else mp.mpf(1))
        v = mp.quad(f, sorted(pts))
        return v if lower else 1 - v
    cdf = cdf_quad if max(a, b) > 500 else (lambda x: mp.betainc(A, B, 0, x, regularized=True))
    x = mp.mpf(x0)
    for _ in range(4):
        dx = (cdf(x) - P) / f(x)
        x -= dx
        if abs(dx) < mp.mpf(10) ** -25:
            return x, cdf_quad, (lambda x: mp.betainc(A, B, 0, x, regularized=True))
    raise AssertionError("no convergence from %r" % x0)


def test_qbeta_against_mpmath_at_40_digits():
    import mpmath as mp
    from scipy.special import betaincinv
    grid = qbeta_grid()
    assert min(min(a, b) for _, a, b in grid) == 1.05 and max(max(a, b) for _, a, b in grid) == QBETA_SMAX
    got = run_qbeta_check(build_qbeta_check(), grid)
    assert got == run_qbeta_check(build_qbeta_check(("-O0",)), grid)        # the same bits whatever the optimiser does
    worst = 0.0
    with mp.workdps(40):
        for (p, a, b), x in zip(grid, got):
            assert 0.0 < x < 1.0
            root, quad, inc = mp_root(p, a, b, x)
            worst = max(worst, float(abs(root - mp.mpf(x))))
            assert abs(x - betaincinv(a, b, p)) <= 1e-14                   # the cross-check
            if 500 < max(a, b) < 5000:                                     # the two forms of the reference agree where both work
                assert abs(quad(mp.mpf(x)) - inc(mp.mpf(x))) < mp.mpf(10) ** -30
    print("largest |qbeta - mpmath's root|: %.3g" % worst)
    assert worst <= QBETA_MEASURED, worst                  # the figure in the README is what is measured
    assert 4 * QBETA_MEASURED < 1e-6 / QBETA_SMAX            # the bound cannot move an index that is decided by 1e-6
    # outside its domain
    assert all(math.isnan(v) for v in run_qbeta_check(build_qbeta_check(), [(0.0, 2, 2), (1.0, 2, 2), (0.5, 1.0, 2), (0.5, 2, 0.5), (0.5, float("nan"), 2)]))


def test_qbeta_under_address_and_undefined_behaviour_sanitizers():
    """a host build of the stand-alone program, run here: the same bits, nothing reported"""
    grid = qbeta_grid()
    exe = build_qbeta_check(("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    assert run_qbeta_check(exe, grid) == run_qbeta_check(build_qbeta_check(), grid)


# ---- 4. the C ABI without a device ---------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    outs = [np.zeros(64) for _ in range(10)]
    tr = np.zeros(8, dtype=np.int32)
    fake = C.c_void_p(4096)            # never dereferenced: every case below is refused before the first device call
    ip = C.POINTER(C.c_int32)

    def call(ptr=fake, chains=4, iters=10, nvars=2, first=0, count=10, cols=None, ncols=None, probs=PROBS, nprobs=None, nlags=0, null=()):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        nc = (len(sel) if sel is not None else 0) if ncols is None else ncols
        pr = np.array(probs, dtype=np.float64) if probs is not None else None
        npr = (len(pr) if pr is not None else 0) if nprobs is None else nprobs
        o = [_capi.dptr(a) for a in outs] + [tr.ctypes.data_as(ip)]
        for j in null:
            o[j] = None
        return L.rh_mcse_device(ptr, 0, chains, iters, nvars, first, count, sel.ctypes.data_as(ip) if sel is not None else None, nc,
                                _capi.dptr(pr) if pr is not None and len(pr) else None, npr, nlags, *o)
    err = lambda: L.rh_last_error(None).decode()
    assert call(ptr=None) == _capi.RH_E_INVALID and "NULL" in err()
    assert call(probs=None, nprobs=2) == _capi.RH_E_INVALID and "NULL" in err()
    for first, count in ((0, 3), (0, 0), (0, 11), (7, 4), (-1, 5), (10, 4)):
        assert call(first=first, count=count) == _capi.RH_E_INVALID, (first, count)
        assert "window" in err() and "at least 4" in err()
    assert call(nvars=0) == _capi.RH_E_INVALID and call(chains=0) == _capi.RH_E_INVALID
    for cols in ([2], [-1], [0, 1, 7]):
        assert call(cols=cols) == _capi.RH_E_INVALID and "outside" in err(), cols
    assert call(cols=[0], ncols=0) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(cols=[0], ncols=-3) == _capi.RH_E_INVALID and "ncols" in err()
    assert call(ncols=1) == _capi.RH_E_INVALID and "ncols" in err()            # no list: 0 or nvars
    assert call(probs=tuple(np.linspace(0.1, 0.9, 17))) == _capi.RH_E_INVALID and "nprobs" in err()
    assert call(nprobs=-1) == _capi.RH_E_INVALID and "nprobs" in err()
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert call(probs=(0.5, bad)) == _capi.RH_E_INVALID and "(0, 1)" in err(), bad
    for nlags in (-1, 256):
        assert call(nlags=nlags) == _capi.RH_E_INVALID and "nlags" in err()
    assert L.rh_sampler_mcse(None, 0, 10, None, 0, None, 0, 0, *[_capi.dptr(a) for a in outs], tr.ctypes.data_as(ip)) == _capi.RH_E_INVALID
    # one column beyond the workspace cap: refused from the shape, whatever the machine
    assert call(chains=2183, iters=2048, count=2048, probs=None) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    assert call(chains=1055, iters=2048, count=2048, probs=tuple(np.linspace(0.03, 0.97, 16))) == _capi.RH_E_UNSUPPORTED and "workspace" in err()
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        assert call(null=range(11)) == _capi.RH_E_DEVICE                        # every output may be NULL
        assert call(ncols=2, probs=None, nlags=255) == _capi.RH_E_DEVICE and call(cols=[1, 1, 0]) == _capi.RH_E_DEVICE and call(chains=1, count=4) == _capi.RH_E_DEVICE
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.mcse_device(4096, 4, 10, 4)


# ---- 5. what the figures mean (sanity bands on fixed seeds, not precision claims) -------------------------------------------------------
def one(x, **kw):
    return emulate(np.ascontiguousarray(x[:, :, None]), **kw)


def test_ess_mean_of_iid_and_ar1_draws():
    S = 4000
    r = one(ar1(4, 1000, 0.0, 21))
    assert S / 2 <= r["ess_mean"][0] <= 2 * S and r["truncated"][0] == 0
    rho = 0.9
    r = one(ar1(4, 1000, rho, 22))
    want = (1 - rho) / (1 + rho)
    assert want / 2 <= r["ess_mean"][0] / S <= 2 * want


def test_mcse_mean_is_the_sd_of_the_mean_over_replications():
    rho = 0.7
    reps = [ar1(4, 1000, rho, 1000 + s) for s in range(200)]
    emp = float(np.std([v.mean() for v in reps], ddof=1))
    r = one(ar1(4, 1000, rho, 23))
    print(r["mcse_mean"][0], emp)
    assert emp / 2 <= r["mcse_mean"][0] <= 2 * emp
    # the quantiles' too: the median of the same replications
    med = float(np.std([np.median(v) for v in reps], ddof=1))
    assert med / 2 <= r["mcse_quantile"][0, 1] <= 2 * med


def test_cauchy_draws_have_a_median_with_a_standard_error_and_a_mean_without():
    """16 replications: the median's standard error keeps to a factor 2 among them (and near pi / 2 / sqrt(4000) = 0.025); the mean's is
    sd / sqrt(ess) with an sd that the largest draw makes, about 1 / U of a uniform U: among 16 of those the largest is typically 16
    times the smallest, and 4 is asked for"""
    rs = [one(np.random.default_rng(30 + s).standard_cauchy((4, 1000))) for s in range(16)]
    mq = np.array([r["mcse_quantile"][0, 1] for r in rs])
    mm = np.array([r["mcse_mean"][0] for r in rs])
    print(mq, mm)
    assert np.all(np.isfinite(mq)) and mq.max() / mq.min() < 2.0 and np.all(mq < 0.05)
    assert np.all(np.isfinite(mm)) and mm.max() / mm.min() > 4.0
