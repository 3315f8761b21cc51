"""Posterior-predictive sampling over device-resident draws (csrc/device/rh_generate.hip.h: Trace.predict of a Distribution,
core/Trace.scala:34-41, core/Generator.scala:171-174), the part that needs no GPU:

  * the kernel cross-compiles for gfx950 through the engine's own path (kernel cache, kernel_health, isacheck), spills nothing and
    uses no scratch;
  * THE ORACLE: a Python restatement of the reference's generators, written here from core/Continuous.scala:54-215 and
    core/Discrete.scala:38-186, on the oracle's java.util.Random (oracle/jmath.c jrandom_*) seeded per draw by the splitmix64 mix and
    with the oracle's fdlibm (jm_strict_log / jm_strict_exp: the JM_DET policy) -- it counts the passes of every loop;
  * the very text of the block routine, compiled with the host g++ (contraction off, the prelude's own rng text around it), every
    "thread" of a phase run in turn, walked over whole buffers as draws_plan.hpp says and compared with the oracle bit for bit (NaN
    matches NaN, -0.0 is not +0.0): every family with column and immediate arguments, both branches of Gamma and Poisson, the
    shapes the GPU tests use;
  * the domain guards and the iteration cap (on the CPU only), independence of shape / sharding / seed, the quality of the per-draw
    streams, and the C ABI's argument errors.

tests/test_gpu_generate_device.py runs the same fixtures through the kernel and asks for the oracle's and the emulation's bits.
"""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, gen
from tests import oracle_lib as O
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")
KERNEL = "rh_generate_kernel"
TILE, SLAB = 256, 31                     # RG_TILE, RG_SLAB (checked against the header below)
F_DOMAIN, F_CAP = _capi.GEN_F_DOMAIN, _capi.GEN_F_CAP
SEED = 20240607

# one row, a wavefront, one short of a tile, a tile, one over, two tiles and a ragged third
SHAPES = [(1, 1), (1, 64), (3, 85), (1, 256), (1, 257), (4, 129)]
NOUTS = [1, 7, SLAB + 1]                 # one op, a few, one more than a slab holds
NIN = 6
BELOW_30 = float(np.nextafter(30.0, 0.0))
GAMMA_SHAPES = [0.3, 1.0, 1.3, 50.0]
POISSON_LAMBDAS = [0.0, 0.5, BELOW_30, 30.0, 1000.0]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def inputs(chains, kept, seed=None):
    """per-draw parameters [chains][kept][NIN], every one in its domain: loc, scale, a Gamma shape, a Poisson lambda (both branches of
    each), a probability, a second shape"""
    rng = np.random.default_rng(7000 * chains + kept if seed is None else seed)
    n = chains * kept
    x = np.empty((n, NIN))
    x[:, 0] = rng.normal(size=n)
    x[:, 1] = np.abs(rng.normal(size=n)) + 0.1
    x[:, 2] = rng.choice(GAMMA_SHAPES, size=n)
    x[:, 3] = rng.choice(POISSON_LAMBDAS, size=n)
    x[:, 4] = rng.uniform(0.05, 0.95, size=n)
    x[:, 5] = rng.uniform(0.2, 3.0, size=n)
    return x.reshape(chains, kept, NIN)


c = gen.col
ALL_OPS = [   # every family with column and with immediate arguments; Gamma and Poisson on both branches
    gen.Real(c(0)), gen.Real(2.5), gen.Normal(c(0), c(1)), gen.Normal(1.0, 2.0), gen.Cauchy(c(0), c(1)), gen.Cauchy(0.0, 1.0),
    gen.Laplace(c(0), c(1)), gen.Laplace(-1.0, 0.5), gen.Uniform(c(0), c(1)), gen.Uniform(2.0, 5.0), gen.LogNormal(c(0), c(1)),
    gen.LogNormal(0.5, 0.25), gen.Gamma(c(2), c(1)), gen.Gamma(0.3, 2.0), gen.Gamma(50.0, 1.0), gen.Exponential(2.0),
    gen.Beta(c(2), c(5)), gen.Beta(0.5, 0.5), gen.Bernoulli(c(4)), gen.Bernoulli(0.3), gen.Geometric(c(4)), gen.Geometric(0.2),
    gen.Poisson(c(3)), gen.Poisson(0.5), gen.Poisson(1000.0), gen.Poisson(30.0), gen.Poisson(BELOW_30), gen.Poisson(0.0),
    gen.Normal(c(0), 1.0), gen.Gamma(1.3, c(1)), gen.Laplace(c(0), 1.0), gen.Cauchy(c(0), c(1)),
]
assert len(ALL_OPS) == SLAB + 1
FEW_OPS = [gen.Normal(c(0), c(1)), gen.Gamma(c(2), c(1)), gen.Poisson(c(3)), gen.Cauchy(c(0), c(1)), gen.Beta(c(2), c(5)),
           gen.Geometric(c(4)), gen.LogNormal(c(0), c(1))]   # (an odd number of gaussians ahead of Cauchy: the pending one is carried)


def table(nout):
    return {1: [gen.Normal(c(0), c(1))], 7: FEW_OPS, SLAB + 1: ALL_OPS}[nout]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """bit for bit; NaN matches NaN, -0.0 is not +0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
NAN = float("nan")


def draw_seed(seed, d):
    """splitmix64's finaliser of seed + (d + 1) * golden, as a signed 64-bit seed of java.util.Random"""
    z = (seed + (d + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z - (1 << 64) if z >> 63 else z


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x


def _d2l(x):   # Java's d2l
    if x != x:
        return 0
    if x >= 2.0 ** 63:
        return (1 << 63) - 1
    if x <= -2.0 ** 63:
        return -(1 << 63)
    return int(x)


class Passes:
    """the most passes each loop needed, and which branches ran"""
    def __init__(self):
        self.most = {"gamma_outer": 0, "gamma_inner": 0, "poisson_small": 0, "poisson_large": 0}
        self.branches = set()

    def see(self, loop, n):
        self.most[loop] = max(self.most[loop], n)


class Stream:
    """ScalaRNG over the oracle's java.util.Random, the JM_DET math next to it"""
    def __init__(self, seed):
        self.r = O.JavaRandom(seed)
        self.log, self.exp = self.r.lib.jm_strict_log, self.r.lib.jm_strict_exp
        self.uniform, self.normal = self.r.next_double, self.r.next_gaussian


def _gamma_standard(s, a, ps):
    """Gamma.standard(a).generator (Continuous.scala:114-144); Math.pow(u, 1 / a) by the JM_DET composition exp((1 / a) * log(u))"""
    boost = None
    if a < 1:
        u = s.uniform()
        boost = s.exp((1.0 / a) * s.log(u))
        ps.branches.add("gamma_boost")
        a = a + 1
    else:
        ps.branches.add("gamma_plain")
    d = a - 1.0 / 3.0
    cc = (1.0 / 3.0) / math.sqrt(d)
    outer = 0
    while True:
        outer += 1
        inner = 1
        x = s.normal()
        v = 1.0 + cc * x
        while v <= 0:
            inner += 1
            x = s.normal()
            v = 1.0 + cc * x
        ps.see("gamma_inner", inner)
        v3 = v * v * v
        u = s.uniform()
        if (u < 1 - 0.0331 * x * x * x * x) or (s.log(u) < 0.5 * x * x + d * (1 - v3 + s.log(v3))):
            ps.see("gamma_outer", outer)
            g = d * v3
            return g if boost is None else g * boost


def _poisson(s, lam, ps):
    """Poisson.generator (Discrete.scala:128-186); math.pow(t, 2) is t * t"""
    if lam < 30.0:
        ps.branches.add("poisson_small")
        l = s.exp(-lam)
        if l >= 1.0:
            return 0.0
        k, p = 0, 1.0
        while p > l:
            k += 1
            p *= s.uniform()
        ps.see("poisson_small", k)
        return float(k - 1)
    ps.branches.add("poisson_large")
    cc = 0.767 - 3.36 / lam
    beta = math.pi / math.sqrt(3.0 * lam)
    alpha = beta * lam
    k = s.log(cc) - lam - s.log(beta)
    passes = 0
    while True:
        passes += 1
        u = s.uniform()
        x = _div(alpha - s.log(_div(1.0 - u, u)), beta)
        n = _d2l(_floor(x + 0.5))
        if n >= 0:
            v = s.uniform()
            y = alpha - beta * x
            t = 1.0 + s.exp(y)
            lhs = y + s.log(_div(v, t * t))
            xf = float(n + 1)
            logfact = ((xf - 0.5) * s.log(xf)) - xf + (0.5 * s.log(2 * math.pi))
            rhs = k + float(n) * s.log(lam) - logfact
            if lhs <= rhs:
                ps.see("poisson_large", passes)
                return float(n)


def _finite_pos(x):
    return math.isfinite(x) and x > 0


def oracle_op(s, op, row, ps):
    """Generator.get of one op on the draw's stream -> (value, flag)"""
    a = row[op.a.col] if op.a.col >= 0 else op.a.value
    b = row[op.b.col] if op.b.col >= 0 else op.b.value
    a, b, f = float(a), float(b), op.family
    if f == _capi.GEN_REAL:
        return a, 0
    if f == _capi.GEN_NORMAL:
        return s.normal() * b + a, 0
    if f == _capi.GEN_CAUCHY:
        g1 = s.normal()
        g2 = s.normal()
        return _div(g1, g2) * b + a, 0
    if f == _capi.GEN_LAPLACE:
        u = s.uniform() - 0.5
        sg = 1.0 if u > 0 else (-1.0 if u < 0 else u)
        return (sg * -1.0 * s.log(1 - (2 * abs(u)))) * b + a, 0
    if f == _capi.GEN_UNIFORM:
        return s.uniform() * b + a, 0
    if f == _capi.GEN_LOGNORMAL:
        return s.exp(s.normal() * b + a), 0
    if f == _capi.GEN_GAMMA:
        if not _finite_pos(a):
            return NAN, F_DOMAIN
        return _gamma_standard(s, a, ps) * b, 0
    if f == _capi.GEN_BETA:
        if not (_finite_pos(a) and _finite_pos(b)):
            return NAN, F_DOMAIN
        z1 = _gamma_standard(s, a, ps) * 1.0
        z2 = _gamma_standard(s, b, ps) * 1.0
        return _div(z1, z1 + z2), 0
    if f == _capi.GEN_BERNOULLI:
        return (1.0 if s.uniform() <= a else 0.0), 0
    if f == _capi.GEN_GEOMETRIC:
        return float(_d2l(_floor(_div(s.log(s.uniform()), s.log(1 - a))))), 0
    if f == _capi.GEN_POISSON:
        if not (math.isfinite(a) and a >= 0):
            return NAN, F_DOMAIN
        return _poisson(s, a, ps), 0
    raise AssertionError(f)


def oracle(x, ops, seed, chain0=0, passes=None):
    """x [chains][kept][nin] -> (samples [chains][kept][nops], flags): every draw on ScalaRNG(draw_seed(seed, chain0 * kept + r))"""
    x = np.asarray(x, dtype=np.float64)
    chains, kept, nin = x.shape
    flat = x.reshape(-1, nin)
    ps = passes if passes is not None else Passes()
    out, flags = np.empty((flat.shape[0], len(ops))), 0
    with np.errstate(all="ignore"):
        for r, row in enumerate(flat):
            s = Stream(draw_seed(seed, (chain0 * kept + r) & M64))
            for o, op in enumerate(ops):
                out[r, o], fl = oracle_op(s, op, row, ps)
                flags |= fl
    return out.reshape(chains, kept, len(ops)), flags


@functools.lru_cache(maxsize=None)
def reference(chains, kept, nout):
    """the oracle over the fixture of one shape, computed once: (x, samples, flags, passes); the arrays are read-only"""
    x, ps = inputs(chains, kept), Passes()
    want, flags = oracle(x, table(nout), SEED, passes=ps)
    x.setflags(write=False); want.setflags(write=False)
    return x, want, flags, ps


# ---- the device text on the host ---------------------------------------------------------------------------------------------------
_PREAMBLE = r'''
#include <cmath>
#include <cstddef>
#include <vector>
typedef unsigned long long rh_u64;
typedef long long rh_i64;
#define RH_DEV static inline
// strict math: the oracle's fdlibm (oracle/jmath.c), which the device's rh_strict_exp / rh_strict_log are bit-compared with on the GPU
extern "C" double jm_strict_exp(double);
extern "C" double jm_strict_log(double);
static inline double rh_strict_exp(double x) { return jm_strict_exp(x); }
static inline double rh_strict_log(double x) { return jm_strict_log(x); }
static inline double rh_strict_sqrt(double x) { return __builtin_sqrt(x); }
'''
_DRIVER = r'''
#define RH_GENERATE_HOST 1
#include "draws_plan.hpp"
// the launch of generate_enqueue (csrc/draws.cpp) and the kernel's index arithmetic, one workgroup after the other
extern "C" int rg_emulate(const double *in, int nin, const rg_op *ops, int nops, long long nrows, long long seed, long long row0_global, double *out) {
  std::vector<double> lds(rh_plan::generate_lds_bytes(nops) / sizeof(double));
  int flags = 0;
  const long long tiles = rh_plan::generate_tiles(nrows);
  for (long long t = 0; t < tiles; t++) {
    const long long r0 = t * RG_TILE;
    const int valid = nrows - r0 < RG_TILE ? (int)(nrows - r0) : RG_TILE;
    rg_block(in + r0 * nin, nin, ops, nops, valid, seed, (rh_u64)row0_global + (rh_u64)r0, lds.data(), out + r0 * nops, &flags, RG_TILE);
  }
  return flags;
}
extern "C" int rg_const(int i) { const int v[] = {RG_TILE, RG_SLAB, RG_MAX_ATTEMPTS, RG_MAX_OPS, (int)sizeof(rg_op), rh_plan::generate_slabs(RG_SLAB + 1), (int)rh_plan::generate_lds_bytes(RG_MAX_OPS)}; return v[i]; }
'''
_emu = {}


def prelude_rng_text():
    """the prelude's java.util.Random, as it stands: the text the kernel is compiled with"""
    src = open(os.path.join(CSRC, "device", "rh_prelude.hip.h")).read()
    return src[src.index("struct rh_rng {"):src.index("RH_DEV int rh_rng_int(")]


def emulation(max_attempts=None):
    """preamble + the prelude's rng + draws_plan.hpp (which brings rh_generate.hip.h in host mode) + the driver -> a host shared library
    (g++ -O2 -ffp-contract=off: every a*b+c stays two roundings, as hiprtc is told for the device)"""
    if max_attempts not in _emu:
        import tempfile
        O.load()                                                    # (builds oracle/liboracle.so when it is not there)
        d = tempfile.mkdtemp(prefix="rh_generate_emu")
        cpp, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(cpp, "w").write(_PREAMBLE + prelude_rng_text() + _DRIVER)
        odir = os.path.join(ROOT, "oracle")
        flags = ["-DRG_MAX_ATTEMPTS=%d" % max_attempts] if max_attempts else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function"] + flags +
                              ["-I", CSRC, "-shared", "-fPIC", cpp, "-o", so, "-L", odir, "-loracle", "-Wl,-rpath," + odir])
        L = C.CDLL(so)
        L.rg_emulate.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(_capi.GenOp), C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_double)]
        _emu[max_attempts] = L
    return _emu[max_attempts]


def emulate(x, ops, seed, chain0=0, max_attempts=None):
    """the host emulation over x [chains][kept][nin] -> (samples [chains][kept][nops], flags)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    chains, kept, nin = x.shape
    arr = (_capi.GenOp * len(ops))(*ops)
    out = np.full((chains, kept, len(ops)), -7.0)
    flags = emulation(max_attempts).rg_emulate(_capi.dptr(x), nin, arr, len(ops), chains * kept, seed, chain0 * kept, _capi.dptr(out))
    return out, flags


# ---- 1. the code object ------------------------------------------------------------------------------------------------------------
def test_generate_kernel_cross_compiles_without_spills_or_scratch():
    code = _capi.generate_lower_only()
    rep = _capi.code_object_report(code)
    assert sorted(k for _, k in rep) == [KERNEL]
    assert _kernel_meta(code, KERNEL, ".vgpr_spill_count") == 0 and _kernel_meta(code, KERNEL, ".sgpr_spill_count") == 0
    assert _kernel_meta(code, KERNEL, ".private_segment_fixed_size") == 0
    r = rep[("object", KERNEL)]
    assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r             # kernel_health: metadata + isacheck's walk
    before = _capi.lib().rh_compile_count()
    assert _capi.generate_lower_only() == code and _capi.lib().rh_compile_count() == before   # served by the kernel cache


def test_plan_constants_are_the_headers():
    L = emulation()
    assert [L.rg_const(i) for i in range(5)] == [TILE, SLAB, 4096, 4096, C.sizeof(_capi.GenOp)]
    assert L.rg_const(5) == 2 and L.rg_const(6) == 8 * TILE * SLAB <= 63 * 1024    # one op over a slab: two slabs; the odd stride 31
    hdr = open(os.path.join(CSRC, "device", "rh_generate.hip.h")).read()
    assert int(re.search(r"#define RG_MAX_ATTEMPTS (\d+)", hdr).group(1)) == 4096


# ---- 2. the host emulation against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,kept", SHAPES)
def test_host_emulation_has_the_oracles_bits(chains, kept):
    for nout in NOUTS:
        x, want, flags, ps = reference(chains, kept, nout)
        got, got_flags = emulate(x, table(nout), SEED)
        assert same_bits(got, want), (chains, kept, nout, np.argwhere(bits(got) != bits(want))[:4])
        assert flags == 0 and got_flags == 0                       # every parameter is in its domain, no loop comes near the cap
        assert max(ps.most.values()) <= 64, ps.most


def test_both_branches_of_gamma_and_poisson():
    ops = [gen.Gamma(a, 1.5) for a in GAMMA_SHAPES] + [gen.Poisson(l) for l in POISSON_LAMBDAS] + [gen.Gamma(c(2), 1.0), gen.Poisson(c(3))]
    x, ps = inputs(2, 150, seed=11), Passes()
    want, flags = oracle(x, ops, SEED + 1, passes=ps)
    got, got_flags = emulate(x, ops, SEED + 1)
    assert same_bits(got, want) and flags == 0 and got_flags == 0
    assert ps.branches == {"gamma_boost", "gamma_plain", "poisson_small", "poisson_large"}
    assert max(ps.most.values()) <= 64 and ps.most["gamma_outer"] >= 2 and ps.most["poisson_large"] >= 2, ps.most   # the retries ran
    assert np.all(want[..., 4] == 0.0)                             # Poisson(0): exp(-0.0) >= 1
    assert np.all(want[..., :4] > 0) and np.all(want[..., 4:9] >= 0) and np.all(want[..., 4:9] == np.floor(want[..., 4:9]))
    # the samplers sample what they say: means within five standard errors over the 300 draws
    for k, a in enumerate(GAMMA_SHAPES):
        assert abs(want[..., k].mean() - 1.5 * a) < 5 * 1.5 * math.sqrt(a / 300)
    for k, l in enumerate(POISSON_LAMBDAS[1:], 5):
        assert abs(want[..., k].mean() - l) < 5 * math.sqrt(l / 300) + 0.51   # (Poisson.large rounds x + 0.5: half a count of slack)


# ---- 3. the edges, on the CPU only -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,bad", [("gamma", [NAN, math.inf, -math.inf, 0.0, -0.0, -1.5]), ("beta_a", [NAN, math.inf, 0.0, -2.0]),
                                        ("beta_b", [NAN, -math.inf, 0.0, -0.1]), ("poisson", [NAN, math.inf, -math.inf, -1.0, -1e-300])])
def test_domain_guards_give_nan_and_leave_the_stream_untouched(family, bad):
    guarded = {"gamma": gen.Gamma(c(0), 2.0), "beta_a": gen.Beta(c(0), 1.5), "beta_b": gen.Beta(1.5, c(0)), "poisson": gen.Poisson(c(0))}[family]
    before, after = [gen.Normal(0.0, 1.0), gen.Poisson(4.0)], [gen.Normal(1.0, 2.0), gen.Gamma(0.7, 1.0), gen.Uniform(0.0, 1.0)]
    x = np.array(bad + [1.25]).reshape(1, -1, 1)                   # the last draw is in the domain
    got, flags = emulate(x, before + [guarded] + after, SEED)
    want, want_flags = oracle(x, before + [guarded] + after, SEED)
    assert same_bits(got, want) and flags == want_flags == F_DOMAIN
    assert np.all(np.isnan(got[0, :-1, 2])) and not np.isnan(got[0, -1, 2])
    # the draw's other ops: a run of the table without the guarded op (which then used nothing of the stream)
    rest, rest_flags = emulate(x, before + after, SEED)
    assert rest_flags == 0 and same_bits(got[0, :-1][:, [0, 1, 3, 4, 5]], rest[0, :-1])
    assert not same_bits(got[0, -1, 3:], rest[0, -1, 2:])          # ... and the op in its domain did use it


def test_iteration_cap_gives_nan_and_the_flag():
    for op, loop in ((gen.Poisson(2.0), "poisson_small"), (gen.Poisson(30.0), "poisson_large"), (gen.Gamma(1.0, 1.0), "gamma_outer")):
        x = np.zeros((1, 1500, 1))
        needed = []
        for r in range(x.shape[1]):                                # the passes every draw needs, by the oracle
            ps = Passes()
            oracle(x[:, r:r + 1], [op], SEED, chain0=r, passes=ps)
            needed.append(max(ps.most[loop], ps.most["gamma_inner"]))   # (Marsaglia-Tsang's two loops share the cap)
        needed = np.array(needed)
        assert (needed == 3).any() and (needed <= 2).any(), (loop, np.bincount(needed))
        want, _ = oracle(x, [op], SEED)
        full, full_flags = emulate(x, [op], SEED)
        assert same_bits(full, want) and full_flags == 0
        got, flags = emulate(x, [op], SEED, max_attempts=2)        # the same text built with RG_MAX_ATTEMPTS = 2
        assert flags == F_CAP, loop
        assert np.all(np.isnan(got[0, needed >= 3, 0])) and same_bits(got[0, needed <= 2], want[0, needed <= 2]), loop


# ---- 4. independence of shape, sharding and seed -----------------------------------------------------------------------------------
def test_results_do_not_depend_on_shape_or_sharding():
    ops = FEW_OPS
    x = inputs(3, 86, seed=5)
    whole, _ = emulate(x, ops, SEED)
    flat, _ = emulate(x.reshape(1, 258, NIN), ops, SEED)
    assert same_bits(whole.reshape(-1), flat.reshape(-1))
    y = inputs(4, 86, seed=6)
    run, _ = emulate(y, ops, SEED)
    shard, _ = emulate(y[2:], ops, SEED, chain0=2)                 # chains 2..3 of the run, as another device would hold them
    assert same_bits(shard, run[2:]) and same_bits(oracle(y[2:], ops, SEED, chain0=2)[0], run[2:])
    again, _ = emulate(y, ops, SEED)
    other, _ = emulate(y, ops, SEED + 1)
    assert same_bits(again, run) and not np.any(bits(other[..., 0]) == bits(run[..., 0]))


# ---- 5. the quality of the per-draw streams ----------------------------------------------------------------------------------------
def test_consecutive_draws_have_uncorrelated_streams():
    n = 20000
    first_u, first_g = np.empty(n), np.empty(n)
    for d in range(n):
        first_u[d] = O.JavaRandom(draw_seed(SEED, d)).next_double()
        first_g[d] = O.JavaRandom(draw_seed(SEED, d)).next_gaussian()

    def lag1_z(v):
        w = v - v.mean()
        return abs(float((w[1:] * w[:-1]).sum() / (w * w).sum())) * math.sqrt(n)
    # five standard errors each (the mix measures below 1.1 on all six; seed + d gives a lag-1 z of 140 for the uniforms)
    assert lag1_z(first_u) < 5 and lag1_z(first_g) < 5
    assert abs(first_u.mean() - 0.5) / math.sqrt(1 / 12 / n) < 5 and abs(first_g.mean()) / math.sqrt(1 / n) < 5
    assert abs(first_u.var() - 1 / 12) / math.sqrt((1 / 80 - 1 / 144) / n) < 5 and abs(first_g.var() - 1) / math.sqrt(2 / n) < 5
    naive = np.array([O.JavaRandom(SEED + d).next_double() for d in range(2000)])
    w = naive - naive.mean()
    assert abs(float((w[1:] * w[:-1]).sum() / (w * w).sum())) * math.sqrt(2000) > 5    # why the seeds are mixed


# ---- 6. the C ABI's argument errors and the Python surface -------------------------------------------------------------------------
def test_argument_errors_before_any_device_call():
    L = _capi.lib()
    err = lambda: L.rh_last_error(None).decode()
    h = C.c_void_p()

    def create(ops, nin=2, nops=None):
        arr = (_capi.GenOp * max(1, len(ops)))(*ops)
        return L.rh_generate_create(arr, len(ops) if nops is None else nops, nin, -1, C.byref(h))
    raw = lambda f, a, b: _capi.GenOp(f, 0, _capi.GenArg(*a), _capi.GenArg(*b))
    assert create([]) == _capi.RH_E_INVALID and "1 .. 4096" in err() and not h
    assert create([gen.Real(1.0)], nops=4097) == _capi.RH_E_INVALID and not h
    assert create([gen.Real(1.0)], nin=-1) == _capi.RH_E_INVALID and not h
    assert create([gen.Real(1.0), raw(11, (-1, 0, 0.0), (-1, 0, 0.0))]) == _capi.RH_E_INVALID and "op 1: unknown family 11" in err()
    assert create([raw(-1, (-1, 0, 0.0), (-1, 0, 0.0))]) == _capi.RH_E_INVALID and "op 0" in err()
    assert create([gen.Normal(c(0), c(2))]) == _capi.RH_E_INVALID and "op 0 (NORMAL): column 2" in err()
    assert create([gen.Normal(0.0, 1.0), raw(_capi.GEN_GAMMA, (-2, 0, 0.0), (-1, 0, 1.0))]) == _capi.RH_E_INVALID and "op 1 (GAMMA): column -2" in err()
    for f, name in ((_capi.GEN_REAL, "REAL"), (_capi.GEN_BERNOULLI, "BERNOULLI"), (_capi.GEN_GEOMETRIC, "GEOMETRIC"), (_capi.GEN_POISSON, "POISSON")):
        assert create([raw(f, (0, 0, 0.0), (1, 0, 0.0))]) == _capi.RH_E_INVALID and "op 0 (%s)" % name in err() and "one argument" in err()
        assert create([raw(f, (0, 0, 0.0), (-1, 0, 0.5))]) == _capi.RH_E_INVALID and not h
    assert L.rh_generate_create(None, 1, 0, -1, C.byref(h)) == _capi.RH_E_INVALID
    assert L.rh_generate_nout(None) == -1
    L.rh_generate_destroy(None)
    # a handle needs no device; a call does
    assert create([gen.Normal(c(0), c(1)), gen.Poisson(3.0)]) == _capi.RH_OK and h and L.rh_generate_nout(h) == 2
    out, fake = np.zeros(8), C.c_void_p(4096)                      # never dereferenced: refused before the first device call
    assert L.rh_generate_device(None, fake, 0, 1, 4, 2, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID
    assert L.rh_generate_device(h, None, 0, 1, 4, 2, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID
    assert L.rh_generate_device(h, fake, 0, 1, 4, 3, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID and "3 columns, the generator reads 2" in err()
    assert L.rh_generate_device(h, fake, 0, 0, 4, 2, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID
    assert L.rh_generate_device(h, fake, 0, 1, 0, 2, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID
    assert L.rh_sampler_generate(None, None, h, 0, 10, 1, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_INVALID
    if L.rh_device_count() == 0:
        assert L.rh_generate_device(h, fake, 0, 1, 4, 2, 1, 0, _capi.dptr(out), None, None) == _capi.RH_E_DEVICE and "no CPU fallback" in err()
        g = R.Generator([gen.Normal(c(0), c(1))], nin=2)
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.generate_device(g, 4096, 1, 4, 2, seed=1)
        g.close()
    L.rh_generate_destroy(h)


def test_python_op_constructors():
    u, e = gen.Uniform(1.0, 3.5), gen.Exponential(4.0)
    assert (u.family, u.a.col, u.a.value, u.b.col, u.b.value) == (_capi.GEN_UNIFORM, -1, 1.0, -1, 2.5)          # scale = to - from
    assert (e.family, e.a.value, e.b.value) == (_capi.GEN_GAMMA, 1.0, 0.25)                                     # Gamma.standard(1.0).scale(1 / rate)
    uc, ec = gen.Uniform(c(0), c(1)), gen.Exponential(c(3))
    assert (uc.a.col, uc.b.col) == (0, 1) and (ec.a.value, ec.b.col) == (1.0, 3)                                # columns: the caller's scale
    n = gen.Normal(c(2), 0.5)
    assert (n.family, n.a.col, n.b.col, n.b.value) == (_capi.GEN_NORMAL, 2, -1, 0.5)
    p = gen.Poisson(c(1))
    assert (p.family, p.a.col, p.b.col, p.b.value) == (_capi.GEN_POISSON, 1, -1, 0.0)
    g = R.Generator([n, p, e], nin=3)
    assert (g.nin, g.nout, g.flags) == (3, 3, 0)
    g.close()
    with pytest.raises(R.RainierHipError, match=r"op 1 \(NORMAL\): column 3"):
        R.Generator([p, gen.Normal(c(3), 1.0)], nin=3)
