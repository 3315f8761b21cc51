"""The count families and the composites of posterior-predictive sampling (csrc/device/rh_generate_ext.hip.h: Binomial,
NegativeBinomial, Categorical as families; BetaBinomial, mixtures and zero inflation as tables of hidden, guarded and carry-reading
ops), the part that needs no GPU:

  * THE ORACLE: tests/test_generate_device_cpu.py's (its java.util.Random stream, fdlibm, d2l and the eleven old families, imported),
    with the new families written here from core/Discrete.scala:81-109, 194-273, core/Multinomial.scala:26-29 and
    core/Generator.scala:49-57, 129-141, and the table's semantics -- guard, selector, carry, hidden -- from include/rainier_hip.h;
  * the very text of the block routine compiled with the host g++ (contraction off), walked as draws_plan.hpp says and compared with
    the oracle bit for bit: every branch at exactly representable parameters, the composites, a table of RG_SLAB + 1 visible columns
    whose slab boundary has a hidden op before it, a carry read across it and a guarded run around it;
  * the domain guards and the cap, what a skipped op leaves of the stream, independence of shape and sharding, an old table through
    the new kernel, the exact paths' laws, the code object, rh_generate_create's refusals and the Python constructors.

tests/test_gpu_generate_families.py runs the same fixtures through the kernel.
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import rainier_amd as R
from rainier_amd import _capi, gen
from tests import oracle_lib as O
from tests.test_capi_cpu import _kernel_meta
from tests.test_generate_device_cpu import (_PREAMBLE, CSRC, F_CAP, F_DOMAIN, FEW_OPS, M64, NAN, ROOT, SEED, SLAB, Passes, Stream, _d2l, _div, _floor,
                                            _poisson, bits, draw_seed, oracle_op, prelude_rng_text, same_bits)
from tests.test_generate_device_cpu import NIN as OLD_NIN, emulate as emulate_old, inputs as old_inputs

KERNEL = "rh_generate_ext_kernel"
HIDDEN, PREV = _capi.GEN_OP_HIDDEN, gen.PREV
MAX_TRIALS = 4096                        # RG_MAX_ATTEMPTS (checked against the header by tests/test_generate_device_cpu.py)
SHAPES = [(1, 1), (1, 64), (3, 85), (1, 257), (4, 129)]
c = gen.col


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
class PassesX(Passes):
    def __init__(self):
        super().__init__()
        self.most.update({"binomial_exact": 0, "negbin_exact": 0})


def _finite(x):
    return math.isfinite(x)


def _binomial(s, p, k, ps):
    """Binomial.generator (Discrete.scala:203-229); the exact path is Multinomial(Map(true -> p, false -> 1 - p), k).generator:
    categorical(pmf).repeat(k), n.toInt(k) draws (Generator.scala:49-57), true where cdf(true) = p + 0.0 >= u (:129-141)"""
    if not (_finite(p) and 0 <= p <= 1 and _finite(k) and k >= 0):
        return NAN, F_DOMAIN
    if k >= 100 and k * p <= 10:
        ps.branches.add("binomial_poisson")
        x = _poisson(s, p * k, ps)
        return float(min(_d2l(x), _d2l(k))), 0
    if k >= 100 and k * p >= 9 and k * (1.0 - p) >= 9:
        ps.branches.add("binomial_normal")
        x = s.normal() * math.sqrt(k * p * (1 - p)) + k * p
        return float(min(max(_d2l(x), 0), _d2l(k))), 0
    n = min(_d2l(k), 2 ** 31 - 1)                                   # d2i
    if n > MAX_TRIALS:
        return NAN, F_CAP
    ps.branches.add("binomial_exact")
    ps.see("binomial_exact", n)
    return float(sum(1 for _ in range(n) if p + 0.0 >= s.uniform())), 0


def _negbinomial(s, p, n, ps):
    """NegativeBinomial.generator (Discrete.scala:87-108): (1L to n.toLong).map(_ => Geometric(1 - p).generator.get).sum"""
    if not (_finite(p) and 0 <= p <= 1 and _finite(n) and n >= 0):
        return NAN, F_DOMAIN
    if p < _div(-100.0, n) + 1 and p > _div(100.0, n) - .25:
        ps.branches.add("negbin_normal")
        x = s.normal() * _div(math.sqrt(n * p), 1 - p) + _div(n * p, 1 - p)
        return float(max(_d2l(x), 0)), 0
    trials = _d2l(n)
    if trials > MAX_TRIALS:
        return NAN, F_CAP
    ps.branches.add("negbin_exact")
    ps.see("negbin_exact", trials)
    total = 0
    for _ in range(trials):
        u = s.uniform()
        total = (total + _d2l(_floor(_div(s.log(u), s.log(1 - (1 - p)))))) & M64   # the JVM's long sum wraps
    return float(total - (1 << 64) if total >> 63 else total), 0


def _categorical(s, w):
    """Generator.categorical (Generator.scala:129-141): cdf by scanLeft p + acc from 0, find cdf >= v, else the last"""
    if not all(_finite(x) and x >= 0 for x in w):
        return NAN, F_DOMAIN
    v, acc = s.uniform(), 0.0
    for i, x in enumerate(w):
        acc = x + acc
        if acc >= v:
            return float(i), 0
    return float(len(w) - 1), 0


def oracle_op_x(s, op, row, carry, ps):
    """one op that runs -> (value, flag): the arguments resolved (a column, an immediate, the carry), then the family"""
    arg = lambda a: carry if a.pad == _capi.GEN_ARG_PREV else (row[a.col] if a.col >= 0 else a.value)
    f = op.family
    if f == _capi.GEN_CATEGORICAL:
        return _categorical(s, [float(x) for x in row[op.a.col:op.a.col + int(op.b.value)]])
    a, b = float(arg(op.a)), float(arg(op.b))
    if f == _capi.GEN_BINOMIAL:
        return _binomial(s, a, b, ps)
    if f == _capi.GEN_NEGBINOMIAL:
        return _negbinomial(s, a, b, ps)
    return oracle_op(s, _capi.GenOp(f, 0, _capi.GenArg(-1, 0, a), _capi.GenArg(-1, 0, b)), row, ps)


def flat_ops(ops):
    return [op for entry in ops for op in (entry if isinstance(entry, (list, tuple)) else [entry])]


def visible(ops):
    return [o for o, op in enumerate(ops) if not op.reserved & HIDDEN]


def oracle(x, ops, seed, chain0=0, passes=None, all_ops=False):
    """x [chains][kept][nin] -> (samples [chains][kept][visible ops], flags).  A draw's ops run left to right on its stream; an op whose
    guard j + 1 does not meet the selector (the sample of the nearest earlier CATEGORICAL that ran) is skipped: nothing drawn, its
    value the carry.  all_ops: a column for every op, hidden ones too."""
    ops = flat_ops(ops)
    x = np.asarray(x, dtype=np.float64)
    chains, kept, nin = x.shape
    flat = x.reshape(-1, nin)
    ps = passes if passes is not None else PassesX()
    cols = list(range(len(ops))) if all_ops else visible(ops)
    out, flags = np.empty((flat.shape[0], len(ops))), 0
    with np.errstate(all="ignore"):
        for r, row in enumerate(flat):
            s = Stream(draw_seed(seed, (chain0 * kept + r) & M64))
            carry, sel = 0.0, None
            for o, op in enumerate(ops):
                guard = op.reserved & 0xff
                if not guard or sel == guard - 1:
                    carry, fl = oracle_op_x(s, op, row, carry, ps)
                    flags |= fl
                    if op.family == _capi.GEN_CATEGORICAL:
                        sel = None if carry != carry else int(carry)
                out[r, o] = carry
    return out[:, cols].reshape(chains, kept, len(cols)), flags


# ---- the device text on the host ---------------------------------------------------------------------------------------------------
_DRIVER = r'''
#define RH_GENERATE_HOST 1
#include "draws_plan.hpp"
// the launch of generate_enqueue (csrc/draws.cpp) for a table of the ext kernel and the kernel's index arithmetic, one workgroup after the other
extern "C" int rgx_emulate(const double *in, int nin, const rg_op *ops, int nops, long long nrows, long long seed, long long row0_global, double *out) {
  const int nout = rh_plan::generate_visible(ops, nops);
  std::vector<double> lds(rh_plan::generate_ext_lds_bytes(nout) / sizeof(double));
  int flags = 0;
  const long long tiles = rh_plan::generate_tiles(nrows);
  for (long long t = 0; t < tiles; t++) {
    const long long r0 = t * RG_TILE;
    const int valid = nrows - r0 < RG_TILE ? (int)(nrows - r0) : RG_TILE;
    rgx_block(in + r0 * nin, nin, ops, nops, nout, valid, seed, (rh_u64)row0_global + (rh_u64)r0, lds.data(), out + r0 * nout, &flags, RG_TILE);
  }
  return flags;
}
// what the plan says of a table: 0 its visible ops, 1 does it need the ext kernel, 2 its slabs, 3 the end of its first slab's ops
extern "C" int rgx_plan(const rg_op *ops, int nops, int what) {
  const int nout = rh_plan::generate_visible(ops, nops);
  int w = 0;
  return what == 0 ? nout : what == 1 ? (int)rh_plan::generate_uses_ext(ops, nops) : what == 2 ? rh_plan::generate_ext_slabs(ops, nops, nout)
                                                                                  : rh_plan::generate_ext_slab_end(ops, nops, nout, 0, &w);
}
'''
_emu = []


def emulation():
    """preamble + the prelude's rng + draws_plan.hpp (rh_generate.hip.h and rh_generate_ext.hip.h in host mode) + the driver -> a host
    shared library (g++ -O2 -ffp-contract=off -Werror, against liboracle's fdlibm)"""
    if not _emu:
        import tempfile
        O.load()
        d = tempfile.mkdtemp(prefix="rh_generate_ext_emu")
        cpp, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(cpp, "w").write(_PREAMBLE + prelude_rng_text() + _DRIVER)
        odir = os.path.join(ROOT, "oracle")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                               "-I", CSRC, "-shared", "-fPIC", cpp, "-o", so, "-L", odir, "-loracle", "-Wl,-rpath," + odir])
        L = C.CDLL(so)
        L.rgx_emulate.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(_capi.GenOp), C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_double)]
        L.rgx_plan.argtypes = [C.POINTER(_capi.GenOp), C.c_int, C.c_int]
        _emu.append(L)
    return _emu[0]


def emulate(x, ops, seed, chain0=0):
    """the host emulation over x [chains][kept][nin] -> (samples [chains][kept][visible ops], flags)"""
    ops = flat_ops(ops)
    x = np.ascontiguousarray(x, dtype=np.float64)
    chains, kept, nin = x.shape
    arr = (_capi.GenOp * len(ops))(*ops)
    out = np.full((chains, kept, len(visible(ops))), -7.0)
    flags = emulation().rgx_emulate(_capi.dptr(x), nin, arr, len(ops), chains * kept, seed, chain0 * kept, _capi.dptr(out))
    return out, flags


def plan(ops, what):
    ops = flat_ops(ops)
    return emulation().rgx_plan((_capi.GenOp * len(ops))(*ops), len(ops), what)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
NIN = 14
P, K, N, W3, PSI, LAM, BA, BB, LOC, SCALE, PEDGE = 0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13
KS = [0.0, 1.0, 2.7, 20.0, 99.0, 128.0, 1000.0]
NS = [0.0, 5.0, 128.0, 400.0]


def inputs(chains, kept, seed=None):
    """per-draw parameters [chains][kept][NIN], every one in its domain: a probability, a trial count and a failure count (every
    branch of both families among them), three weights (rows that sum below 1 and rows with a zero weight among them), psi and
    1 - psi, a Poisson rate on both branches, two Beta shapes, a location and a scale, a probability at the edges"""
    rng = np.random.default_rng(9100 * chains + kept if seed is None else seed)
    n = chains * kept
    x = np.empty((n, NIN))
    x[:, P] = rng.uniform(0.02, 0.98, size=n)
    x[:, K] = rng.choice(KS, size=n)
    x[:, N] = rng.choice(NS, size=n)
    w = rng.dirichlet([1.0, 1.0, 1.0], size=n) * rng.choice([1.0, 0.5], size=n)[:, None]
    w[rng.uniform(size=n) < 0.2, 1] = 0.0
    x[:, W3:W3 + 3] = w
    x[:, PSI] = rng.uniform(0.1, 0.9, size=n)
    x[:, PSI + 1] = 1 - x[:, PSI]
    x[:, LAM] = rng.choice([0.5, 3.0, 40.0], size=n)
    x[:, BA] = rng.uniform(0.3, 3.0, size=n)
    x[:, BB] = rng.uniform(0.3, 3.0, size=n)
    x[:, LOC] = rng.normal(size=n)
    x[:, SCALE] = np.abs(rng.normal(size=n)) + 0.1
    x[:, PEDGE] = rng.choice([0.0, 1.0, 10 / 128, 9 / 128], size=n)
    return x.reshape(chains, kept, NIN)


BETABIN = gen.BetaBinomial(c(BA), c(BB), c(K))
MIX3 = gen.Mixture(W3, [gen.Poisson(c(LAM)), gen.BetaBinomial(c(BA), c(BB), 20.0), gen.NegativeBinomial(c(P), 5.0)])   # a discrete mixture, a two-op component
MIX_NORMAL = gen.Mixture(PSI, [gen.Normal(c(LOC), c(SCALE)), gen.Normal(3.0, 0.5)])                                    # a continuous two-normal mixture
ZIP = gen.ZeroInflated(PSI, gen.Poisson(c(LAM)))
ONE = [gen.Binomial(c(P), c(K))]
FEW = [gen.Binomial(c(P), c(K)), gen.NegativeBinomial(c(P), c(N)), gen.Categorical(W3, 3), BETABIN, MIX3, MIX_NORMAL, ZIP, gen.Uniform(0.0, 1.0)]
# RG_SLAB + 1 visible columns.  Column 31 (the second slab's only one) is a mixture's: its hidden ops -- the CATEGORICAL, component 0,
# and the hidden BETA of component 1's BetaBinomial -- trail the first slab's 31st visible op, so (a) a hidden op is the last op before
# the boundary, (b) BINOMIAL(PREV) reads the carry across it and (c) the guarded run lies on both sides of it.
WIDE_HEAD = [gen.Binomial(c(P), 20.0), gen.hidden(gen.Normal(0.0, 1.0)), gen.Real(PREV), gen.NegativeBinomial(c(P), 5.0), gen.Categorical(W3, 3), gen.Categorical(PSI, 2),
             BETABIN, ZIP, gen.Binomial(c(PEDGE), 128.0), gen.Binomial(0.5, 1000.0), gen.hidden(gen.Gamma(c(BA), 1.0)), gen.Poisson(PREV), gen.NegativeBinomial(0.5, 400.0),
             gen.Normal(c(LOC), c(SCALE)), MIX_NORMAL, gen.Binomial(c(PEDGE), c(K)), gen.hidden(gen.Uniform(0.0, 1.0)), gen.Binomial(PREV, 7.0), gen.Geometric(c(P)),
             gen.NegativeBinomial(c(PEDGE), 3.0), gen.Bernoulli(c(P)), MIX3, gen.Cauchy(0.0, 1.0), gen.Binomial(c(P), 2.7), gen.Beta(c(BA), c(BB)), gen.Poisson(c(LAM)),
             gen.Binomial(0.25, 99.0), gen.NegativeBinomial(c(P), 2.0), gen.Laplace(c(LOC), 1.0), gen.Binomial(1.0, 5.0), gen.Binomial(0.0, 5.0), gen.LogNormal(0.5, 0.25),
             gen.Exponential(2.0), gen.Gamma(0.3, 2.0)]
WIDE = WIDE_HEAD + [gen.Mixture(W3, [gen.Poisson(c(LAM)), gen.BetaBinomial(c(BA), c(BB), 20.0), 4.0])[:3]
                    + [gen._copy(gen.Binomial(PREV, 20.0), guard=2, hidden=False)]]   # (component 1 last: its BINOMIAL is the column's op)
TABLES = {"one": ONE, "few": FEW, "wide": WIDE}


def test_the_wide_table_has_its_slab_boundary_where_the_docstring_says():
    ops = flat_ops(WIDE)
    vis = visible(ops)
    assert len(vis) == SLAB + 1 and plan(WIDE, 0) == SLAB + 1 and plan(WIDE, 2) == 2 and plan(WIDE, 1) == 1
    end = plan(WIDE, 3)                                            # the first slab's ops end here: the second starts at the last op
    assert end == len(ops) - 1 == vis[-1]
    before, after = ops[end - 1], ops[end]
    assert before.reserved & HIDDEN and before.family == _capi.GEN_BETA and before.reserved & 0xff == 2          # (a), and (c): guard 2 ...
    assert after.a.pad == _capi.GEN_ARG_PREV and after.family == _capi.GEN_BINOMIAL and after.reserved & 0xff == 2   # (b), ... on both sides
    assert ops[end - 2].reserved & 0xff == 1 and ops[end - 3].family == _capi.GEN_CATEGORICAL
    assert plan(ONE, 2) == 1 and plan(FEW, 0) == len(FEW) and plan(FEW_OPS, 1) == 0 and plan([gen.hidden(gen.Real(1.0))] + FEW_OPS, 1) == 1


@functools.lru_cache(maxsize=None)
def reference(chains, kept, name):
    """the oracle over the fixture of one shape, computed once: (x, samples, flags, passes); the arrays are read-only"""
    x, ps = inputs(chains, kept), PassesX()
    want, flags = oracle(x, TABLES[name], SEED, passes=ps)
    x.setflags(write=False); want.setflags(write=False)
    return x, want, flags, ps


# ---- 1. the host emulation against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,kept", SHAPES)
def test_host_emulation_has_the_oracles_bits(chains, kept):
    for name in TABLES:
        x, want, flags, ps = reference(chains, kept, name)
        got, got_flags = emulate(x, TABLES[name], SEED)
        assert same_bits(got, want), (chains, kept, name, np.argwhere(bits(got) != bits(want))[:4])
        assert flags == 0 and got_flags == 0
        # no in-domain fixture comes near the cap: the rejection loops as before, the exact paths at most the largest count of the fixture, 1000 of 4096
        assert max(v for k, v in ps.most.items() if not k.endswith("_exact")) <= 64 and max(ps.most["binomial_exact"], ps.most["negbin_exact"]) <= 1000, ps.most


# every branch, at exactly representable parameters (no boundary depends on a rounding): (op, the path the oracle must take)
BRANCHES = [(gen.Binomial(0.3, k), "binomial_exact") for k in (0.0, 1.0, 2.7, 99.0)] + [
    (gen.Binomial(10 / 128, 128.0), "binomial_poisson"),           # k * p = 10
    (gen.Binomial(9 / 128, 128.0), "binomial_poisson"),            # k * p = 9: Poisson wins over normal
    (gen.Binomial(1 - 9 / 128, 128.0), "binomial_normal"),         # k * (1 - p) = 9
    (gen.Binomial(1 - 8 / 128, 128.0), "binomial_exact"),          # 128 trials
    (gen.Binomial(0.5, 1000.0), "binomial_normal"),
    (gen.Binomial(0.0, 20.0), "binomial_exact"), (gen.Binomial(1.0, 20.0), "binomial_exact"),
    (gen.Binomial(0.0, 128.0), "binomial_poisson"), (gen.Binomial(1.0, 128.0), "binomial_exact"),
    (gen.NegativeBinomial(0.3, 0.0), "negbin_exact"),              # no trials
    (gen.NegativeBinomial(0.3, 5.0), "negbin_exact"),
    (gen.NegativeBinomial(0.1, 128.0), "negbin_exact"), (gen.NegativeBinomial(0.4, 128.0), "negbin_exact"),   # n = 128: the condition is empty
    (gen.NegativeBinomial(0.5, 400.0), "negbin_normal"),
    (gen.NegativeBinomial(0.75, 400.0), "negbin_exact"),           # 400 trials
    (gen.NegativeBinomial(0.0, 400.0), "negbin_exact"),            # all zeros
]


def test_every_branch_of_binomial_and_negbinomial():
    x = np.zeros((2, 60, 1))
    ops = [op for op, _ in BRANCHES]
    for o, (op, path) in enumerate(BRANCHES):
        ps = PassesX()
        oracle(x[:, :3], [op], SEED, passes=ps)
        assert {b for b in ps.branches if b.startswith(("binomial", "negbin"))} == {path}, (o, ps.branches)
    want, flags = oracle(x, ops, SEED + 2)
    got, got_flags = emulate(x, ops, SEED + 2)
    assert same_bits(got, want) and flags == 0 and got_flags == 0, np.argwhere(bits(got) != bits(want))[:4]
    col = lambda o: want[..., o].reshape(-1)
    assert np.all(col(0) == 0) and set(col(1)) == {0.0, 1.0} and set(col(2)) <= {0.0, 1.0, 2.0} and np.all(col(3) <= 99)   # (int)2.7 = 2 trials
    assert np.all(col(9) == 0) and np.all(col(10) == 20) and np.all(col(11) == 0) and np.all(col(12) == 128)             # p = 0 and p = 1
    assert np.all(col(13) == 0) and np.all(col(19) == 0)                                                                # n = 0; p = 0
    assert np.all(want >= 0) and np.all(want == np.floor(want)) and np.all(col(8) <= 1000) and np.all(col(7) <= 128)


@pytest.mark.parametrize("m", [2, 3, 5])
def test_categorical_walks_the_cdf(m):
    rng = np.random.default_rng(40 + m)
    w = rng.dirichlet(np.ones(m), size=300)
    w[:100] *= 0.25                                                # the weights sum below 1: the "else the last" arm
    w[100:200, 0] = 0.0                                            # a zero weight in front
    w[200:250, m - 1] = 0.0
    x = w.reshape(3, 100, m)
    ops = [gen.Categorical(0, m), gen.Uniform(0.0, 1.0)]
    want, flags = oracle(x, ops, SEED + m)
    got, got_flags = emulate(x, ops, SEED + m)
    assert same_bits(got, want) and flags == 0 and got_flags == 0
    u = np.array([O.JavaRandom(draw_seed(SEED + m, d)).next_double() for d in range(300)])
    idx = want[..., 0].reshape(-1)
    assert np.all(idx[:100][u[:100] > 0.2501] == m - 1) and (u[:100] > 0.2501).sum() > 50                  # u beyond the last cdf
    assert np.all(idx[100:200] >= 1) and set(idx) == set(range(m))


def test_composites():
    x = inputs(2, 150, seed=21)
    ops = [BETABIN, MIX3, MIX_NORMAL, ZIP]
    ps = PassesX()
    want, flags = oracle(x, ops, SEED + 3, passes=ps)
    got, got_flags = emulate(x, ops, SEED + 3)
    assert want.shape == (2, 150, 4) and same_bits(got, want) and flags == 0 and got_flags == 0
    assert max(v for k, v in ps.most.items() if not k.endswith("_exact")) <= 64, ps.most
    every, _ = oracle(x, ops, SEED + 3, all_ops=True)
    flat = flat_ops(ops)
    # BetaBinomial: its column is Binomial(the hidden Beta's sample, k)
    assert np.all((0 < every[..., 0]) & (every[..., 0] < 1)) and np.all(want[..., 0] <= x[..., K]) and same_bits(every[..., 1], want[..., 0])
    # the mixtures: the last op's column is the chosen component's sample in every draw
    cat = flat.index(MIX3[0], 2)
    sel = every[..., cat]
    assert set(sel.reshape(-1)) == {0.0, 1.0, 2.0}
    for j, last in ((0, cat + 1), (1, cat + 3), (2, cat + 4)):
        assert same_bits(every[..., last][sel == j], want[..., 1][sel == j])
    zsel = every[..., len(flat) - 3]
    assert np.all(want[..., 3][zsel == 0] == 0.0) and (zsel == 0).sum() > 50 and (want[..., 3][zsel == 1] > 0).any()
    assert abs((zsel == 0).mean() - x[..., PSI].mean()) < 5 * 0.5 / math.sqrt(300)


# ---- 2. the guards -----------------------------------------------------------------------------------------------------------------
BAD = {"binomial_p": [NAN, math.inf, -math.inf, -0.1, 1.5], "binomial_k": [NAN, math.inf, -math.inf, -1.0],
       "negbin_p": [NAN, math.inf, -0.1, 1.5], "negbin_n": [NAN, math.inf, -math.inf, -1.0], "weight": [NAN, math.inf, -math.inf, -0.25]}


@pytest.mark.parametrize("what", sorted(BAD))
def test_domain_guards_give_nan_and_leave_the_stream_untouched(what):
    bad = BAD[what]
    guarded = {"binomial_p": gen.Binomial(c(0), 20.0), "binomial_k": gen.Binomial(0.3, c(0)), "negbin_p": gen.NegativeBinomial(c(0), 5.0),
               "negbin_n": gen.NegativeBinomial(0.3, c(0)), "weight": gen.Categorical(0, 2)}[what]
    before, after = [gen.Normal(0.0, 1.0)], [gen.Normal(1.0, 2.0), gen.Uniform(0.0, 1.0)]
    good = 6.0 if what in ("binomial_k", "negbin_n") else 0.5
    x = np.array([[v, 0.5] for v in bad] + [[good, 0.5]]).reshape(1, -1, 2)   # the last draw is in the domain
    got, flags = emulate(x, before + [guarded] + after, SEED)
    want, want_flags = oracle(x, before + [guarded] + after, SEED)
    assert same_bits(got, want) and flags == want_flags == F_DOMAIN
    assert np.all(np.isnan(got[0, :-1, 1])) and not np.isnan(got[0, -1, 1])
    rest, rest_flags = emulate(x, before + [gen.hidden(gen.Real(0.0))] + after, SEED)   # the table without the guarded op
    assert rest_flags == 0 and same_bits(got[0, :-1][:, [0, 2, 3]], rest[0, :-1])       # the next op's sample: as had the op not been there
    assert not same_bits(got[0, -1, 2:], rest[0, -1, 1:])                              # ... and the op in its domain did draw


def test_an_exact_path_beyond_the_cap_gives_nan_and_draws_nothing():
    x = np.zeros((1, 5, 1))
    for op in (gen.Binomial(1 - 5 / 8192, 8192.0), gen.NegativeBinomial(0.99, 8192.0), gen.Binomial(1.0, 1e300), gen.NegativeBinomial(1.0, 1e300)):
        tail = [gen.Uniform(0.0, 1.0), gen.Normal(0.0, 1.0)]
        got, flags = emulate(x, [op] + tail, SEED)
        want, want_flags = oracle(x, [op] + tail, SEED)
        assert same_bits(got, want) and flags == want_flags == F_CAP and np.all(np.isnan(got[..., 0]))
        rest, _ = emulate(x, [gen.hidden(gen.Real(0.0))] + tail, SEED)
        assert same_bits(got[..., 1:], rest)                       # an untouched stream
    full = [gen.Binomial(1.0, 4096.0), gen.NegativeBinomial(0.99, 4096.0)]      # 4096 trials are not beyond it
    at_cap, flags = emulate(x[:, :2], full, SEED)
    assert flags == 0 and np.all(at_cap[..., 0] == 4096) and same_bits(at_cap, oracle(x[:, :2], full, SEED)[0])


def test_a_nan_selector_leaves_the_mixtures_column_nan():
    x = inputs(1, 40, seed=8).copy()
    x[0, ::3, W3 + 1] = -1.0                                       # a negative weight: the CATEGORICAL is NaN, no guard matches
    ops = [gen.Normal(0.0, 1.0), MIX3, gen.Uniform(0.0, 1.0)]
    got, flags = emulate(x, ops, SEED)
    want, want_flags = oracle(x, ops, SEED)
    assert same_bits(got, want) and flags == want_flags == F_DOMAIN
    assert np.all(np.isnan(got[0, ::3, 1])) and not np.any(np.isnan(got[0, 1::3, 1])) and not np.any(np.isnan(got[0, 2::3, 1]))
    plain, _ = emulate(x, [gen.Normal(0.0, 1.0), gen.Uniform(0.0, 1.0)], SEED)
    assert same_bits(got[0, ::3][:, [0, 2]], plain[0, ::3])        # nothing was drawn for the mixture there


# ---- 3. the semantics of the table -------------------------------------------------------------------------------------------------
def test_a_skipped_op_draws_nothing_and_hidden_ops_leave_no_column():
    x = inputs(2, 100, seed=12)
    mix = gen.Mixture(PSI, [gen.Gamma(c(BA), 1.0), gen.Poisson(40.0)])
    ops = [mix, gen.Uniform(0.0, 1.0)]
    got, flags = emulate(x, ops, SEED)
    every, _ = oracle(x, ops, SEED, all_ops=True)
    assert flags == 0 and got.shape == (2, 100, 2) and same_bits(got, every[..., [2, 3]])   # hidden ops leave no column
    sel = every[..., 0]
    # the stream position behind the mixture, through the trailing UNIFORM: that of a table with the chosen component alone
    for j, comp in ((0, gen.Gamma(c(BA), 1.0)), (1, gen.Poisson(40.0))):
        alone, _ = emulate(x, [gen.hidden(gen.Uniform(0.0, 1.0)), comp, gen.Uniform(0.0, 1.0)], SEED)   # (the CATEGORICAL's one uniform first)
        assert (sel == j).sum() > 20 and same_bits(got[sel == j], alone[sel == j])
    # a visible guarded op that is skipped shows the carry
    raw = [gen.Real(7.5), gen.hidden(gen.Categorical(PSI, 2)), gen._copy(gen.Normal(0.0, 1.0), guard=2), gen.Real(PREV)]
    got, _ = emulate(x, raw, SEED)
    sel = oracle(x, raw, SEED, all_ops=True)[0][..., 1]
    assert np.all(got[..., 1][sel == 0] == 0.0) and np.all(got[..., 1][sel == 1] != 0.0) and same_bits(got[..., 1], got[..., 2])   # (the carry: the CATEGORICAL's 0)
    assert same_bits(got, oracle(x, raw, SEED)[0])


def test_results_do_not_depend_on_shape_or_sharding():
    x = inputs(3, 86, seed=5)
    whole, _ = emulate(x, WIDE, SEED)
    flat, _ = emulate(x.reshape(1, 258, NIN), WIDE, SEED)
    assert same_bits(whole.reshape(-1), flat.reshape(-1))
    y = inputs(4, 86, seed=6)
    run, _ = emulate(y, FEW, SEED)
    shard, _ = emulate(y[2:], FEW, SEED, chain0=2)
    assert same_bits(shard, run[2:]) and same_bits(oracle(y[2:], FEW, SEED, chain0=2)[0], run[2:])
    other, _ = emulate(y, FEW, SEED + 1)
    assert same_bits(emulate(y, FEW, SEED)[0], run) and not same_bits(other[..., -1], run[..., -1])


def test_an_old_table_through_the_ext_kernel_has_rh_generates_bits():
    from tests.test_generate_device_cpu import ALL_OPS
    for old in (FEW_OPS, ALL_OPS):
        x = old_inputs(2, 150, seed=31)
        want, _ = emulate_old(x, old, SEED)
        for at in (0, len(old) // 2, len(old)):                    # one hidden REAL forces the ext kernel
            ops = old[:at] + [gen.hidden(gen.Real(1.0))] + old[at:]
            assert plan(old, 1) == 0 and plan(ops, 1) == 1
            got, flags = emulate(x, ops, SEED)
            assert flags == 0 and same_bits(got, want), at


# ---- 4. the exact paths sample what they say ---------------------------------------------------------------------------------------
def test_the_exact_paths_have_their_laws():
    """20 000 draws of the host emulation, |mean - mu| <= 5 sigma / sqrt(N) (and the frequencies likewise): the exact paths ARE
    binomial, negative binomial (failures n, success probability p: mean n p / (1 - p), variance n p / (1 - p)^2) and categorical.
    The approximated branches are not: only the bitwise oracle pins them."""
    n = 20000
    w = np.array([0.125, 0.5, 0.375])
    x = np.tile(w, (1, n, 1))
    p2 = 1 - 8 / 128
    ops = [gen.Binomial(0.3, 20.0), gen.Binomial(p2, 128.0), gen.NegativeBinomial(0.3, 5.0), gen.Categorical(0, 3)]
    got, flags = emulate(x, ops, SEED + 9)
    assert flags == 0
    for o, (mu, var) in enumerate([(20 * 0.3, 20 * 0.3 * 0.7), (128 * p2, 128 * p2 * (1 - p2)), (5 * 0.3 / 0.7, 5 * 0.3 / 0.7 ** 2)]):
        assert abs(got[0, :, o].mean() - mu) <= 5 * math.sqrt(var / n), (o, got[0, :, o].mean(), mu)
    for i, wi in enumerate(w):
        assert abs((got[0, :, 3] == i).mean() - wi) <= 5 * math.sqrt(wi * (1 - wi) / n)


# ---- 5. the code object ------------------------------------------------------------------------------------------------------------
def test_ext_kernel_cross_compiles_without_spills_or_scratch():
    code = _capi.generate_ext_lower_only()
    rep = _capi.code_object_report(code)
    assert sorted(k for _, k in rep) == [KERNEL]                   # ... and not a second rh_generate_kernel
    assert _kernel_meta(code, KERNEL, ".vgpr_spill_count") == 0 and _kernel_meta(code, KERNEL, ".sgpr_spill_count") == 0
    assert _kernel_meta(code, KERNEL, ".private_segment_fixed_size") == 0
    r = rep[("object", KERNEL)]
    assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r
    import glob
    kc = os.path.join(ROOT, "rainier_amd", "kcache")
    if not os.environ.get("RH_KERNEL_CACHE"):
        assert any(open(f, "rb").read() == code for f in glob.glob(os.path.join(kc, "*.generate_ext.co")))   # it travels in the kernel cache
    before = _capi.lib().rh_compile_count()
    assert _capi.generate_ext_lower_only() == code and _capi.lib().rh_compile_count() == before   # served by the kernel cache
    assert _capi.generate_lower_only() != code


# ---- 6. rh_generate_create's refusals and the Python constructors --------------------------------------------------------------------
def test_create_refuses_with_the_op_named():
    L = _capi.lib()
    err = lambda: L.rh_last_error(None).decode()
    h = C.c_void_p()

    def create(ops, nin=4):
        ops = flat_ops(ops)
        arr = (_capi.GenOp * max(1, len(ops)))(*ops)
        return L.rh_generate_create(arr, len(ops), nin, -1, C.byref(h))
    raw = lambda f, a, b, res=0: _capi.GenOp(f, res, _capi.GenArg(*a), _capi.GenArg(*b))
    imm = lambda v: (-1, 0, v)
    bad = lambda ops, *texts, **kw: create(ops, **kw) == _capi.RH_E_INVALID and not h and all(t in err() for t in texts)
    # guards
    assert bad([gen.Real(1.0), gen._copy(gen.Normal(0.0, 1.0), guard=1)], "op 1 (NORMAL)", "no earlier CATEGORICAL")
    assert bad([gen.Categorical(0, 2), gen._copy(gen.Poisson(1.0), guard=3)], "op 1 (POISSON)", "selector 2", "2 outcomes")
    assert bad([gen.Categorical(0, 3), gen.Categorical(0, 2), gen._copy(gen.Real(1.0), guard=3)], "op 2 (REAL)", "2 outcomes")   # the NEAREST one
    assert bad([raw(_capi.GEN_REAL, imm(1.0), imm(0.0), res=0x200)], "op 0 (REAL)", "unknown flag bits")
    # PREV
    assert bad([gen.Binomial(PREV, 5.0)], "op 0 (BINOMIAL)", "RH_GEN_ARG_PREV at op 0")
    assert bad([gen.Real(0.5), raw(_capi.GEN_BINOMIAL, (0, 1, 0.0), imm(5.0))], "op 1 (BINOMIAL)", "col must be -1")
    assert bad([gen.Real(0.5), raw(_capi.GEN_NORMAL, (-1, 2, 0.0), imm(5.0))], "op 1 (NORMAL)", "unknown argument source 2")
    # hidden
    assert bad([gen.hidden(gen.Real(1.0)), gen.hidden(gen.Poisson(2.0))], "no visible op")
    # CATEGORICAL
    assert bad([raw(_capi.GEN_CATEGORICAL, imm(0.5), imm(2.0))], "op 0 (CATEGORICAL)", "must be a column")
    assert bad([gen.Real(1.0), raw(_capi.GEN_CATEGORICAL, (-1, 1, 0.0), imm(2.0))], "op 1 (CATEGORICAL)", "must be a column")
    for m in (1.0, 256.0, 2.5, NAN):
        assert bad([raw(_capi.GEN_CATEGORICAL, (0, 0, 0.0), imm(m))], "op 0 (CATEGORICAL)", "integer in 2 .. 255")
    assert bad([raw(_capi.GEN_CATEGORICAL, (0, 0, 0.0), (1, 0, 0.0))], "op 0 (CATEGORICAL)", "immediate")
    assert bad([gen.Categorical(2, 3)], "op 0 (CATEGORICAL)", "weight columns 2 .. 4")
    assert bad([raw(19, imm(0.0), imm(0.0))], "op 0: unknown family 19") and bad([raw(15, imm(0.0), imm(0.0))], "op 0: unknown family 15")
    # ... and what is sound needs no device
    assert create([gen.Categorical(1, 3)]) == _capi.RH_OK and L.rh_generate_nout(h) == 1
    L.rh_generate_destroy(h)
    assert create([MIX_NORMAL, gen.Real(PREV)], nin=NIN) == _capi.RH_OK and L.rh_generate_nout(h) == 2
    L.rh_generate_destroy(h)


def test_python_constructors():
    b, nb = gen.Binomial(c(1), 12.0), gen.NegativeBinomial(0.25, c(2))
    assert (b.family, b.reserved, b.a.col, b.a.pad, b.b.col, b.b.value) == (_capi.GEN_BINOMIAL, 0, 1, 0, -1, 12.0) and _capi.GEN_BINOMIAL == 16
    assert (nb.family, nb.a.col, nb.a.value, nb.b.col) == (_capi.GEN_NEGBINOMIAL, -1, 0.25, 2)
    cat = gen.Categorical(c(3), 4)
    assert (cat.family, cat.a.col, cat.b.col, cat.b.value) == (_capi.GEN_CATEGORICAL, 3, -1, 4.0) and gen.Categorical(3, 4).a.col == 3
    bb = gen.BetaBinomial(c(0), 2.0, 9.0)
    assert [(o.family, o.reserved) for o in bb] == [(_capi.GEN_BETA, HIDDEN), (_capi.GEN_BINOMIAL, 0)]
    assert (bb[1].a.col, bb[1].a.pad, bb[1].b.value) == (-1, _capi.GEN_ARG_PREV, 9.0)
    mix = gen.Mixture(2, [gen.Poisson(3.0), bb, 1.5])
    assert [(o.family, o.reserved) for o in mix] == [(_capi.GEN_CATEGORICAL, HIDDEN), (_capi.GEN_POISSON, HIDDEN | 1), (_capi.GEN_BETA, HIDDEN | 2),
                                                     (_capi.GEN_BINOMIAL, HIDDEN | 2), (_capi.GEN_REAL, 3)]
    assert (mix[0].a.col, mix[0].b.value, mix[4].a.value) == (2, 3.0, 1.5) and bb[0].reserved == HIDDEN   # the component's own ops are copied
    z = gen.ZeroInflated(c(0), gen.Poisson(c(2)))
    assert [(o.family, o.reserved, o.a.col, o.a.value) for o in z] == [(_capi.GEN_CATEGORICAL, HIDDEN, 0, 0.0), (_capi.GEN_REAL, HIDDEN | 1, -1, 0.0),
                                                                       (_capi.GEN_POISSON, 2, 2, 0.0)]
    with pytest.raises(ValueError, match="mixture itself"):
        gen.Mixture(0, [mix, gen.Real(1.0)])
    g = R.Generator([b, bb, mix, z, gen.hidden(gen.Normal(0.0, 1.0)), gen.Real(PREV)], nin=5)   # one level of nesting is flattened
    assert (g.nin, g.nout, g.flags) == (5, 5, 0)                   # the visible ops: one per plain op and per composite
    g.close()
    flat = R.Generator([gen.Normal(c(0), 1.0), gen.Poisson(2.0)], nin=1)                        # a flat list behaves as before
    assert flat.nout == 2
    flat.close()
    with pytest.raises(R.RainierHipError, match=r"op 1 \(BINOMIAL\): column 5"):
        R.Generator([gen.Real(1.0), gen.Binomial(c(5), 3.0)], nin=5)
