"""Trace.predict / Trace.thin over device-resident draws (csrc/device/rh_predict.hip.h), the part that needs no GPU:

  * three requirements programs -- funnel_predict(10) (dense in a short vector: the flat staging), 4 of 704 parameters (the gathered
    staging) and all 704 (more than a wavefront of staged draws holds: the direct kernel) -- cross-compile for gfx950 through the
    engine's own path (kernel cache, kernel_health, isacheck) in fast and strict math; their kernels spill nothing and use no
    scratch, and RH_NREF / rh_req_ref name exactly the parameters the program reads;
  * the source rh_requirements_eval builds is the one it built before the predictor existed (kernel-cache key);
  * the very text of the block routine, compiled with the host g++ (contraction off, the oracle's fdlibm behind RH_EXP / RH_LOG)
    with every "thread" of a phase run in turn, walked over whole buffers exactly as the launches walk them and compared with the
    oracle's OracleDensity.requirements of the kept rows, bit for bit;
  * the C ABI's argument errors, its refusal to compute without a device, and the host Trace's thin / predict.

tests/test_gpu_predict_device.py runs the same fixtures through the kernels and asks for the emulation's bits.
"""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rainier_amd import _capi, models
from tests import oracle_lib as O
from tests.test_capi_cpu import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT, GATHER, DIRECT = 0, 1, 2
KERNEL = {FLAT: "rh_predict_flat_kernel", GATHER: "rh_predict_gather_kernel", DIRECT: "rh_predict_direct_kernel"}

SHAPES = [(1, 1), (3, 33), (2, 257), (2, 1000)]


def windows(n):
    """(first, count, thin) that fit n iterations: everything, all but the first, thinned, a short thinned window inside, thin > count
    (one kept row), the last row alone"""
    w = [(0, n, 1), (1, n - 1, 1), (0, n, 3), (5, 20, 7), (0, n, n + 1), (n - 1, 1, 1)]
    return sorted({x for x in w if x[1] >= 1 and x[0] + x[1] <= n})


def programs():
    """name -> (rir, nreq, nvars, the parameters it reads, the kernels it gets)"""
    return {
        "funnel": models.funnel_predict(10) + (10, list(range(10)), (FLAT, GATHER)),
        "sparse": models.sparse_predict(704) + (704, [0, 351, 352, 703], (GATHER,)),
        "dense": models.dense_predict(704) + (704, list(range(704)), (DIRECT,)),
    }


def synthetic_draws(chains, iterations, nvars, seed=None):
    rng = np.random.default_rng(1000 * chains + iterations + nvars if seed is None else seed)
    return rng.normal(size=(chains, iterations, nvars)) * 0.7


_oracles = {}


def oracle_rows(name, rows):
    """OracleDensity.requirements (fdlibm exp / log: the strict mode's arithmetic) of every row of rows [..., nvars]"""
    rir, nreq, nvars = programs()[name][:3]
    if name not in _oracles:
        _oracles[name] = O.OracleDensity(models.ModelSpec("req", rir, [], [0] * nreq, nvars), O.JM_DET)
    d = _oracles[name]
    flat = np.ascontiguousarray(rows).reshape(-1, nvars)
    return np.array([d.requirements(q, nreq) for q in flat]).reshape(rows.shape[:-1] + (nreq,))


def kept_rows(x, first, count, thin):
    return x[:, first:first + count:thin, :]


# ---- the device text on the host ---------------------------------------------------------------------------------------------------
_PREAMBLE = r'''
#include <cmath>
#include <vector>
#define RH_PREDICT_HOST 1
#define RH_DEV static inline
#define RH_NAN (__builtin_nan(""))
#define RH_INF (__builtin_inf())
// strict math: the oracle's fdlibm (oracle/jmath.c), which the device's rh_strict_exp / rh_strict_log are bit-compared with on the GPU
extern "C" double jm_strict_exp(double);
extern "C" double jm_strict_log(double);
static inline double rh_strict_exp(double x) { return jm_strict_exp(x); }
static inline double rh_strict_log(double x) { return jm_strict_log(x); }
static inline int rh_d2i(double x) { if (x != x) return 0; if (x >= 2147483647.0) return 2147483647; if (x <= -2147483648.0) return (-2147483647 - 1); return (int)x; }
static inline double rh_compare(double a, double b) { return a > b ? 1.0 : (a == b ? 0.0 : -1.0); }
using std::exp; using std::log; using std::fabs;
'''
_DRIVER = r'''
// the launch of predict_run (csrc/draws.cpp) and the kernels' index arithmetic, one workgroup after the other
template <int FORM> static int rp_walk(const double *draws, int chains, long long iterations, int first, int count, int thin, double *out) {
  const int kept = (count + thin - 1) / thin, tile = rp_cfg<FORM>::TILE, ntiles = (kept + tile - 1) / tile;
  std::vector<double> lds(rp_lds<FORM>::DOUBLES);
  int err = 0;
  for (int chain = 0; chain < chains; chain++)
    for (int t = 0; t < ntiles; t++) {
      const int k0 = t * tile, valid = kept - k0 < tile ? kept - k0 : tile;
      rp_block<FORM>(draws + ((long long)chain * iterations + first) * RH_NVARS, thin, k0, valid, lds.data(),
                     out + ((long long)chain * kept + k0) * RH_NREQ, &err, tile);
    }
  return err;
}
// form < 0: the engine's choice (flat when the program has that kernel and thin == 1, else gathered, else direct)
extern "C" int rp_emulate(int form, const double *draws, int chains, long long iterations, int first, int count, int thin, double *out) {
  if (form < 0) form = (RP_HAVE_FLAT && thin == 1) ? RP_FLAT : (RP_HAVE_GATHER ? RP_GATHER : RP_DIRECT);
#if RP_HAVE_FLAT
  if (form == RP_FLAT && thin == 1) return rp_walk<RP_FLAT>(draws, chains, iterations, first, count, thin, out);
#endif
#if RP_HAVE_GATHER
  if (form == RP_GATHER) return rp_walk<RP_GATHER>(draws, chains, iterations, first, count, thin, out);
#endif
#if RP_HAVE_DIRECT
  if (form == RP_DIRECT) return rp_walk<RP_DIRECT>(draws, chains, iterations, first, count, thin, out);
#endif
  return -1;
}
'''
_PROBE = r'''
extern "C" int rp_have(int form) { return form == RP_FLAT ? RP_HAVE_FLAT : form == RP_GATHER ? RP_HAVE_GATHER : RP_HAVE_DIRECT; }
extern "C" int rp_tile(int form) { return form == RP_FLAT ? RP_FTILE : form == RP_GATHER ? RP_GTILE : RP_DTILE; }
extern "C" int rp_lds_bytes(int form) { return 8 * (form == RP_FLAT ? rp_lds<RP_FLAT>::DOUBLES : form == RP_GATHER ? rp_lds<RP_GATHER>::DOUBLES : rp_lds<RP_DIRECT>::DOUBLES); }
extern "C" int rp_nref(void) { return RH_NREF; }
extern "C" int rp_ref(int s) { return rh_req_ref[s]; }
'''
_emu = {}


def split_source(src):
    """the lowered source -> (the program's defines, the generated rh_pred_eval): what surrounds rh_shared.h / the prelude"""
    head = src[:src.index("// rh_shared.h")]
    i = src.index("template <class RH_TH> RH_DEV void rh_pred_eval")
    j = src.rfind("#pragma clang fp contract(fast)", 0, i)
    body = src[j if j >= 0 and src[j:i].strip() == "#pragma clang fp contract(fast)" else i:src.index("// rh_predict.hip.h")]
    return head, body


def _compile(head, body, driver, opt="-O2"):
    """preamble + the program's defines + its generated code + rh_predict.hip.h + a driver -> a host shared library (g++,
    -ffp-contract=off: every a*b+c stays two roundings, as hiprtc is told for the device)"""
    import tempfile
    O.load()                                                    # (builds oracle/liboracle.so when it is not there)
    d = tempfile.mkdtemp(prefix="rh_predict_emu")
    cpp, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
    hdr = os.path.join(ROOT, "rainier_amd", "csrc", "device", "rh_predict.hip.h")
    open(cpp, "w").write(_PREAMBLE + head + body + '#include "%s"\n' % hdr + driver)
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-std=c++17", opt, "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-Wno-unused-variable", "-shared", "-fPIC", cpp, "-o", so, "-L", odir, "-loracle", "-Wl,-rpath," + odir])
    return C.CDLL(so)


def emulation(name):
    """the strict-math lowering of one of programs(), compiled for the host with the walking driver"""
    if name not in _emu:
        rir = programs()[name][0]
        src, _ = _capi.lower_predict(rir, _capi.compile_opts(math_mode=_capi.MATH_STRICT), compile=False)
        head, body = split_source(src)
        L = _compile(head, body, _DRIVER + _PROBE)
        L.rp_emulate.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        _emu[name] = L
    return _emu[name]


def emulate(name, x, first=0, count=None, thin=1, form=-1):
    """the host emulation over x [chains][iterations][nvars] -> [chains][kept][nreq] (strict math); form: one of the program's kernels,
    -1: the one the engine launches for this `thin`"""
    L = emulation(name)
    nreq = programs()[name][1]
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, iters, _ = x.shape
    count = iters - first if count is None else count
    out = np.full((m, -(-count // thin), nreq), -7.0)
    rc = L.rp_emulate(form, _capi.dptr(x), m, iters, first, count, thin, _capi.dptr(out))
    assert rc == 0, (name, form, rc)
    return out


# ---- 1. the code objects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["funnel", "sparse", "dense"])
def test_predict_kernels_cross_compile_without_spills_or_scratch(name):
    rir, nreq, nvars, reads, forms = programs()[name]
    for mode in (_capi.MATH_FAST, _capi.MATH_STRICT):
        src, code = _capi.lower_predict(rir, _capi.compile_opts(math_mode=mode))
        rep = _capi.code_object_report(code)
        assert sorted(k for _, k in rep) == sorted(KERNEL[f] for f in forms), (name, mode, sorted(rep))
        for f in forms:
            k = KERNEL[f]
            assert _kernel_meta(code, k, ".vgpr_spill_count") == 0 and _kernel_meta(code, k, ".sgpr_spill_count") == 0
            assert _kernel_meta(code, k, ".private_segment_fixed_size") == 0
            r = rep[("object", k)]
            assert r["fit"] == 1 and r["scratch"] == 0 and r["why"] == "", r       # kernel_health: metadata + isacheck's walk
        # the parameters the program reads, and nothing of a full-length array in the generated code
        assert int(re.search(r"#define RH_NREF (\d+)", src).group(1)) == len(reads)
        assert [int(v) for v in re.search(r"#define RH_REQ_REF_INIT \{([^}]*)\}", src).group(1).split(",")] == reads
        head, body = split_source(src)
        assert "th[" not in body and "th(" in body and "double th[RH_NVARS]" not in src
        # a second call is served by the kernel cache
        before = _capi.lib().rh_compile_count()
        assert _capi.lower_predict(rir, _capi.compile_opts(math_mode=mode))[1] == code and _capi.lib().rh_compile_count() == before
    # registers follow the program's live temporaries, not RH_NREF: the 704-parameter programs stay far below the 512 of a lane
    assert _kernel_meta(code, KERNEL[forms[-1]], ".vgpr_count") <= 128


def test_the_bound_on_referenced_parameters():
    """64 draws x (RH_NREF | 1) doubles must fit the 8064 staged doubles (63 KiB): 125 referenced parameters are staged, 126 are
    not; up to 31 the tile is 256 draws"""
    from rainier_amd.frontend import Graph
    for nref, want in ((31, (1, 256, 0)), (32, (1, 192, 0)), (125, (1, 64, 0)), (126, (0, 0, 1))):
        g = Graph(300, [])
        s = g.param(0) * 1.0
        for i in range(1, nref):
            s = s + g.param(2 * i)
        src, _ = _capi.lower_predict(g.compile_requirements([s]), compile=False)
        head, _body = split_source(src)
        assert "#define RH_NREF %d\n" % nref in head
        L = _compile(head, "", _PROBE, opt="-O0")
        assert (L.rp_have(GATHER), L.rp_tile(GATHER), L.rp_have(DIRECT)) == want and L.rp_have(FLAT) == 0, nref
        assert L.rp_lds_bytes(GATHER if want[0] else DIRECT) <= 63 * 1024          # two workgroups share a CU's 160 KiB


# ---- 2. rh_requirements_eval is what it was --------------------------------------------------------------------------------------------
# sha256 of the kernel-cache key (the file name build_source gives the code object: a hash of architecture, compiler and SOURCE) of
# the program rh_requirements_eval builds for funnel_predict(10), default options, taken on the commit before rh_predict existed
REQ_EVAL_KEY_SHA = "d4f82ec826b9a9bcf9a0e01f96405873371442bf038d474fa392f55c4248bb33"


def requirements_eval_cache_key():
    """in a fresh process (the key carries which compiler libraries the process has bound): rh_requirements_eval of funnel_predict(10)
    with an empty kernel cache of its own -> the name of the one file it leaves there"""
    import tempfile
    d = tempfile.mkdtemp(prefix="rh_req_key")
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from rainier_amd import _capi, models\n"
            "rir, nreq = models.funnel_predict(10)\n"
            "x, o = np.zeros((1, 10)), np.zeros((1, nreq))\n"
            "rc = _capi.lib().rh_requirements_eval(C.create_string_buffer(rir, len(rir)), len(rir), None, _capi.dptr(x), 0, _capi.dptr(o))\n"
            "assert rc == 0, rc\n" % ROOT)
    env = dict(os.environ, RH_KERNEL_CACHE=d, RH_DIAG="1", RH_LOWER_ONLY="1")
    env.pop("RH_NO_KERNEL_CACHE", None)
    subprocess.check_call([sys.executable, "-c", code], env=env)
    names = [f for f in os.listdir(d) if f.endswith(".hsaco")]
    assert len(names) == 1, names
    return names[0]


def test_requirements_eval_source_is_unchanged():
    assert hashlib.sha256(requirements_eval_cache_key().encode()).hexdigest() == REQ_EVAL_KEY_SHA
    # and the predictor's source is another translation unit: its own kernels, none of rh_requirements_eval's
    src, _ = _capi.lower_predict(models.funnel_predict(10)[0], compile=False)
    assert "rh_req_kernel" not in src and "void rh_req_eval(" not in src and "RP_KERNEL(rh_predict_gather_kernel" in src


# ---- 3. the device text, on the host, against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,n", SHAPES)
@pytest.mark.parametrize("name", ["funnel", "sparse"])
def test_host_emulation_matches_the_oracle_bit_for_bit(name, chains, n):
    nvars, forms = programs()[name][2], programs()[name][4]
    x = synthetic_draws(chains, n, nvars)
    for first, count, thin in windows(n):
        want = oracle_rows(name, kept_rows(x, first, count, thin))
        for form in forms:
            if form == FLAT and thin != 1:
                continue                                        # the flat staging needs contiguous rows
            got = emulate(name, x, first, count, thin, form)
            assert got.shape == want.shape and np.array_equal(got, want), (name, chains, n, first, count, thin, form)
        assert np.array_equal(emulate(name, x, first, count, thin), want)      # the engine's own choice of kernel


def test_host_emulation_direct_form_and_tiles():
    """all 704 parameters: no staging, 64 draws per tile (a boundary at 64 and a ragged last tile of 257 - 256 = 1)"""
    x = synthetic_draws(2, 257, 704)
    for first, count, thin in ((0, 257, 1), (1, 256, 1), (0, 257, 3), (5, 20, 7), (256, 1, 1)):
        assert np.array_equal(emulate("dense", x, first, count, thin), oracle_rows("dense", kept_rows(x, first, count, thin)))
    L = emulation("funnel")
    assert (L.rp_have(FLAT), L.rp_have(GATHER), L.rp_have(DIRECT)) == (1, 1, 0) and L.rp_tile(FLAT) == 256 and L.rp_tile(GATHER) == 256
    L = emulation("sparse")
    assert (L.rp_have(FLAT), L.rp_have(GATHER), L.rp_have(DIRECT)) == (0, 1, 0) and L.rp_tile(GATHER) == 256
    assert [L.rp_ref(s) for s in range(L.rp_nref())] == [0, 351, 352, 703]
    L = emulation("dense")
    assert (L.rp_have(FLAT), L.rp_have(GATHER), L.rp_have(DIRECT)) == (0, 0, 1) and L.rp_tile(DIRECT) == 64


# ---- 4. the C ABI without a device, and the host Trace -------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    L = _capi.lib()
    err = lambda: L.rh_last_error(None).decode()
    h = C.c_void_p()
    rir = models.funnel_predict(10)[0]
    create = lambda blob: L.rh_predict_create(C.create_string_buffer(blob, len(blob)), len(blob), None, C.byref(h))
    assert create(models.funnel(10).rir) == _capi.RH_E_INVALID and err() == "not a requirements program (header kind != 1)" and not h
    assert create(rir[:20]) == _capi.RH_E_INVALID and not h
    assert L.rh_predict_create(None, 0, None, C.byref(h)) == _capi.RH_E_INVALID
    assert L.rh_predict_nreq(None) == -1 and L.rh_predict_nvars(None) == -1
    L.rh_predict_destroy(None)
    out = np.zeros(8)
    fake = C.c_void_p(4096)            # never dereferenced: refused before the first device call
    assert L.rh_predict_device(None, fake, 0, 4, 10, 10, 0, 10, 1, _capi.dptr(out), None) == _capi.RH_E_INVALID
    assert L.rh_sampler_predict(None, None, 0, 10, 1, _capi.dptr(out), None) == _capi.RH_E_INVALID
    with pytest.raises(_capi.RainierHipError, match="header kind"):
        _capi.lower_predict(models.funnel(10).rir)
    if L.rh_device_count() == 0:
        assert create(rir) == _capi.RH_E_DEVICE and "no CPU fallback" in err() and not h
        import rainier_amd as R
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.Predictor(rir)


def test_host_trace_thin_and_python_surface():
    import inspect
    import rainier_amd as R
    from rainier_amd import distributed
    x = synthetic_draws(3, 10, 2)
    tr = R.Trace(x, np.ones((3, 2)), ["stats"])
    assert tr.thin(1).chains.shape == x.shape and np.array_equal(tr.thin(1).chains, x)          # Trace.scala:23-32: i % n == 0
    for n in (2, 3, 4, 10, 11):
        t = tr.thin(n)
        keep = [i for i in range(10) if i % n == 0]
        assert np.array_equal(t.chains, x[:, keep, :]) and t.mass is tr.mass and t.stats is tr.stats
    with pytest.raises(ValueError):
        tr.thin(0)
    assert list(inspect.signature(R.Trace.predict).parameters)[:3] == ["self", "requirements_rir", "n_requirements"]
    assert list(inspect.signature(R.Sampler.predict).parameters) == ["self", "predictor", "first", "count", "thin", "to_host", "diagnostics"]
    assert list(inspect.signature(R.predict_device).parameters)[:9] == ["predictor", "ptr", "chains", "iterations", "nvars", "device", "first", "count", "thin"]
    assert list(inspect.signature(R.Predictor.__init__).parameters)[:4] == ["self", "requirements_rir", "device", "math_mode"]
    assert callable(distributed.Comm.predict) and callable(R.Predictor.close)
