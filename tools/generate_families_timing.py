"""Times the count families and the composites of posterior-predictive sampling on the device (rh_generate_device through
rh_generate_ext_kernel, csrc/device/rh_generate_ext.hip.h): 1024 chains x 200 kept draws x 434 outputs per table -- Binomial in each
of its three branches, NegativeBinomial's exact path at n = 50, ZeroInflated(Poisson) -- over a parameter buffer that is already on
the device, samples left there.  For comparison, in the same process: rh_generate_kernel's Poisson table of the same shape, and
the route there was before -- the parameters copied to the host and modeling.py's generate in a Python loop -- on 1/100 of the rows,
scaled up.  There is no earlier device route and no speed bar.  Also reports what the code object says.  Per device figure one warm
call, then the median of 5.  Prints one JSON line.

    python tools/generate_families_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from rainier_amd import _capi, gen, modeling  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
CHAINS, KEPT, NOUT, NIN, SEED = 1024, 200, 434, 6, 20240607
P_SMALL, P_MID, P_HIGH, PSI, LAM = 0, 1, 2, 3, 5    # columns; PSI + 1 holds 1 - psi


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def parameters():
    rng = np.random.default_rng(3)
    n = CHAINS * KEPT
    x = np.empty((n, NIN))
    x[:, P_SMALL] = rng.uniform(0.005, 0.045, size=n)    # k = 200: k p <= 10, the Poisson branch
    x[:, P_MID] = rng.uniform(0.2, 0.8, size=n)          # k = 200: the normal branch; k = 50: the exact one
    x[:, P_HIGH] = rng.uniform(0.96, 0.99, size=n)       # k = 200: k (1 - p) < 9, the exact branch at 200 trials
    x[:, PSI] = rng.uniform(0.1, 0.6, size=n)
    x[:, PSI + 1] = 1 - x[:, PSI]
    x[:, LAM] = rng.choice([0.5, 5.0, 29.0, 100.0], size=n)
    return x.reshape(CHAINS, KEPT, NIN)


def host_route(x, dist_of, ptr):
    """the copy of the parameters to the host and modeling.py's generate, one draw at a time, on every 100th row; scaled by 100"""
    back = np.empty_like(x)
    t0 = time.perf_counter()
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, x.nbytes, 2) == 0
    copy_s = time.perf_counter() - t0
    rng = modeling.JavaRandom(SEED)
    rows = back.reshape(-1, NIN)[::100]
    t0 = time.perf_counter()
    for row in rows:
        d = dist_of(row)
        for _ in range(NOUT):
            d.generate(rng)
    loop_s = time.perf_counter() - t0
    return {"copy_s": copy_s, "loop_rows": int(rows.shape[0]), "loop_s": loop_s, "host_s_scaled": copy_s + loop_s * (x.shape[0] * x.shape[1] / rows.shape[0])}


def table(name, op, x, ptr, dist_of=None):
    ops = [op] * NOUT
    g = R.Generator(ops, nin=NIN, device=0)
    assert g.nout == NOUT
    dev, dev_all = median5(lambda: R.generate_device(g, ptr.value, CHAINS, KEPT, NIN, SEED, device=0, to_host=False))
    out = {"table": name, "chains": CHAINS, "kept": KEPT, "nout": NOUT, "flags": g.flags, "device_s_median5": dev, "device_s_all": dev_all,
           "samples_per_s": CHAINS * KEPT * NOUT / dev}
    g.close()
    if dist_of is not None:
        out["host"] = host_route(x, dist_of, ptr)
    return out


def main():
    c = gen.col
    x = parameters()
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), x.nbytes) == 0
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    M = modeling
    out = [table("Binomial(p, 200), k p <= 10: Poisson branch", gen.Binomial(c(P_SMALL), 200.0), x, ptr, lambda r: M.Binomial(r[P_SMALL], 200.0)),
           table("Binomial(p, 200), normal branch", gen.Binomial(c(P_MID), 200.0), x, ptr),
           table("Binomial(p, 200), k (1 - p) < 9: exact, 200 trials", gen.Binomial(c(P_HIGH), 200.0), x, ptr),
           table("Binomial(p, 50): exact, 50 trials", gen.Binomial(c(P_MID), 50.0), x, ptr, lambda r: M.Binomial(r[P_MID], 50.0)),
           table("NegativeBinomial(p, 50): exact, 50 trials", gen.NegativeBinomial(c(P_MID), 50.0), x, ptr, lambda r: M.NegativeBinomial(r[P_MID], 50.0)),
           table("ZeroInflated(Poisson(lambda))", gen.ZeroInflated(PSI, gen.Poisson(c(LAM))), x, ptr),
           table("Poisson(lambda) through rh_generate_kernel", gen.Poisson(c(LAM)), x, ptr, lambda r: M.Poisson(r[LAM]))]
    hip.hipFree(ptr)
    keys = ("vgprs", "sgprs", "vgpr_spills", "sgpr_spills", "scratch")
    ext = _capi.code_object_report(_capi.generate_ext_lower_only())[("object", "rh_generate_ext_kernel")]
    old = _capi.code_object_report(_capi.generate_lower_only())[("object", "rh_generate_kernel")]
    print(json.dumps({"generate_families_timing": out, "rh_generate_ext_kernel": {k: ext[k] for k in keys}, "rh_generate_kernel": {k: old[k] for k in keys},
                      "compiles": int(_capi.lib().rh_compile_count())}))


if __name__ == "__main__":
    main()
