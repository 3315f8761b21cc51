"""Times posterior-predictive sampling on the device (rh_generate_device, csrc/device/rh_generate.hip.h): per shape the seconds of one
call over a parameter buffer that is already on the device (samples left there, and copied to the host) and the samples per
second.  There is no earlier device route to compare with and no speed bar: the only other route is a Python loop over
modeling.py's generate on the host.  Also reports what the code object says: VGPRs, SGPRs, and the tile and LDS bytes of each
shape's launch.  One process; per figure one warm call, then the median of 5.  Prints one JSON line.

    python tools/generate_device_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from rainier_amd import _capi, gen  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
TILE, SLAB = 256, 31     # RG_TILE, RG_SLAB (csrc/device/rh_generate.hip.h)


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def shape(name, ops, chains, kept):
    rng = np.random.default_rng(3)
    n = chains * kept
    x = np.stack([rng.normal(size=n), np.abs(rng.normal(size=n)) + 0.1, rng.choice([0.3, 1.3, 50.0], size=n),
                  rng.choice([0.5, 29.0, 1000.0], size=n), rng.uniform(0.05, 0.95, size=n)], axis=1).reshape(chains, kept, 5)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), x.nbytes) == 0
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    g = R.Generator(ops, nin=5, device=0)
    dev, dev_all = median5(lambda: R.generate_device(g, ptr.value, chains, kept, 5, 20240607, device=0, to_host=False))
    dev_host, _ = median5(lambda: R.generate_device(g, ptr.value, chains, kept, 5, 20240607, device=0))
    flags = g.flags
    g.close(); hip.hipFree(ptr)
    w = min(len(ops), SLAB)
    return {"shape": name, "chains": chains, "kept": kept, "nout": len(ops), "tile": TILE, "lds_bytes": 8 * TILE * (w | 1), "flags": flags,
            "device_s_median5": dev, "device_s_all": dev_all, "device_with_copy_to_host_s": dev_host, "samples_per_s": n * len(ops) / dev}


def main():
    c = gen.col
    mixed = [gen.Normal(c(0), c(1)), gen.Gamma(c(2), c(1)), gen.Poisson(c(3)), gen.Cauchy(c(0), c(1)), gen.Beta(c(2), 1.5), gen.Geometric(c(4)),
             gen.LogNormal(c(0), c(1))]
    rep = _capi.code_object_report(_capi.generate_lower_only())[("object", "rh_generate_kernel")]
    out = [shape("1024x1000 yhat ~ Normal(mu, sigma)", [gen.Normal(c(0), c(1))], 1024, 1000),
           shape("1024x1000 seven families", mixed, 1024, 1000),
           shape("1024x1000 Poisson(lambda), both branches", [gen.Poisson(c(3))], 1024, 1000),
           shape("256x40 thirty-two ops (two slabs)", (mixed * 5)[:32], 256, 40)]
    print(json.dumps({"generate_device_timing": out, "kernel": {k: rep[k] for k in ("vgprs", "sgprs", "vgpr_spills", "sgpr_spills", "scratch")},
                      "compiles": int(_capi.lib().rh_compile_count())}))


if __name__ == "__main__":
    main()
