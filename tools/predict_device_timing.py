"""Times Trace.predict on the device (rh_predict_device, csrc/device/rh_predict.hip.h) against the only route there was before it
-- the draws copied to the host, then rh_requirements_eval (upload, one thread per draw, download) -- at the shapes of cfg 2
(1024 chains x 1000 iterations x 5 parameters, funnel_predict(5)) and of the big-mode tests (256 x 40 x 704: 4 of the parameters,
and all of them).  One process; per figure one warm call, then the median of 5.  The buffers are synthetic normal draws uploaded
once.  Prints one JSON line.

    python tools/predict_device_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from rainier_amd import _capi, models  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
HBM_PEAK = 8.0e12        # bytes / s, MI355X


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def shape(name, rir, nreq, nref, m, n, k):
    x = np.random.default_rng(3).normal(size=(m, n, k)) * 0.5
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), x.nbytes) == 0
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    p = R.Predictor(rir, device=0)
    # the kernel and the wait for it (results stay on the device), and the same with the results copied to the host
    dev, dev_all = median5(lambda: R.predict_device(p, ptr.value, m, n, k, device=0, to_host=False))
    dev_host, _ = median5(lambda: R.predict_device(p, ptr.value, m, n, k, device=0))
    back = np.empty_like(x)

    def host_route():
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, x.nbytes, 2) == 0          # what rh_sampler_draws does
        return R.predict(rir, back, nreq, device=0)
    host, host_all = median5(host_route)
    same = bool(np.array_equal(R.predict_device(p, ptr.value, m, n, k, device=0), host_route()))
    p.close(); hip.hipFree(ptr)
    moved = m * n * (nref + nreq) * 8.0           # the doubles that must cross HBM once: referenced parameters in, results out
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "nref": nref, "nreq": nreq, "device_s_median5": dev, "device_s_all": dev_all,
            "device_with_copy_to_host_s": dev_host, "host_route_s_median5": host, "host_route_s_all": host_all, "same_bits": same,
            "needed_bytes": moved, "achieved_bytes_per_s": moved / dev, "hbm_frac": moved / dev / HBM_PEAK}


def main():
    out = []
    rir, nreq = models.funnel_predict(5)
    out.append(shape("cfg2 1024x1000x5 funnel_predict(5)", rir, nreq, 5, 1024, 1000, 5))
    rir, nreq = models.sparse_predict(704)
    out.append(shape("256x40x704 sparse (4 of 704)", rir, nreq, 4, 256, 40, 704))
    rir, nreq = models.dense_predict(704)
    out.append(shape("256x40x704 dense (704 of 704)", rir, nreq, 704, 256, 40, 704))
    print(json.dumps({"predict_device_timing": out, "compiles": int(_capi.lib().rh_compile_count())}))


if __name__ == "__main__":
    main()
