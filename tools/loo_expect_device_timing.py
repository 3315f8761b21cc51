"""Times PSIS leave-one-out expectations on the device (rh_loo_expect_device: the pooled sort of every log-likelihood column, the
Pareto fit of the tail, the draws' weights, the weighted sums) against the only route there was for the same answer: the
log-likelihood and value matrices copied to the host and the contract restated in numpy, pair by pair
(tests/test_loo_expect_device_cpu.py's restate_pair, in longdouble).  Shape: KidIQ's at the bench's chain count, 1024 chains x 200
draws x 434 observations, a log-likelihood buffer and a buffer of replicated observations (711 MB each), made on the host in blocks
of 64 chains with seeds of their own and uploaded once.  One process; every figure -- device call, copy, numpy -- is one warm call,
then 5 repetitions: the median and all five.  The numpy route is timed over the first 8 pairs and scaled to 434 (it is a loop over
the pairs); the figure says so.  Prints one JSON line.

    python tools/loo_expect_device_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from tests.test_loo_expect_device_cpu import restate_pair  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
BLOCK = 64


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def block(n, k, seed):
    """BLOCK chains x n x k log-likelihoods and replicated observations: observation i is y_i = c_i against N(theta, s_i^2) over
    theta ~ N(0, 1), the c_i spread over (-1.5, 1.5) and the s_i over (1, 3) (tools/loo_device_timing.py's buffer: Pareto k from about
    0.1 to beyond 0.7); y_rep = theta + s_i N(0, 1)"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((BLOCK, n, k))
    c, s = np.linspace(-1.5, 1.5, k), 1.0 + 2.0 * ((np.arange(k) * 7) % k) / k
    return np.ascontiguousarray(-0.5 * ((t - c) / s) ** 2 - np.log(s)), np.ascontiguousarray(t + s * rng.standard_normal((BLOCK, n, k)))


def shape(name, m, n, k, host_pairs):
    pl, pv = C.c_void_p(), C.c_void_p()
    nbytes = m * n * k * 8
    assert hip.hipMalloc(C.byref(pl), nbytes) == 0 and hip.hipMalloc(C.byref(pv), nbytes) == 0
    for r in range(m // BLOCK):
        bl, bv = block(n, k, 100 + r)
        for ptr, blk in ((pl, bl), (pv, bv)):
            assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    y = np.linspace(-1.5, 1.5, k)
    cols = list(range(k))
    call = lambda sel: R.loo_expect_device(pl.value, pv.value, m, n, k, k, sel, sel, y=y[sel], device=0)
    back_l, back_v = np.empty((m, n, k)), np.empty((m, n, k))
    copy, copy_all = median5(lambda: (hip.hipMemcpy(back_l.ctypes.data_as(C.c_void_p), pl, nbytes, 2), hip.hipMemcpy(back_v.ctypes.data_as(C.c_void_p), pv, nbytes, 2)))
    dev, dev_all = median5(lambda: call(cols))
    one, _ = median5(lambda: call([0]))
    got = call(cols)
    res = []
    host, host_all = median5(lambda: res.append([restate_pair(back_l[:, :, p].reshape(-1), back_v[:, :, p].reshape(-1), float(y[p])) for p in range(host_pairs)]))
    for p, want in enumerate(res[-1]):
        have = [getattr(got, f)[p] for f in ("mean", "var", "pit", "pit_lt", "ess", "pareto_k", "tail_n")]
        assert np.allclose(have, [want[f] for f in ("mean", "var", "pit", "pit_lt", "ess", "pareto_k", "tail_n")], rtol=1e-9, atol=1e-12), (name, p, have, want)
    S = m * n
    out = {"shape": name, "chains": m, "iterations": n, "pairs": k, "S": S, "ll_bytes": nbytes, "val_bytes": nbytes, "workspace_bytes_per_pair": 16 * S + 8 * int(np.max(got.tail_n)),
           "tail_n": int(got.tail_n[0]), "host_copy_s_median5": copy, "host_copy_s_all": copy_all, "device_s_median5": dev, "device_s_all": dev_all,
           "device_one_pair_s_median5": one, "host_numpy_pairs_timed": host_pairs, "host_numpy_s_median5": host, "host_numpy_s_all": host_all,
           "host_numpy_s_scaled_to_all_pairs": host * k / host_pairs, "pit_min": float(np.min(got.pit)), "pit_max": float(np.max(got.pit)),
           "ess_min": float(np.min(got.ess)), "ess_median": float(np.median(got.ess)), "pareto_k_min": float(np.min(got.pareto_k)),
           "pareto_k_max": float(np.max(got.pareto_k)), "pareto_k_above_0.7": int(np.sum(got.pareto_k > 0.7))}
    out["host_route_s"] = copy + out["host_numpy_s_scaled_to_all_pairs"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / dev
    hip.hipFree(pl); hip.hipFree(pv)
    return out


if __name__ == "__main__":
    print(json.dumps([shape("kidiq_1024x200x434", 1024, 200, 434, 8)]))
