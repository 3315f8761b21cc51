"""Times leave-one-out predictive quantiles, CRPS and spread on the device (rh_loo_quantile_device: the pooled sort and Pareto fit of
every log-likelihood column, the draws' weights, the sort of the (value, weight) pairs, the scan) against the only route there was
for the same answer: the two matrices copied to the host and, pair by pair, numpy's lexsort and cumsum
(tests/test_loo_quantile_device_cpu.py's restatement, in longdouble, with tests/test_loo_expect_device_cpu.py's weights).  Shapes:
KidIQ's at the bench's chain count, 1024 chains x 200 draws x 434 observations with three probabilities, a log-likelihood buffer and
a buffer of replicated observations (711 MB each), made on the host in blocks of 64 chains with seeds of their own and uploaded once;
and a narrow one, 64 chains x 2000 draws x 8.  One process; every figure -- device call, plain-mode call, copy, numpy -- is one warm
call, then 5 repetitions: the median and all five.  The numpy route is timed over the first 8 pairs and scaled to all of them (it is
a loop over the pairs); the figure says so.  Prints one JSON line.

    python tools/loo_quantile_device_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from tests.test_loo_quantile_device_cpu import restate  # noqa: E402
from tools.loo_expect_device_timing import block, hip, median5, BLOCK  # noqa: E402

PROBS = (0.05, 0.5, 0.95)


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
    call = lambda sel: R.loo_quantile_device(pl.value, pv.value, m, n, k, k, sel, sel, probs=PROBS, y=y[sel], device=0)
    plain = lambda sel: R.loo_quantile_device(None, pv.value, m, n, 0, k, None, sel, probs=PROBS, y=y[sel], device=0)
    back_l, back_v = np.empty((m, n, k)), np.empty((m, n, k))
    copy, copy_all = median5(lambda: (hip.hipMemcpy(back_l.ctypes.data_as(C.c_void_p), pl, nbytes, 2), hip.hipMemcpy(back_v.ctypes.data_as(C.c_void_p), pv, nbytes, 2)))
    dev, dev_all = median5(lambda: call(cols))
    pln, pln_all = median5(lambda: plain(cols))
    one, _ = median5(lambda: call([0]))
    got = call(cols)

    def host_pair(p):
        e = restate(back_l[:, :, p].reshape(-1), back_v[:, :, p].reshape(-1), False)
        return [float(e.quantile(q)) for q in PROBS] + list(e.scores(float(y[p])))
    res = []
    host, host_all = median5(lambda: res.append([host_pair(p) for p in range(host_pairs)]))
    for p, want in enumerate(res[-1]):
        have = list(got.quantiles[p]) + [got.crps[p], got.spread[p]]
        assert np.allclose(have, want, rtol=1e-8, atol=1e-10), (name, p, have, want)
    S = m * n
    out = {"shape": name, "chains": m, "iterations": n, "pairs": k, "S": S, "probs": list(PROBS), "ll_bytes": nbytes, "val_bytes": nbytes,
           "workspace_bytes_per_pair": 32 * S + 8 * int(np.max(got.tail_n)), "tail_n": int(got.tail_n[0]), "host_copy_s_median5": copy, "host_copy_s_all": copy_all,
           "device_s_median5": dev, "device_s_all": dev_all, "device_plain_mode_s_median5": pln, "device_plain_mode_s_all": pln_all, "device_one_pair_s_median5": one,
           "host_numpy_pairs_timed": host_pairs, "host_numpy_s_median5": host, "host_numpy_s_all": host_all, "host_numpy_s_scaled_to_all_pairs": host * k / host_pairs,
           "crps_mean": float(np.mean(got.crps)), "spread_mean": float(np.mean(got.spread)), "pareto_k_max": float(np.max(got.pareto_k)),
           "pareto_k_above_0.7": int(np.sum(got.pareto_k > 0.7))}
    out["host_route_s"] = copy + out["host_numpy_s_scaled_to_all_pairs"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / dev
    hip.hipFree(pl); hip.hipFree(pv)
    return out


if __name__ == "__main__":
    which = sys.argv[1:] or ["kidiq", "narrow"]
    res = []
    if "narrow" in which:
        res.append(shape("narrow_64x2000x8", 64, 2000, 8, 8))
    if "kidiq" in which:
        res.append(shape("kidiq_1024x200x434", 1024, 200, 434, 8))
    print(json.dumps(res))
