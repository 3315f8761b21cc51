"""Times the joint convergence diagnostics on the device (rh_joint_diagnostics_device: batch means, three Gram matrices of centred
rows on the fp64 matrix cores, the K x K finish on the host) against what there was before it for the same answer: the draws copied
to the host and a numpy restatement (matrix products for the three Grams, slogdet, eigvalsh).  Shapes: cfg 2's (1024 chains x 1000
iterations x 5 parameters), 1024 x 400 x 160 and 256 x 40 x 256.  One process; every figure is one warm call, then the median of 5.
The buffers are synthetic AR(1) draws: 16 distinct chains generated on the host and uploaded chains / 16 times, each copy with an
offset of its own so that the between-chain matrix has full rank.  The host finish on its own: the call with mess and mpsrf asked for
less the call without them (the matrices are computed and copied either way).  Beside the times: the bytes each pass asks for (by the
kernels' own arithmetic, not counters).  Prints one JSON line.

    python tools/joint_device_timing.py
"""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from rainier_amd import _capi  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
SPLIT, TC = 4096, 64                    # RC_SPLIT, RC_TC (csrc/device/rh_cov.hip.h)


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def host_route(x):
    """the same figures in numpy (float64) from the draws on the host"""
    c, n0, k = x.shape
    b = math.isqrt(n0)
    a = n0 // b
    n = a * b
    u = x[:, n0 - n:, :]
    m, mu, y = u.mean(1), u.reshape(-1, k).mean(0), u.reshape(c, a, b, k).mean(2)
    dw, ds, db = (u - m[:, None, :]).reshape(-1, k), (y - mu).reshape(-1, k), m - mu
    gw, gb = dw.T @ dw, db.T @ db
    w, bn, sig, lam = gw / (c * (n - 1)), gb / (c - 1), b * (ds.T @ ds) / (c * a - 1), (gw + n * gb) / (c * n - 1)
    mess = c * n * math.exp((np.linalg.slogdet(lam)[1] - np.linalg.slogdet(sig)[1]) / k)
    li = np.linalg.inv(np.linalg.cholesky(w))
    return mess, math.sqrt((n - 1) / n + (c + 1) / c * np.linalg.eigvalsh(li @ bn @ li.T)[-1])


def shape(name, m, n, k):
    rng = np.random.default_rng(1)
    blk = rng.standard_normal((16, n, k))
    for i in range(1, n):
        blk[:, i, :] += 0.5 * blk[:, i - 1, :]
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // 16):
        part = blk + 0.05 * rng.standard_normal((16, 1, k))
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * part.nbytes), part.ctypes.data_as(C.c_void_p), part.nbytes, 1) == 0
    res = {}

    def device():
        res["dev"] = R.joint_diagnostics_device(ptr.value, m, n, k, device=0)
    dev, dev_all = median5(device)
    mats, scal = np.zeros((4, k, k)), np.zeros(2)

    def raw(scalars):      # the C call itself, with and without the two scalars that need the host finish
        out = [_capi.dptr(scal[0:1]), _capi.dptr(scal[1:2])] if scalars else [None, None]
        _capi.check(_capi.lib().rh_joint_diagnostics_device(ptr, 0, m, n, k, 0, n, 0, None, 0, *out, None, None, *[_capi.dptr(mats[q]) for q in range(4)], None))
    with_finish, _ = median5(lambda: raw(True))
    without_finish, _ = median5(lambda: raw(False))
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    host, host_all = median5(lambda: res.__setitem__("host", host_route(back)))
    hip.hipFree(ptr)
    d = res["dev"]
    N, ca, draws = m * d.batch * d.batches, m * d.batches, m * n * k * 8
    T = -(-k // TC)
    pairs, splits = T * (T + 1) // 2, [-(-r // SPLIT) for r in (N, ca, m)]
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "batch": d.batch, "batches": d.batches, "N": N, "draws_bytes": draws,
            "tile_pairs": pairs, "splits_within_sigma_between": splits, "mess": d.mess, "mpsrf": d.mpsrf, "host_route_mess_mpsrf": res["host"],
            "device_s_median5": dev, "device_s_all": dev_all, "c_call_with_scalars_s": with_finish, "c_call_without_scalars_s": without_finish,
            "host_finish_s_by_difference": with_finish - without_finish,
            "bytes": {"batch_pass_reads": N * k * 8, "batch_pass_writes": (ca + 2 * m) * k * 8, "within_gram_reads": N * TC * 8 * T * T,
                      "sigma_gram_reads": ca * TC * 8 * T * T, "between_gram_reads": m * TC * 8 * T * T,
                      "partials_written_and_read": 2 * pairs * sum(splits) * TC * TC * 8, "matrices_written_and_copied": 2 * 4 * 8 * k * k},
            "host_copy_s_median5": copy, "host_numpy_s_median5": host, "host_numpy_s_all": host_all, "host_route_s": copy + host,
            "host_route_bytes_over_the_link": draws}


if __name__ == "__main__":
    print(json.dumps([shape(*s) for s in [("cfg2", 1024, 1000, 5), ("1024x400x160", 1024, 400, 160), ("256x40x256", 256, 40, 256)]]))
