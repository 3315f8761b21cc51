"""What the tick engine's rounds look like on the device's timeline: reads the kernel trace of a bench run taken with
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps STEPS --warmup W` and writes, for the timed
region (the last 2 x STEPS x LEAPFROG gradient launches: two lanes), the no-kernel gaps (those above 100 us are the seams between
rounds), how far lane 1's first gradient launch of a round lags lane 0's, how many gradient launches ran with no launch of the
other lane beside them, and for how long one lane's / both lanes' gradient launches were running (profiles/round_seams_cfg2).
usage: trace_seams.py DIR STEPS LEAPFROG OUT.json"""
import csv
import glob
import json
import os
import sys
from collections import Counter, defaultdict

d, steps, leap, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
best = None
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    rows = list(csv.DictReader(open(f)))
    n = sum(1 for r in rows if "rh_grad" in r.get("Kernel_Name", ""))
    if best is None or n > best[0]:
        best = (n, f, rows)
assert best and best[0] > 0, "no kernel trace with gradient launches under " + d
_, f, rows = best
cols = list(rows[0].keys())
K = []
for r in rows:
    K.append(dict(name=r["Kernel_Name"], t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"]),
                  key=(r.get("Queue_Id", ""), r.get("Stream_Id", ""))))
K.sort(key=lambda k: k["t0"])
grads = [k for k in K if "rh_grad" in k["name"]]
per_name = defaultdict(list)
for k in K:
    per_name[k["name"].split("(")[0]].append(k["t1"] - k["t0"])
want = 2 * steps * leap
timed = grads[-want:]
res = {"file": os.path.basename(f), "columns": cols, "kernels_in_trace": len(K), "grad_launches_in_trace": len(grads),
       "timed_grad_launches_taken": len(timed),
       "kernel_stats_us": {n: {"calls": len(v), "mean": sum(v) / len(v) / 1e3, "total_ms": sum(v) / 1e6} for n, v in sorted(per_name.items())}}
keys = Counter(k["key"] for k in timed)
res["lane_keys"] = {str(k): v for k, v in keys.items()}
lanes = [k for k, _ in keys.most_common(2)]
w0, w1 = timed[0]["t0"], max(k["t1"] for k in timed)
res["window_ms"] = (w1 - w0) / 1e6
inwin = [k for k in K if k["t1"] > w0 and k["t0"] < w1]
# no-kernel gaps inside the window
gaps, end = [], w0
for k in sorted(inwin, key=lambda k: k["t0"]):
    if k["t0"] > end:
        gaps.append((end, k["t0"]))
    end = max(end, k["t1"])
big = [(a, b) for a, b in gaps if b - a > 100_000]
res["no_kernel_gaps"] = {"count": len(gaps), "total_ms": sum(b - a for a, b in gaps) / 1e6,
                         "over_100us": {"count": len(big), "total_ms": sum(b - a for a, b in big) / 1e6,
                                        "each_us": [round((b - a) / 1e3, 1) for a, b in big]},
                         "under_100us_total_ms": sum(b - a for a, b in gaps if b - a <= 100_000) / 1e6}
# rounds: the stretches between the big gaps; lane 1's first gradient launch against lane 0's
if len(lanes) == 2:
    cuts = [w0] + [b for _, b in big] + [w1 + 1]
    lags = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        first = {}
        for k in timed:
            if a <= k["t0"] < b and k["key"] not in first:
                first[k["key"]] = k
        if len(first) == 2:
            ks = sorted(first.values(), key=lambda k: k["t0"])
            lags.append({"round_ms": (b - a) / 1e6, "second_lane_first_launch_lag_us": (ks[1]["t0"] - ks[0]["t0"]) / 1e3,
                         "first_launch_us": (ks[0]["t1"] - ks[0]["t0"]) / 1e3,
                         "grad_launches": sum(1 for k in timed if a <= k["t0"] < b)})
    res["rounds"] = lags
    # launches that ran with no launch of the other lane beside them at any time, and the time a gradient launch ran alone
    A = [k for k in timed if k["key"] == lanes[0]]
    B = [k for k in timed if k["key"] == lanes[1]]

    def alone(xs, ys):
        n, j = 0, 0
        for x in xs:
            while j < len(ys) and ys[j]["t1"] <= x["t0"]:
                j += 1
            if j >= len(ys) or ys[j]["t0"] >= x["t1"]:
                n += 1
        return n
    na, nb = alone(A, B), alone(B, A)
    res["launches_with_no_overlap"] = {"lane0": na, "lane1": nb, "of": len(timed), "share": (na + nb) / len(timed)}
    ev = []
    for k in timed:
        ev.append((k["t0"], 1)); ev.append((k["t1"], -1))
    ev.sort()
    open_, prev, solo, both = 0, w0, 0, 0
    for t, s in ev:
        if open_ == 1:
            solo += t - prev
        elif open_ >= 2:
            both += t - prev
        prev = t
        open_ += s
    res["grad_time_ms"] = {"one_lane_only": solo / 1e6, "both_lanes": both / 1e6, "none": (w1 - w0 - solo - both) / 1e6}
    res["mean_grad_launch_us"] = sum(k["t1"] - k["t0"] for k in timed) / len(timed) / 1e3
else:
    res["note"] = "the gradient launches of the timed region carry one queue/stream key only: lanes cannot be told apart"
json.dump(res, open(out, "w"), indent=1)
print(json.dumps({k: res[k] for k in res if k not in ("columns", "kernel_stats_us")})[:3000])
