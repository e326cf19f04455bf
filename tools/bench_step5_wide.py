"""Step 5's tail above 16 neighbours at W = 8, per rank, on one GPU: the two
bin-split routes of fused.Steps47 from the accumulated Gram to the neighbour
lists (idx_l) --

    allreduce     all-reduce of the whole Gram, mirror, every rank selects all n rows
    row_exchange  reduce-scatter of the segments, the transposed tiles' all-to-all,
                  every rank selects its own 2B rows, all-gather of the lists

through fused.SimComm(8, r) for r = 0 (blocks 0 and 15: the widest and the
narrowest segment) and r = 7 (blocks 7 and 8).  SimComm does each collective's
local memory work and counts the bytes the real one would bring into the rank
(bytes_in); the interconnect's time is NOT in these numbers.  The Gram is a
seeded random one: the tail reads nothing else.  The two routes alternate in
one process after a warm-up; times are device events (Steps47's stage marks),
reported as median and [min, max] over the repeats.

    python tools/bench_step5_wide.py [--sizes 3202,50000] [--k 500] [--json profiles/step5_wide_k500.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grid_amd import _abi  # noqa: E402
from grid_amd.fused import HipOps, SimComm, Steps47, TorchAlloc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="3202,50000")
ap.add_argument("--k", type=int, default=500)
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--ranks", default="0,7")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=0, help="timed runs per route (0: 20 below n = 20000, 7 above)")
ap.add_argument("--json", default="")
a = ap.parse_args()

W, M_LOCAL = a.world, 8192          # step 4's buffers are not under test: one 8192-bin block per rank
ROUTES = ("allreduce", "row_exchange")
dev = _abi.Device(0)
dev.set_stream(torch.cuda.current_stream())


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def one_rank(n, r, reps):
    chains = {}
    for route in ROUTES:
        comm = SimComm(W, r)
        st = Steps47(HipOps(dev), TorchAlloc(0), n, W * M_LOCAL, r * M_LOCAL, M_LOCAL, k=a.k, comm=comm,
                     step5_wide="allreduce" if route == "allreduce" else "auto")
        assert st.row_exchange == (route == "row_exchange") and st.full_rows == (route == "allreduce")
        chains[route] = (st, comm)
    # the accumulated Gram: off-diagonal cells below 2^20, the diagonal 2^30 (every d2 positive, 32 bits)
    g0 = chains[ROUTES[0]][0].gram
    torch.manual_seed(20260821 + n)
    g0.random_(0, 1 << 20)
    g0.view(-1)[: g0.shape[1] * g0.shape[1]: g0.shape[1] + 1] = 1 << 30
    chains[ROUTES[1]][0].gram.copy_(g0)
    total = {route: [] for route in ROUTES}
    stages = {route: {} for route in ROUTES}
    nbytes = {}
    for it in range(a.warmup + reps):
        for route in ROUTES:                      # alternate the routes
            st, comm = chains[route]
            comm.bytes_in = {}
            st.marks = []
            st._mark("start")
            st._step5()
            st._mark("topk")
            torch.cuda.synchronize()
            if it < a.warmup:
                continue
            ms = st.stage_ms()
            total[route].append(sum(ms.values()))
            for name, v in ms.items():
                stages[route].setdefault(name, []).append(v)
            nbytes[route] = dict(comm.bytes_in)
    st = chains["row_exchange"][0]
    out = {"rank": r, "B": st.B, "np": st.np_, "npw": st.npw}
    for route in ROUTES:
        out[route] = {"ms": spread(total[route]), "runs_ms": total[route],
                      "stage_ms": {name: float(np.median(v)) for name, v in stages[route].items()},
                      "bytes_in": nbytes[route], "bytes_in_total": int(sum(nbytes[route].values()))}
    out["row_exchange_below_allreduce_beyond_spread"] = out["row_exchange"]["ms"]["max"] < out["allreduce"]["ms"]["min"]
    return out


res = {"k": a.k, "world": W, "interconnect_time": "not measured (SimComm: local copies only)", "shapes": []}
for n in (int(x) for x in a.sizes.split(",")):
    reps = a.repeats or (20 if n < 20000 else 7)
    shape = {"n": n, "repeats": reps, "ranks": []}
    for r in (int(x) for x in a.ranks.split(",")):
        shape["ranks"].append(one_rank(n, r, reps))
        torch.cuda.empty_cache()
        print(json.dumps({"n": n, **shape["ranks"][-1]}), flush=True)
    res["shapes"].append(shape)
res["row_exchange_below_allreduce_everywhere"] = all(
    rk["row_exchange_below_allreduce_beyond_spread"] for s in res["shapes"] for rk in s["ranks"])
print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
