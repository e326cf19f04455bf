"""BASELINE config 5, step 6: dipCN of every region of a loci table in one
batched launch (engine.dipcn_loci -> grid_dipcn_loci) against the per-locus
path (one engine.dipcn call per region, which uploads the shared neighbour
arrays every time).

Synthetic inputs: ``--samples`` rows with ``--list`` random neighbours each, scales ~ U(0.8, 1.25), integer counts with ``--absent`` of
the (sample, locus) cells missing.  Both paths are timed on the same host
arrays, upload + launch + download; the outputs of the per-locus calls are
checked against the batched ones bit for bit.  Prints one JSON line.

    python tools/bench_dipcn_loci.py [--loci 734] [--samples 50000] [--list 500] [--n-nbr 300]
                                     [--per-locus-calls N]   (default: every locus)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grid_amd import _abi, engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--loci", type=int, default=734)
ap.add_argument("--samples", type=int, default=50000)
ap.add_argument("--list", type=int, default=500)
ap.add_argument("--n-nbr", type=int, default=300)
ap.add_argument("--absent", type=float, default=0.03)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--per-locus-calls", type=int, default=-1, help="time this many engine.dipcn calls (-1: all loci)")
a = ap.parse_args()

rng = np.random.default_rng(20261021)
n, k, nl = a.samples, a.list, a.loci
t0 = time.perf_counter()
nbr = rng.integers(0, n, (n, k)).astype(np.int32)
scale = rng.uniform(0.8, 1.25, n)
nsc = scale[nbr]
cnt = np.full(n, k, np.int32)
ldl = -(-nl // 8) * 8
reads = np.full((n, ldl), np.nan)
reads[:, :nl] = rng.integers(20, 2000, (n, nl))
reads[:, :nl][rng.random((n, nl)) < a.absent] = np.nan
gen_s = time.perf_counter() - t0

dev = _abi.Device(0)
batched, res = [], None
for _ in range(a.reps + 1):                     # first call: warm-up
    t1 = time.perf_counter()
    res = engine.dipcn_loci(dev, reads, scale, nbr, nsc, cnt, a.n_nbr, n)
    batched.append(time.perf_counter() - t1)
out, valid, zerodiv, missed = res

# the launch alone, on resident buffers
bufs = [dev.upload(x) for x in (reads, scale, nbr, nsc, cnt)]
d_out, d_valid = dev.alloc((n, ldl), np.float64), dev.alloc((n, ldl), np.uint8)
d_zd, d_miss = dev.alloc(nl, np.int32), dev.alloc((n, ldl), np.uint8)
kern_ms = []
for _ in range(a.reps + 1):
    dev.record(0)
    _abi.call("grid_dipcn_loci", dev.ctx, n, n, nl, ldl, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
              bufs[4].ptr, k, a.n_nbr, d_out.ptr, d_valid.ptr, d_zd.ptr, d_miss.ptr)
    dev.record(1)
    dev.sync()
    kern_ms.append(dev.elapsed_ms(0, 1))
for b in bufs + [d_out, d_valid, d_zd, d_miss]:
    b.free()

calls = nl if a.per_locus_calls < 0 else min(a.per_locus_calls, nl)
per, same = [], True
for col in range(calls):
    has = ~np.isnan(reads[:, col])
    rd = np.where(has, reads[:, col], 0.0)
    t2 = time.perf_counter()
    o1, v1 = engine.dipcn(dev, rd, has.astype(np.uint8), scale, nbr, nsc, cnt, a.n_nbr, n_rows=n)
    per.append(time.perf_counter() - t2)
    if (col + 1) % 100 == 0:
        print(f"per-locus path: {col + 1}/{calls} calls, {np.sum(per):.1f} s", file=sys.stderr, flush=True)
    same = same and np.array_equal(v1, valid[:, col]) and \
        np.array_equal(o1[v1].view(np.uint64), out[v1, col].view(np.uint64))
per_total = float(np.sum(per))
print(json.dumps({
    "metric": "s for step 6 over a loci table (config 5), batched launch", "value": min(batched[1:]), "unit": "s",
    "config": {"loci": nl, "samples": n, "list": k, "n_nbr": a.n_nbr, "absent": a.absent},
    "batched_s": min(batched[1:]), "batched_first_call_s": batched[0], "batched_all_s": batched,
    "kernel_ms": min(kern_ms[1:]), "kernel_first_ms": kern_ms[0],
    "per_locus_calls": calls, "per_locus_total_s": per_total,
    "per_locus_mean_s": per_total / max(calls, 1), "per_locus_scaled_to_all_loci_s": per_total / max(calls, 1) * nl,
    "speedup": (per_total / max(calls, 1) * nl) / min(batched[1:]),
    "outputs_equal": bool(same), "valid_fraction": float(valid.mean()), "zerodiv_loci": int(zerodiv.sum()),
    "missed_ids_mean": float(missed.mean()),
    "synthetic_generation_s": gen_s,
}), flush=True)
