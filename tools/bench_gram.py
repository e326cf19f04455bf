"""Timing of the exact Gram's product paths at the bench shape (interleaved in
one process, random integer data in [-qmax, qmax]): `rm` the row-major panel
through grid_knn_gram, `kb` the K-blocked panel through grid_knn_gram_kb.
Every path's Gram is checked against the float64 product.

    python tools/bench_gram.py [--n 3202] [--k 2700000] [--reps 3] [--paths rm,kb:LAG=2:KC=9]

--pad 128 pads the rows to a multiple of 128 only: where that is no multiple
of 256 (e.g. --n 3100), `rm` runs k_gram_dma instead of k_gram8.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grid_amd import _abi  # noqa: E402

KNOBS = ("LAG", "SPIN", "KC", "KX")          # performance knobs (results are exact for any value)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3202)
ap.add_argument("--k", type=int, default=2_700_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--paths", default="rm,kb", help="comma-separated rm | kb, each with optional :KEY=VAL knobs "
                                                 "(GRID_GRAM_ + " + ", ".join(KNOBS) + ")")
ap.add_argument("--qmax", type=int, default=200)
ap.add_argument("--pad", type=int, default=256, choices=(128, 256), help="row padding")
ap.add_argument("--ld-extra", type=int, default=0, help="extra bf16 columns of row padding (row stride)")
a = ap.parse_args()

paths = a.paths.split(",")
for pp in paths:
    p, *knobs = pp.split(":")
    if p not in ("rm", "kb") or any(kv.split("=")[0] not in KNOBS for kv in knobs):
        sys.exit(f"bad path {pp!r}: rm or kb, knobs {KNOBS}")
np_ = -(-a.n // a.pad) * a.pad
if np_ % 256 and any(pp.startswith("kb") for pp in paths):
    sys.exit(f"kb needs np % 256 == 0 (np = {np_})")
kpad = -(-a.k // 64) * 64
dev = _abi.Device(0)
dev.set_stream(torch.cuda.current_stream())
g = torch.Generator(device="cuda").manual_seed(1)
ld = kpad + a.ld_extra
zb = torch.zeros((np_, ld), dtype=torch.int16, device="cuda")
for r0 in range(0, a.n, 256):
    r1 = min(a.n, r0 + 256)
    zi = torch.randint(-a.qmax, a.qmax + 1, (r1 - r0, kpad), device="cuda", dtype=torch.int32, generator=g)
    zb[r0:r1, :kpad] = zi.to(torch.bfloat16).view(torch.int16)
    del zi
gram = torch.zeros((np_, np_), dtype=torch.int64, device="cuda")
zbb = None
if any(pp.startswith("kb") for pp in paths):   # K-blocked [kpad/KBW][np][KBW]
    zbb = zb[:, :kpad].reshape(np_, kpad // _abi.KBW, _abi.KBW).permute(1, 0, 2).contiguous()
res = {}
first = None
flops = 2.0 * a.n * a.n * a.k
for rep in range(a.reps):
    for pp in paths:
        p, *knobs = pp.split(":")
        for kv in KNOBS:
            os.environ.pop("GRID_GRAM_" + kv, None)
        for kv in knobs:
            key, val = kv.split("=")
            os.environ["GRID_GRAM_" + key] = val
        gram.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if p == "kb":
            _abi.call("grid_knn_gram_kb", dev.ctx, zbb.data_ptr(), np_, kpad, a.qmax, gram.data_ptr())
        else:
            _abi.call("grid_knn_gram", dev.ctx, zb.data_ptr(), np_, kpad, ld, a.qmax, gram.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        res.setdefault(pp, []).append(ms)
        if rep == 0:
            # check a few upper-triangle tiles against a float64 product on the GPU
            zz = zb[:256, :kpad].view(torch.bfloat16).double()
            ref = (zz @ zz.T).long()
            ok = torch.equal(gram[:128, :256], ref[:128, :256])
            # every path's whole Gram (upper tiles) against the first path's
            if first is None:
                first = gram.clone()
                same = True
            else:
                same = torch.equal(gram, first)
            print(f"path {pp}: tile check {'OK' if ok else 'MISMATCH'}, "
                  f"whole Gram {'equal to' if same else 'DIFFERENT from'} the first path", flush=True)
for v, t in res.items():
    ms = min(t)
    print(f"path {v}: min {ms:.2f} ms  median {np.median(t):.2f} ms  "
          f"-> {flops / ms / 1e9:.0f} TFLOP/s (2N^2K), {flops / ms / 1e9 / 2516.6 * 100:.1f}% of bf16 peak",
          flush=True)
