"""Region coverage of a loci table over a mosdepth cohort: the device step
(grid_amd/utils/coverage_device.py) timed on every file, the host restatement
(grid_amd/utils/mosdepth.py region_coverages, the reference's per-line Python
semantics with one walk per file instead of one per region) timed on a SAMPLE
of the files and SCALED to the cohort -- the scaled figure is an estimate and
is labelled so.

    python tools/bench_cover.py [--data /dev/shm/grid_e2e] [--samples 3202] [--bins 3000000] [--bgzf]
                                [--loci tests/golden/loci/734_...uniq.txt] [--host-files 2]
                                [--json bench_outputs/bench_cover.json]

The cohort is tools/e2e_files.py's (tools/gen_cohort: BASELINE config 2 is
3,202 files x 3 M bins of 1 kb, every line on "chr1" over 3 Gb); it is
generated into --data when it is not there.  The synthetic cohort has ONE
chromosome, so every region of the table is placed on it at its own
coordinates (``--keep-chrom`` keeps the table's names: then no line matches
and only read + inflate + parse are timed).  The device result of the host
sample's files is compared with the restatement's, cell by cell.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--data", default="/dev/shm/grid_e2e")
ap.add_argument("--samples", type=int, default=3202)
ap.add_argument("--bins", type=int, default=3_000_000)
ap.add_argument("--bgzf", action="store_true", help="BGZF files (what mosdepth writes) when the cohort is generated")
ap.add_argument("--gen-threads", type=int, default=16)
ap.add_argument("--loci", default=os.path.join(ROOT, "tests", "golden", "loci",
                                               "734_possible_coding_vntr_regions.IBD2R_gt_0.25.uniq.txt"))
ap.add_argument("--keep-chrom", action="store_true")
ap.add_argument("--host-files", type=int, default=2, help="files the host restatement is timed on")
ap.add_argument("--batch-files", type=int, default=None)
ap.add_argument("--repeat", type=int, default=1, help="device runs (the first includes the buffers' allocation)")
ap.add_argument("--json", default=os.path.join(ROOT, "bench_outputs", "bench_cover.json"))
a = ap.parse_args()

mos = os.path.join(a.data, "mosdepth")
os.makedirs(mos, exist_ok=True)
have = sorted(f for f in os.listdir(mos) if f.endswith(".regions.bed.gz"))
if len(have) != a.samples:
    gen = os.path.join(ROOT, "tools", "gen_cohort")
    if not os.path.exists(gen) or os.path.getmtime(gen) < os.path.getmtime(gen + ".cpp"):
        subprocess.run(["g++", "-O3", "-std=c++17", "-pthread", "-o", gen, gen + ".cpp", "-lz", "-ldl"], check=True)
    subprocess.run([gen, mos, str(a.samples), str(a.bins), "20260821", str(a.gen_threads), "0"]
                   + (["bgzf"] if a.bgzf else []), check=True)
    have = sorted(f for f in os.listdir(mos) if f.endswith(".regions.bed.gz"))
paths = [os.path.join(mos, f) for f in have]

from grid_amd.device import get_device  # noqa: E402
from grid_amd.utils.coverage_device import cover_files  # noqa: E402
from grid_amd.utils.hi_inference import read_loci_file  # noqa: E402
from grid_amd.utils.mosdepth import region_coverages  # noqa: E402

span = a.bins * 1000
loci = [(lc["chrom"] if a.keep_chrom else "chr1", lc["start"] % span, lc["start"] % span + (lc["end"] - lc["start"]))
        for lc in read_loci_file(a.loci)]
dev = get_device()
runs = []
for _ in range(max(1, a.repeat)):
    t0 = time.perf_counter()
    res = cover_files(dev, paths, loci, batch_files=a.batch_files)
    runs.append({"total_s": time.perf_counter() - t0, "phases_s": dict(res.times), "batches": res.batches,
                 "regrown": res.regrown})
    print(f"[cover] device: {runs[-1]['total_s']:.2f} s  {runs[-1]['phases_s']}  batches {res.batches}",
          file=sys.stderr, flush=True)
paths_rec = {p: res.path.count(p) for p in sorted(set(res.path))}
nonzero = sum(1 for row in res.coverage for v in row if v)

# the host restatement on a sample of the files, spread over the cohort
k = max(1, min(a.host_files, len(paths)))
pick = [round(i * (len(paths) - 1) / max(k - 1, 1)) for i in range(k)] if k > 1 else [0]
t0 = time.perf_counter()
same = True
for f in pick:
    got = region_coverages(paths[f], loci)
    same = same and [None if isinstance(v, Exception) else v for v in got] == res.coverage[f]
host_s = time.perf_counter() - t0
out = {"config": {"files": len(paths), "bins": a.bins, "loci": len(loci),
                  "cohort_bytes": sum(map(os.path.getsize, paths)),
                  "regions_on": "their own chromosome names" if a.keep_chrom
                  else "chr1 (the cohort's only chromosome)"},
       "device": {"runs": runs, "best_total_s": min(r["total_s"] for r in runs), "files_by_path": paths_rec,
                  "nonzero_cells": nonzero},
       "host_restatement": {"files_timed": len(pick), "seconds": host_s, "per_file_s": host_s / len(pick),
                            "scaled_to_cohort_s": host_s / len(pick) * len(paths),
                            "note": "SCALED from the timed files to the cohort (one thread, one walk per file for "
                                    "all regions; the reference walks each file once per region)",
                            "equals_device_on_timed_files": same}}
os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
with open(a.json, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
sys.exit(0 if same else 1)
