"""The device ingest's key modes from files (ingest_device.py: "strict", and
"general" for cohorts that repeat or unsort (start, end) keys), on the BGZF
cohort of tools/bench_dev_ingest.py and on a DECOY copy of it: every file gets
a tail of chr10 lines -- chr1's first ~134 k coordinates with other depths, and
a few bins past chr1's last -- appended as extra BGZF members before the EOF
member, which is what ``chrom: chr1`` keeps of a whole-genome mosdepth file
(the reference's raw startswith; the last line of a key wins).

Timed, digests compared as that tool does (within each cohort):
    host_decoy     the host parser on the decoy cohort
    strict_clean   strict keys on the clean cohort
    general_clean  general keys on the clean cohort (the second pass and the atomics)
    general_decoy  general keys on the decoy cohort
    auto_decoy     ingest(device_keys="auto") on the decoy cohort (strict declines first)

    python tools/bench_ingest_keys.py [--samples 256] [--bins 3000000] [--json profiles/ingest_general_keys.json]
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grid_amd import _abi  # noqa: E402
from grid_amd.device import release_ingest_buffers  # noqa: E402
from grid_amd.utils import normalize_mosdepth as nm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--bins", type=int, default=3_000_000)
ap.add_argument("--tail", type=int, default=134_000, help="chr10 decoy bins per file (chr1's first coordinates)")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--dir", default="/dev/shm/grid_dev_ingest")
ap.add_argument("--modes", default="host_decoy,strict_clean,general_clean,general_decoy,auto_decoy")
ap.add_argument("--repeats", type=int, default=5, help="timed runs per device mode (the host parser runs once)")
ap.add_argument("--json", default="")
a = ap.parse_args()

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_members(data, block=65280):
    """BGZF members of ``data`` (no EOF member)."""
    out = bytearray()
    for p in range(0, len(data), block):
        chunk = data[p:p + block]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out += bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 6)
        out += b"BC" + struct.pack("<HH", 2, 12 + 6 + len(body) + 8 - 1) + body
        out += struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    return bytes(out)


clean = os.path.join(a.dir, "bgzf")
decoy = os.path.join(a.dir, "bgzf_decoy")
os.makedirs(clean, exist_ok=True)
os.makedirs(decoy, exist_ok=True)
gen = os.path.join(ROOT, "tools", "gen_cohort")
if not os.path.exists(gen):
    subprocess.run(["g++", "-O3", "-std=c++17", "-pthread", "-o", gen, gen + ".cpp", "-lz"], check=True)
t0 = time.perf_counter()
if len([f for f in os.listdir(clean) if f.endswith(".regions.bed.gz")]) != a.samples:
    for i0 in range(0, a.samples, 64):
        n = min(64, a.samples - i0)
        subprocess.run([gen, clean, str(n), str(a.bins), "20260821", str(a.threads), str(i0), "bgzf"], check=True)
        print(f"generated {i0 + n} files", flush=True)
ids = [f"S{i:05d}" for i in range(a.samples)]
ntail = min(a.tail, a.bins)
if len([f for f in os.listdir(decoy) if f.endswith(".regions.bed.gz")]) != a.samples:
    bins = list(range(ntail)) + list(range(a.bins, a.bins + 5))
    head = [f"chr10\t{i * 1000}\t{(i + 1) * 1000}\t" for i in bins]
    rng = np.random.default_rng(20260821)
    depth = [f"{d / 100:.2f}\n" for d in rng.integers(1500, 7000, len(bins))]

    def one(k):
        src = open(os.path.join(clean, f"{ids[k]}.regions.bed.gz"), "rb").read()
        assert src.endswith(EOF_MEMBER)
        r = (7919 * k + 1) % len(depth)                    # every file its own decoy depths
        text = "".join(map(str.__add__, head, depth[r:] + depth[:r])).encode()
        with open(os.path.join(decoy, f"{ids[k]}.regions.bed.gz"), "wb") as f:
            f.write(src[:-len(EOF_MEMBER)] + bgzf_members(text) + EOF_MEMBER)
    with ThreadPoolExecutor(a.threads) as ex:
        list(ex.map(one, range(a.samples)))
gen_s = time.perf_counter() - t0


def individuals(d):
    m = nm.map_mosdepth_files_to_samples(d, ids)
    return {k: m[k] for k in ids}


dev = _abi.Device(0)
dev.set_stream(torch.cuda.current_stream())


def digest(r):
    q = r[2].numpy() if isinstance(r[2], _abi.DevBuf) else r[2]
    h = hashlib.sha256(q.tobytes())
    h.update(repr((r[0], r[1][:5], r[1][-5:], len(r[1]))).encode())
    return h.hexdigest()[:16], q.shape


def size_gb(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / 1e9


res = {"samples": a.samples, "bins": a.bins, "tail_bins": ntail, "threads": a.threads, "generate_s": gen_s,
       "clean_gb": size_gb(clean), "decoy_gb": size_gb(decoy), "modes": {}}
first = {}
# untimed: the first device ingest of a process allocates the cached buffers and the staging
del_me = nm._ingest_dev(dev, individuals(clean), clean, "chr1", None, None, {}, 20, 100, a.threads)
del del_me
for mode in a.modes.split(","):
    how, which = mode.split("_")
    d = clean if which == "clean" else decoy
    inds = individuals(d)
    runs = []
    for _ in range(1 if how == "host" else max(1, a.repeats)):
        r = None
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if how == "host":
            r = nm.ingest_native(inds, d, "chr1", None, None, {}, 20, 100, a.threads)
        elif how == "auto":
            r = nm.ingest(inds, d, "chr1", None, None, {}, 20, 100, a.threads, dev=dev, device_keys="auto")
            assert isinstance(r[2], _abi.DevBuf), "auto handed the cohort to the host parser"
        else:
            r = nm._ingest_dev(dev, inds, d, "chr1", None, None, {}, 20, 100, a.threads, keys=how)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t1)
    dg = digest(r)
    first.setdefault(which, dg)
    # seconds: the median run
    res["modes"][mode] = {"seconds": float(np.median(runs)), "runs": runs, "digest": dg[0], "shape": list(dg[1]),
                          "same_as_first": dg == first[which]}
    print(json.dumps({mode: res["modes"][mode]}), flush=True)
    del r
release_ingest_buffers(dev)
assert all(v["same_as_first"] for v in res["modes"].values())
m = res["modes"]
if "general_clean" in m and "strict_clean" in m:
    res["general_over_strict_clean"] = m["general_clean"]["seconds"] / m["strict_clean"]["seconds"]
if "general_decoy" in m and "host_decoy" in m:
    res["general_faster_than_host_on_decoy"] = m["general_decoy"]["seconds"] < m["host_decoy"]["seconds"]
print(json.dumps(res), flush=True)
if a.json:
    open(a.json, "w").write(json.dumps(res) + "\n")
