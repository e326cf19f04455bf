"""Step 5's read of the normalised matrix file: the host reader plus the
upload of its matrix (what a stand-alone step 5 did before the device
reader) against _abi.read_normalized_gz_dev, alternating in one process,
each timed with a host clock that ends in a device synchronise, after one
warm-up of each.  The file is written by the device writer from a seeded
matrix (a block of seeded rows tiled over the samples).  The two matrices
are compared once on the device (their CRC-32 in HBM).

    python tools/bench_ntext_read.py [--n 3202] [--r 2700000] [--json profiles/ntext_read_config2.json]

The cost rule's constants in grid_amd/utils/ntext_device.py come from this
tool's records: WAVE_RATE = member text / the inflate phase of one batch,
HOST_RATE_PER_THREAD = text / (host read seconds x threads).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grid_amd import _abi  # noqa: E402
from grid_amd.device import release_ingest_buffers  # noqa: E402
from grid_amd.utils import ntext_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3202)
ap.add_argument("--r", type=int, default=2_700_000)
ap.add_argument("--block", type=int, default=32, help="seeded rows generated on the host, tiled to n")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--dir", default=None, help="where the file lives (default: a fresh directory under TMPDIR or /tmp)")
ap.add_argument("--json", default=None)
a = ap.parse_args()


def fstype(path):
    best = ("", "?")
    real = os.path.realpath(path)
    for line in open("/proc/mounts"):
        p = line.split()
        if len(p) >= 3 and (real == p[1] or real.startswith(p[1].rstrip("/") + "/")) and len(p[1]) > len(best[0]):
            best = (p[1], p[2])
    return best[1]


def say(msg):
    print(f"[bench_ntext_read] {msg}", file=sys.stderr, flush=True)


dev = _abi.Device(0)
rng = np.random.default_rng(0)
nb = min(a.block, a.n)
blk = np.rint(rng.normal(0, 100, (nb, a.r))).astype(np.int32)      # z in hundredths, as step 4 leaves it
dz = dev.alloc((a.n, a.r), np.int32)
d_blk = dev.upload(blk)
for i in range(0, a.n, nb):
    k = min(nb, a.n - i)
    _abi.call("grid_d2d", dev.ctx, dz.ptr + i * a.r * 4, d_blk.ptr, k * a.r * 4)
del d_blk, blk
raw = rng.uniform(20, 40, a.n)
means, ratios = rng.uniform(0.8, 1.2, a.r), rng.uniform(0.5, 20, a.r)
ids = [f"S{i:06d}" for i in range(a.n)]
d = a.dir or tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(d, exist_ok=True)
fs = fstype(d)
path = os.path.join(d, "ntext_bench.tsv.gz")
t0 = time.perf_counter()
_abi.write_normalized_gz_dev(dev, path, ids, raw, means, ratios, dz, a.n, a.r, a.r, level=1, threads=a.threads)
t_write = time.perf_counter() - t0
del dz
ix = _abi.ntext_index(path)
text = int(ix["isize"].sum())
say(f"file {os.path.getsize(path)} B, text {text} B, {len(ix['isize'])} members, written in {t_write:.2f} s")


def host_path():
    t0 = time.perf_counter()
    got = _abi.read_normalized_gz(path, threads=a.threads)
    t1 = time.perf_counter()
    dzq = dev.upload(got[4])
    dev.sync()
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, got[:4], dzq


def dev_path():
    t0 = time.perf_counter()
    got = _abi.read_normalized_gz_dev(dev, path, threads=a.threads)
    dev.sync()
    t = time.perf_counter() - t0
    return t, got[:4], got[4]


def phases():
    tm = {}
    _abi.read_normalized_gz_dev(dev, path, threads=a.threads, timings=tm)
    return tm


def crc(buf):
    n = buf.nbytes
    offs = np.arange(0, n, 1 << 30, dtype=np.int64)
    return _abi.text_crc32(dev, buf.ptr, offs, np.minimum(1 << 30, n - offs)).tolist()


# warm-up of each, and the output check
t, _, ha, hz = host_path()
say(f"warm-up host {t:.2f} s")
t, da, dzq = dev_path()
say(f"warm-up device {t:.2f} s")
equal = (ha[0] == da[0] and ha[1].tobytes() == da[1].tobytes() and ha[2].tobytes() == da[2].tobytes()
         and ha[3].tobytes() == da[3].tobytes() and hz.shape == dzq.shape and crc(hz) == crc(dzq))
say(f"outputs equal: {equal}")
del hz, dzq, ha, da
host_s, host_read_s, dev_s = [], [], []
for rep in range(a.reps):
    t, tr, _, hz = host_path()
    del hz
    host_s.append(t)
    host_read_s.append(tr)
    t, _, dzq = dev_path()
    del dzq
    dev_s.append(t)
    say(f"rep {rep}: host {host_s[-1]:.2f} s (read {tr:.2f}), device {dev_s[-1]:.2f} s")
ph = phases()
release_ingest_buffers(dev)
os.remove(path)
if a.dir is None:
    shutil.rmtree(d, ignore_errors=True)
rec = {"n": a.n, "r": a.r, "members": len(ix["isize"]), "member_text_max": int(ix["isize"].max()),
       "gzip_bytes": int(ix["off"][-1] + ix["len"][-1]), "text_bytes": text, "threads": a.threads,
       "host_read_plus_upload_s": host_s, "host_read_s": host_read_s, "device_read_s": dev_s,
       "host_text_GBps": [text / t / 1e9 for t in host_s], "device_text_GBps": [text / t / 1e9 for t in dev_s],
       "device_phases_s": ph, "outputs_equal": bool(equal), "file_dir": d, "file_fstype": fs,
       "write_s": t_write,
       "accept_default_on": bool(equal and max(dev_s) <= 0.5 * min(host_s)),
       "wave_rate_Bps": int(ix["isize"].max()) / ph["inflate"] * ph["batches"] if ph.get("inflate") else None,
       "host_rate_per_thread_Bps": text / min(host_read_s) / a.threads}
line = json.dumps(rec)
print(line)
if a.json:
    os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
