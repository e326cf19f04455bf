"""Step 5's read on the device: the normalised matrix file (<prefix>.tsv.gz,
grid_amd/csrc/textio.cpp) -> the int32 hundredths matrix in HBM, without the
host ever inflating or parsing a row.  The write path's mirror
(gzwrite.hip writes this file on the GPU).

The file is a multi-member gzip with the 'GR' index: member 0 holds the two
header lines, every other member whole rows from its ``first_row``.  The host
reads the member table and the header member (grid_ntext_index_*), then per
batch of row members (bounded compressed and text bytes, BATCH_IN /
BATCH_TEXT): host threads read the compressed members into staging while the
GPU works on the previous batch, a copy stream moves them to HBM,
grid_gunzip_batch inflates them one wave per member (CRC-checked) and
grid_ntext_count / grid_ntext_parse / grid_ntext_prefix turn the text into
zq [N][R] and the first bytes of every row, from which the host takes the ID
and the scale with the host reader's own float parser.

One wave inflates one member, serially: a file's device time is the time of
one member however many members there are, up to the resident waves.  So the
batches are as large as the bounds allow (one batch for a cohort of a few
thousand samples), and ``prefer_device`` estimates both readers' times.

The contract: ``read`` returns exactly what _abi.read_normalized_gz returns,
or raises DeviceReadUnsupported and the caller uses that reader, which then
gives whatever result or error it gives for the file.  Raised for: no 'GR'
index, N == 0 or R == 0, a member of 2 GiB or more, first rows that are not
the running sums of the members' rows, a member that fails to inflate or its
CRC, any parse flag (GRID_NT_*), and a matrix plus batch buffers beyond the
free HBM.
"""
from __future__ import annotations

import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _abi
from .._abi import call
from .gz_batch import CH, READ_THREADS, align, chunk_table, staging

BATCH_IN = 20 << 30             # compressed bytes per batch
BATCH_TEXT = 48 << 30           # inflated bytes per batch
WAVES_PER_CU = 32               # k_inflate: 8 waves on each of a CU's 4 SIMDs (inflate.hip GRID_INFLATE_WPE)
P = _abi.NT_PREFIX_BYTES

# The automatic choice (config key mosdepth.neighbors.device_read absent):
# estimated device time against estimated host time, in the style of
# ingest_device._Split.  Both rates come from tools/bench_ntext_read.py; see
# the values' comments for the records they were taken from.
# One wave's rate: a member's text over the inflate phase of its (one) batch --
# 8.86 MB/s with 3,202 members of 14.8 MB resident at once
# (profiles/ntext_read_config2.json), 11.0 MB/s with 64
# (profiles/ntext_read_64rows.json); the fuller device's figure is kept.
WAVE_RATE = 8.86e6
# One host thread's rate inside grid_read_normalized_gz, text over its seconds
# over 16 threads: 267 MB/s at config 2 (profiles/ntext_read_config2.json),
# 101 MB/s at 64 members, which leave the threads' last round part empty
# (profiles/ntext_read_64rows.json); the busy threads' figure is kept.
HOST_RATE_PER_THREAD = 267e6
# Default on: at config 2 the slowest of the device reader's three runs took
# 2.63 s, the fastest host read plus upload 11.76 s.
AUTO_DEVICE = True


class DeviceReadUnsupported(Exception):
    """The file leaves what the device reader covers (see the module doc)."""


def prefer_device(members, member_text, text, threads, cus):
    """The cost rule: device time = ceil(members / resident waves) x one
    member's text / one wave's rate (a file of few, huge members is serial on
    the GPU); host time = text / (threads x one thread's rate)."""
    if not AUTO_DEVICE or not WAVE_RATE or not HOST_RATE_PER_THREAD:
        return False
    resident = max(1, int(cus) * WAVES_PER_CU)
    t_dev = -(-int(members) // resident) * float(member_text) / WAVE_RATE
    t_host = float(text) / (max(1, int(threads)) * HOST_RATE_PER_THREAD)
    return t_dev < t_host


def auto_choice(dev, path, threads):
    """prefer_device for ``path`` (False for a file without the index)."""
    if not AUTO_DEVICE:
        return False
    try:
        ix = _abi.ntext_index(path, header=False)     # the member table alone: no header parse
    except _abi.GridNativeError:
        return False
    if not len(ix["isize"]):
        return False
    return prefer_device(len(ix["isize"]), int(ix["isize"].max()), int(ix["isize"].sum()), threads,
                         _abi.device_cu_count(dev))


def plan_batches(clen, tlen, batch_in=None, batch_text=None):
    """Members (compressed and text bytes, file order) -> batches of member
    indices in file order, each within both bounds (256-B aligned sizes); a
    member larger than a bound is alone in its batch."""
    bi = BATCH_IN if batch_in is None else batch_in
    bt = BATCH_TEXT if batch_text is None else batch_text
    batches, cur, cin, ctx = [], [], 0, 0
    for m in range(len(clen)):
        a, b = align(max(int(clen[m]), 1)), align(max(int(tlen[m]), 1))
        if cur and (cin + a > bi or ctx + b > bt):
            batches.append(cur)
            cur, cin, ctx = [], 0, 0
        cur.append(m)
        cin += a
        ctx += b
    if cur:
        batches.append(cur)
    return batches


def _cached(dev, name, want, budget):
    """dev.cached(name, want) against a byte budget of new HBM."""
    budget[0] -= max(0, want - dev.cached_nbytes(name))
    if budget[0] < 0:
        raise DeviceReadUnsupported("the matrix and the batch buffers do not fit in the free HBM")
    return dev.cached(name, want)


def read(dev, path, threads=None, timings=None):
    """-> (ids, scales [n], means [r], ratios [r], zq DevBuf [n][r] int32);
    raises DeviceReadUnsupported.  ``timings`` (a dict): per-phase seconds
    (disk read, copy to HBM, inflate, parse), each phase then ends in a
    device synchronise."""
    path = str(path)
    try:
        ix = _abi.ntext_index(path)
    except _abi.GridNativeError as e:
        if e.code != _abi.GRID_EUNSUPPORTED:
            raise
        raise DeviceReadUnsupported("no 'GR' member index (not this project's writer)") from None
    N, R = ix["n"], ix["r"]
    off, clen, frow, isize = ix["off"], ix["len"], ix["first_row"], ix["isize"]
    M = len(off)
    if N == 0 or R == 0:
        raise DeviceReadUnsupported("an empty matrix (N == 0 or R == 0)")
    if M == 0:
        raise DeviceReadUnsupported("no row members")
    if int(clen.max()) >= 2 ** 31:
        raise DeviceReadUnsupported("a member of 2 GiB or more")
    if int(isize.min()) == 0:
        raise DeviceReadUnsupported("a member without text")
    # every member holds at least one row: first rows start at 0 and increase
    if frow[0] != 0 or np.any(np.diff(frow) <= 0) or frow[-1] >= N:
        raise DeviceReadUnsupported("member first rows are not running row counts")
    batches = plan_batches(clen, isize)
    in_need = 256 + max(int(align(np.maximum(clen[b], 1)).sum()) for b in batches)
    text_need = 256 + P + max(int(align(np.maximum(isize[b], 1)).sum()) for b in batches)
    nchunk_max = max(int((-(-isize[b] // CH)).sum()) for b in batches)
    small = N * (8 + P) + 64 * nchunk_max + 256 * max(len(b) for b in batches) + (64 << 20)
    free, _total = dev.mem_info()
    budget = [int(free) - N * R * 4 - small]
    if budget[0] < 0:
        raise DeviceReadUnsupported("the matrix does not fit in the free HBM")
    nin = min(2, len(batches))
    d_ins = [_cached(dev, f"ingest_in{p}", in_need, budget) for p in range(nin)]
    d_text = _cached(dev, "ingest_text", text_need, budget)
    zq = dev.alloc((N, R), np.int32)
    rowoff = dev.alloc(N, np.int64).fill_bytes(0xFF)
    pre = dev.zeros((N, P), np.uint8)
    stag = [staging(f"in{p}", BATCH_IN + 512) for p in range(nin)]
    pool = ThreadPoolExecutor(max(1, READ_THREADS))
    rpool = ThreadPoolExecutor(1)
    cdev = _abi.Device(dev.index)             # the copy stream
    fd = os.open(path, os.O_RDONLY)
    tm = {"disk_read": 0.0, "copy_to_hbm": 0.0, "inflate": 0.0, "parse": 0.0}

    def read_batch(bi):
        t0 = time.perf_counter()
        ms = batches[bi]
        ioff = np.zeros(len(ms) + 1, np.int64)
        ioff[1:] = np.cumsum(align(np.maximum(clen[ms], 1)))
        buf = stag[bi % 2].get(int(ioff[-1]) + 256)
        mv = memoryview(buf)

        def one(k):
            m = ms[k]
            a, n, o = int(ioff[k]), int(clen[m]), int(off[m])
            while n:
                got = os.preadv(fd, [mv[a:a + n]], o)
                if got <= 0:
                    raise DeviceReadUnsupported(f"{path} changed while reading")
                a, n, o = a + got, n - got, o + got
        list(pool.map(one, range(len(ms))))
        return buf, ioff, time.perf_counter() - t0

    keep, outs = [], []
    pending = rpool.submit(read_batch, 0)
    try:
        for bi, ms in enumerate(batches):
            buf, ioff, t_read = pending.result()
            tm["disk_read"] += t_read
            # staging of parity bi % 2 is free again once this batch's copy
            # below has returned; d_ins[bi % 2] was last read by batch bi - 2,
            # done before batch bi - 1's tables went up (dev.upload synchronises)
            t0 = time.perf_counter()
            d_in = d_ins[bi % 2]
            call("grid_h2d", cdev.ctx, d_in.ptr, buf.ctypes.data, int(ioff[-1]))
            tm["copy_to_hbm"] += time.perf_counter() - t0
            pending = rpool.submit(read_batch, bi + 1) if bi + 1 < len(batches) else None
            nb = len(ms)
            tlen = isize[ms].astype(np.int64)
            toff = np.zeros(nb + 1, np.int64)
            toff[1:] = np.cumsum(align(np.maximum(tlen, 1)))
            cfile, cstart, cfirst, nch = chunk_table(np.arange(nb), tlen)
            up = [dev.upload(np.ascontiguousarray(a)) for a in
                  (ioff[:-1], clen[ms].astype(np.int64), toff[:-1], tlen, frow[ms].astype(np.int64), cfile, cstart,
                   cfirst)]
            d_ioff, d_clen, d_toff, d_tlen, d_frow, d_cfile, d_cstart, d_cfirst = up
            mem = dev.alloc(nb * _abi.GZ_MEMBER_BYTES, np.uint8)
            st, ln, nm = dev.alloc(nb, np.int32), dev.alloc(nb, np.int64), dev.alloc(nb, np.int32)
            csep, cnl, cfield0 = dev.alloc(nch, np.int32), dev.alloc(nch, np.int32), dev.alloc(nch, np.int64)
            nrows, flags = dev.zeros(nb, np.int64), dev.zeros(nb, np.int32)
            call("grid_stream_after", dev.ctx, cdev.ctx)
            t0 = time.perf_counter()
            call("grid_gunzip_batch", dev.ctx, d_in.ptr, d_ioff.ptr, d_clen.ptr, nb, d_text.ptr, d_toff.ptr,
                 d_tlen.ptr, mem.ptr, 1, st.ptr, ln.ptr, nm.ptr)
            if timings is not None:
                dev.sync()
                tm["inflate"] += time.perf_counter() - t0
                t0 = time.perf_counter()
            call("grid_ntext_count", dev.ctx, d_text.ptr, d_toff.ptr, d_tlen.ptr, nch, d_cfile.ptr, d_cstart.ptr,
                 d_cfirst.ptr, nb, csep.ptr, cnl.ptr, cfield0.ptr, nrows.ptr, flags.ptr, st.ptr)
            call("grid_ntext_parse", dev.ctx, d_text.ptr, d_toff.ptr, d_tlen.ptr, d_frow.ptr, nch, d_cfile.ptr,
                 d_cstart.ptr, cfield0.ptr, N, R, zq.ptr, R, rowoff.ptr, flags.ptr, st.ptr)
            call("grid_ntext_prefix", dev.ctx, d_text.ptr, int(toff[-1]), rowoff.ptr, N, pre.ptr)
            if timings is not None:
                dev.sync()
                tm["parse"] += time.perf_counter() - t0
            keep.append((up, mem, ln, nm, csep, cnl, cfield0))
            outs.append((st, nrows, flags))
        dev.sync()
        status = np.concatenate([o[0].numpy() for o in outs])
        rows = np.concatenate([o[1].numpy() for o in outs])
        fl = np.concatenate([o[2].numpy() for o in outs])
    finally:
        try:
            if pending is not None:
                try:
                    pending.result()
                except Exception:
                    pass
            dev.sync()
            cdev.sync()
        finally:
            rpool.shutdown(wait=True)
            pool.shutdown(wait=True)
            os.close(fd)
            keep.clear()
            outs.clear()
            cdev.close()
    if timings is not None:
        timings.update(tm, batches=len(batches), members=M)
    if np.any(status != 0):
        k = int(np.flatnonzero(status)[0])
        raise DeviceReadUnsupported(f"member {k + 1} does not inflate (status {int(status[k])})")
    if np.any(fl != 0):
        k = int(np.flatnonzero(fl)[0])
        raise DeviceReadUnsupported(f"member {k + 1}: {_abi.ntext_flag_text(fl[k])}")
    first = np.zeros(M, np.int64)
    np.cumsum(rows[:-1], out=first[1:])
    if not np.array_equal(first, frow) or int(rows.sum()) != N:
        raise DeviceReadUnsupported("member first rows are not the running sums of the members' rows")
    ids, scales, rfl = _abi.ntext_rows(pre.numpy())
    if np.any(rfl != 0):
        k = int(np.flatnonzero(rfl)[0])
        raise DeviceReadUnsupported(f"row {k}: {_abi.ntext_flag_text(rfl[k])}")
    return ids, scales, ix["means"].copy(), ix["ratios"].copy(), zq
