"""Region coverage of a loci table from the cohort's mosdepth files, on the
device (reference grid/utils/mosdepth.py compute_region_coverage :264-297 for
every (file, region); kernels: grid_amd/csrc/mosdepth_dev.hip k_md_cover).

The reference walks every sample's regions.bed.gz in Python once per region.
Here a batch of files is read, inflated in HBM (grid_gunzip_batch: one wave per
BGZF member, one wave per file for a plain gzip file, as the step-4 ingest
does), cut in 16 KiB chunks, its lines numbered (grid_md_count) and ONE pass
over the text (grid_md_cover) serves every region of the table: each line that
overlaps a locus of its own chromosome leaves a hit, the hits are sorted by
(file, locus, line) and summed in that order, so the fp64 sum of a region takes
its lines in file order as the reference's loop does, whatever workgroup
parsed them.  The next batch's files are read while the device works.

Per file, what ``CoverResult.path`` records:
  * "device"               inflated and parsed on the device;
  * "device:host-inflate"  the device did not inflate it, the host did
                           (grid_gunzip_host) and its text was parsed on the
                           device;
  * "host"                 the device handed it over -- a line outside the
                           canonical mosdepth grammar (GRID_MD_EXOTIC: an empty
                           line, other than four fields, a CR, a byte >= 0x80,
                           a depth like 1e3 or nan, more than 256 bytes), or
                           text that does not fit where the device put it --
                           and mosdepth.region_coverages recomputed it; the
                           other files of its batch stay on the device;
  * "failed"               it inflates on neither side: no value, as the
                           reference's "Error" for a file gzip cannot read.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from .. import _abi
from .._abi import call
from .gz_batch import READ_THREADS, align, chunk_table, fold_members, member_units, whole_units
from .gz_batch import gpu_inflate as _gpu_inflate      # cover_files launches through this module's name (a test seam)
from .mosdepth import region_sums, coverage_value

BATCH_FILES = 256               # files per batch (n_loci * files stays far below 2^31)
BATCH_TEXT = 8 << 30            # inflated bytes per batch
READ_AHEAD = 4 << 30            # compressed bytes read ahead of the parse
HIT_CAPACITY = 1 << 20          # hit records per batch to start with (20 bytes each); grown on demand
MAXPOS = 1 << 60                # mosdepth_dev.hip: the table's starts and ends lie in [0, 2^60), as a line's do


class CoverUnsupported(Exception):
    """The loci table leaves what the device kernel reads (a start or end
    outside [0, 2^60)): the caller runs the host restatement."""


@dataclass
class CoverResult:
    coverage: list              # [files][loci]: int, or None where the reference gives "Error"
    region_cov: np.ndarray      # [files][loci] float64: the reference's region_cov sum
    covered_bp: np.ndarray      # [files][loci] int64
    path: list                  # per file, see the module doc
    regrown: int = 0            # times a batch was repeated with a larger hit buffer
    batches: int = 0
    times: dict = field(default_factory=dict)   # seconds: read (waited for), inflate, parse, host


class LociTable:
    """The table on the device (include/grid_abi.h grid_cover_loci), uploaded
    once: chromosomes sorted by (length, bytes), each one's loci by start."""

    def __init__(self, dev, loci):
        if not loci:
            raise ValueError("no locus")
        for _, s, e in loci:
            if not (0 <= int(s) < MAXPOS and 0 <= int(e) < MAXPOS):
                raise CoverUnsupported(f"locus bounds {s}-{e} outside [0, 2^60)")
        names = sorted({c.encode() for c, _, _ in loci}, key=lambda b: (len(b), b))
        cid = {b: i for i, b in enumerate(names)}
        order = sorted(range(len(loci)), key=lambda i: (cid[loci[i][0].encode()], int(loci[i][1])))
        first = np.zeros(len(names) + 1, np.int32)
        for i in order:
            first[cid[loci[i][0].encode()] + 1] += 1
        np.cumsum(first, out=first)
        start = np.array([int(loci[i][1]) for i in order], np.int64)
        end = np.array([int(loci[i][2]) for i in order], np.int64)
        length = np.maximum(end - start, 0)
        maxlen = np.array([length[first[c]:first[c + 1]].max() for c in range(len(names))], np.int64)
        name_off = np.zeros(len(names) + 1, np.int32)
        name_off[1:] = np.cumsum([len(b) for b in names])
        self.n = len(loci)
        self._keep = [dev.upload(np.frombuffer(b"".join(names) or b"\0", np.uint8)), dev.upload(name_off),
                      dev.upload(first), dev.upload(maxlen), dev.upload(start), dev.upload(end),
                      dev.upload(np.array(order, np.int32))]
        k = self._keep
        self.desc = _abi.CoverLoci(self.n, len(names), k[0].ptr, k[1].ptr, k[2].ptr, k[3].ptr, k[4].ptr, k[5].ptr,
                                   k[6].ptr)


def _read(path):
    """(compressed bytes, (text size, members) or None, BGZF member table or None)"""
    try:
        v = np.fromfile(path, np.uint8)
    except OSError:
        return np.zeros(1, np.uint8), None, None     # unreadable: not gzip, no value
    if not v.size:
        return v, (0, 0), None
    return v, _abi.gz_text_size(v), _abi.gz_members(v)


def _host_inflate(v, cap):
    """The file's text inflated on the host, or None.  ``cap`` is the size its
    trailer states; a file of several plain gzip members states only its last
    member's, so the room doubles while the host reports it too small."""
    cap = max(int(cap), 1 << 16)
    while cap <= 1 << 36:
        out = np.empty(cap, np.uint8)
        st, n = _abi.gunzip_host(v, out)
        if st == _abi.GZ_OK:
            return out[:n]
        if st != _abi.GZ_ESPACE:
            return None
        cap *= 4
    return None


def cover_files(dev, paths, loci, batch_files=None, hit_capacity=None, batch_text=None):
    """Coverage of every (file, locus): ``paths`` the regions.bed.gz files,
    ``loci`` (chrom, start, end) triples.  ``batch_files`` / ``batch_text``
    bound a batch, ``hit_capacity`` is the hit buffer's first size (a batch
    with more hits is repeated with a buffer that holds them).  Returns a
    CoverResult; a table the device does not read (CoverUnsupported) is
    computed by the host restatement, file by file."""
    loci = [(str(c), int(s), int(e)) for c, s, e in loci]
    nf, nl = len(paths), len(loci)
    res = CoverResult([[None] * nl for _ in range(nf)], np.zeros((nf, nl), np.float64), np.zeros((nf, nl), np.int64),
                      ["failed"] * nf, times=dict(read=0.0, inflate=0.0, parse=0.0, host=0.0))

    def on_host(f):
        t0 = time.perf_counter()
        cov, bp, err = region_sums(paths[f], loci)
        for l in range(nl):
            v = err[l]
            if v is None:
                try:
                    v = coverage_value(cov[l], bp[l])
                except Exception as e:
                    v = e
            res.coverage[f][l] = None if isinstance(v, Exception) else v
            res.region_cov[f, l] = cov[l]
            res.covered_bp[f, l] = bp[l] if bp[l] < 1 << 63 else -1
        res.path[f] = "host"
        res.times["host"] += time.perf_counter() - t0

    try:
        table = LociTable(dev, loci)
    except CoverUnsupported:
        for f in range(nf):
            on_host(f)
        return res
    batch_files = max(1, int(batch_files or BATCH_FILES))
    batch_text = int(batch_text or BATCH_TEXT)
    cap = max(1, int(hit_capacity or HIT_CAPACITY))
    hits = None
    ld = -(-nl // 8) * 8
    iopool = ThreadPoolExecutor(max(1, READ_THREADS))
    sizes = [os.path.getsize(p) if os.path.exists(p) else 0 for p in paths]
    queue, nxt, ahead = deque(), 0, 0

    def pump():
        """Start reads, in file order, up to READ_AHEAD compressed bytes ahead of the parse."""
        nonlocal nxt, ahead
        while nxt < nf and len(queue) < 2 * batch_files and (not queue or ahead + sizes[nxt] <= READ_AHEAD):
            queue.append((nxt, iopool.submit(_read, paths[nxt])))
            ahead += sizes[nxt]
            nxt += 1

    try:
        pump()
        while queue:
            # the next batch: files in order while their text fits the bound
            t0 = time.perf_counter()
            fs, info, size = [], [], 0
            while queue and len(fs) < batch_files:
                f, fut = queue[0]
                one = fut.result()
                size += align(max(min(one[1][0], 1032 * one[0].size + 1024) if one[1] else 0, 1))
                if fs and size > batch_text:
                    break
                queue.popleft()
                ahead -= sizes[f]
                fs.append(f)
                info.append(one)
            pump()                                   # the reads go on while the device works
            res.batches += 1
            t1 = time.perf_counter()
            res.times["read"] += t1 - t0
            nb, h1 = len(fs), res.times["host"]      # (host recomputes are timed on their own)
            # ---- inflate: the GPU first, then the host for what it refused ----
            # the text size a file states, bounded by what DEFLATE can expand its bytes to (1032:1):
            # a damaged trailer must not size the buffers
            tsize = np.array([min(ts[0], 1032 * v.size + 1024) if ts else 0 for v, ts, _ in info], np.int64)
            off = np.zeros(nb + 1, np.int64)
            off[1:] = np.cumsum([align(max(v.size, 1)) for v, _, _ in info])
            tcap = np.array([align(max(c, 1)) for c in tsize], np.int64)
            toff = np.zeros(nb + 1, np.int64)
            toff[1:] = np.cumsum(tcap)
            # the batch's device buffers are kept between batches (an allocation of GBs per batch
            # costs more than its parse) and released when the cohort is done
            d_in = dev.cached("cover_in", int(off[-1]) + 256)
            d_text = dev.cached("cover_text", int(toff[-1]) + 256)
            for k, (v, _, _) in enumerate(info):
                if v.size:
                    call("grid_h2d", dev.ctx, d_in.ptr + int(off[k]), v.ctypes.data, int(v.size))
            gst = np.zeros(nb, np.int32)
            tlen = np.zeros(nb, np.int64)
            mu = [k for k in range(nb) if info[k][0].size and info[k][1] and info[k][2] is not None]
            wu = [k for k in range(nb) if info[k][0].size and info[k][1] and info[k][2] is None]
            for k in range(nb):
                if info[k][0].size and not info[k][1]:
                    gst[k] = _abi.GZ_EHEADER                  # not gzip
            if wu:                                            # plain gzip: one wave per file
                units, mcap = whole_units(off, [v.size for v, _, _ in info], toff, tsize, wu)
                whole = _gpu_inflate(dev, d_in, d_text, units, mcap)
                gst[wu], tlen[wu] = whole[2].numpy(), whole[3].numpy()
            if mu:                                            # BGZF: one wave per member
                *units, owner = member_units([m for _, _, m in info], off, toff, mu)
                parts = _gpu_inflate(dev, d_in, d_text, units, 1)
                d_owner, d_bad = dev.upload(owner), dev.alloc(nb, np.int32)
                call("grid_file_status", dev.ctx, parts[2].ptr, d_owner.ptr, len(owner), d_bad.ptr, nb)
                tot = fold_members(nb, owner, unit_len=parts[3].numpy())[1]
                gst[mu], tlen[mu] = d_bad.numpy()[mu], tot[mu]
            for k in range(nb):
                f = fs[k]
                res.path[f] = "device"
                if gst[k] == 0:
                    continue
                tlen[k] = 0
                text = _host_inflate(info[k][0], tsize[k])
                if text is None:
                    res.path[f] = "failed"
                elif text.size > tcap[k]:
                    on_host(f)
                else:
                    if text.size:
                        call("grid_h2d", dev.ctx, d_text.ptr + int(toff[k]), text.ctypes.data, int(text.size))
                    gst[k], tlen[k] = 0, text.size
                    res.path[f] = "device:host-inflate"
            dev.sync()
            t2 = time.perf_counter()
            res.times["inflate"] += t2 - t1 - (res.times["host"] - h1)
            # ---- parse: line numbers, then every locus in one pass ----
            on_dev = [k for k in range(nb) if res.path[fs[k]].startswith("device")]
            okb = [k for k in on_dev if tlen[k] > 0]
            flags = np.zeros(nb, np.int32)
            cov = np.zeros((nb, ld), np.float64)
            bp = np.zeros((nb, ld), np.int64)
            out = np.zeros((nb, ld), np.int64)
            cfile, cstart, cfirst, nch = chunk_table(okb, tlen)
            if nch:
                fst = np.ones(nb, np.int32)
                fst[okb] = 0
                d_tl, d_toff, d_fst = dev.upload(tlen), dev.upload(toff[:nb]), dev.upload(fst)
                d_cfile, d_cstart, d_cfirst = dev.upload(cfile), dev.upload(cstart), dev.upload(cfirst)
                cnl, cline0 = dev.alloc(nch, np.int32), dev.alloc(nch, np.int64)
                d_flags = dev.zeros(nb, np.int32)
                d_cov, d_bp, d_out = (dev.alloc((nb, ld), np.float64), dev.alloc((nb, ld), np.int64),
                                      dev.alloc((nb, ld), np.int64))
                call("grid_md_count", dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, nch, d_cfile.ptr, d_cstart.ptr,
                     d_cfirst.ptr, len(okb), cnl.ptr, cline0.ptr, d_flags.ptr, d_fst.ptr)
                while True:
                    if hits is None:
                        hits = (dev.alloc(cap, np.uint64), dev.alloc(cap, np.int64), dev.alloc(cap, np.int32))
                    need = C.c_int64()
                    call("grid_md_cover", dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, nch, d_cfile.ptr, d_cstart.ptr,
                         cline0.ptr, d_fst.ptr, nb, C.byref(table.desc), hits[0].ptr, hits[1].ptr, hits[2].ptr, cap,
                         C.byref(need), d_cov.ptr, d_bp.ptr, d_out.ptr, ld, d_flags.ptr)
                    if need.value <= cap:
                        break
                    # nothing was written: the same batch again, with room for its hits
                    cap, hits = max(int(need.value), 2 * cap), None
                    res.regrown += 1
                flags, cov, bp, out = d_flags.numpy(), d_cov.numpy(), d_bp.numpy(), d_out.numpy()
            res.times["parse"] += time.perf_counter() - t2
            for k in on_dev:
                f = fs[k]
                if flags[k]:
                    on_host(f)
                    continue
                res.coverage[f] = [int(x) for x in out[k, :nl]]
                res.region_cov[f], res.covered_bp[f] = cov[k, :nl], bp[k, :nl]
            whole = parts = d_in = d_text = None
    finally:
        iopool.shutdown(wait=True, cancel_futures=True)
        dev.release_cached("cover_")
    return res
