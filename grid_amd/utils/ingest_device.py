"""Step-4 ingest on the device: mosdepth regions.bed.gz files -> the int32
hundredths depth matrix in HBM (R1-R4, normalize_mosdepth.py:96-112 and
:218-416), for the cohorts the host parser would read the common way.

Per batch of files (bounded compressed and text bytes): host threads read the
compressed bytes into pinned memory and find each file's BGZF members (what
mosdepth writes: independent gzip members of <= 64 KiB text).  The batch's
files are then inflated by the GPU and the host CPUs AT ONCE, split by a cost
model whose rates are re-measured every batch (``_Split``):
  * GPU (grid_gunzip_batch, CRC-checked): one wave per BGZF member -- a
    member-granular work list that fills every CU -- or one wave per file for
    a single-member gzip file (serial by nature: the model gives the GPU such
    a file only when a wave's rate makes it worth it);
  * CPU (grid_gunzip_host: libdeflate, zlib without it): threads inflate
    whole files into pinned staging, copied to HBM on a second stream while
    the GPU works.
The text then is cut in 16 KiB chunks and parsed on the GPU (grid_md_count /
grid_md_parse_map: the reference's line filters, each record placed by its
(start, end) in the key list K of the reference file).  Then the population
means in file order, the valid columns, the empty-sample filter and the rows
in sorted-ID order (grid_md_finish / grid_md_gather) -- the matrix never
exists on the host.

Text the host threads inflated is checked where it sits in HBM before it is
parsed: the CRC-32 of each such file's text in d_text (grid_text_crc32) must
equal the CRC its gzip trailers give (the GPU-inflated members are checked the
same way by grid_gunzip_batch's k_gz_crc); a mismatch hands the cohort to the
host parser.

Two key modes (``keys=``).  "strict", the fast common case: the reference
file's kept (start, end) keys are strictly increasing in line order and no
file repeats a key; otherwise DeviceIngestKeys (a DeviceIngestUnsupported).
"general", the reference's own semantics for any order and any repeats (its
raw ``startswith("chr1")`` also keeps the lines of chr10..chr19, whose bins
repeat chr1's coordinates): the columns are the sorted, de-duplicated kept keys
of the reference file (grid_md_parse_ref_general) and within a file a key takes
the value of the LAST line in file order that passes every filter
(grid_md_parse_map_general: a tag pass and a resolve pass over the same text,
no memory beyond the matrix).  normalize_mosdepth.ingest tries strict first and
general on DeviceIngestKeys (config ``mosdepth.normalize.device_keys``).

What still hands over in either mode -- a line outside the canonical mosdepth
grammar or a non-ASCII byte, a line of more than 256 bytes (mosdepth_dev.hip
MAXLINE: the look-ahead a parse chunk holds; it applies to every line, one
that fails the chromosome prefix and the file's unterminated last line
included), with no chromosome prefix an empty line (the reference skips it,
the device grammar has no such line), a key outside K, text in HBM that does not match
its gzip CRC, a file of plain gzip members whose total size its trailer does
not give, a reference file that keeps no record; in strict mode reference keys
that are not strictly increasing or a repeated key (DeviceIngestKeys); in
general mode a file of more than 2^31 - 3 lines -- raises
DeviceIngestUnsupported and the caller reads the cohort with the host parser
(ingest.cpp), which covers every case the reference reads.  A file that does
not inflate (corrupt, truncated, not gzip) is dropped as the reference drops
it.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from collections.abc import Sequence
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _abi
from .._abi import MdOpts, call
# the batch layer shared with the coverage and step 5's read; device.py, tools and tests reach some through here
from .gz_batch import (CH, READ_THREADS, _STAGING, align, chunk_table, fold_members, gpu_inflate,  # noqa: F401
                       member_units, release_staging, staging, staging_bytes, whole_units)
_chunks, _staging = chunk_table, staging    # their names before gz_batch

BATCH_IN = 4 << 30              # compressed bytes per batch
BATCH_TEXT = 24 << 30           # inflated bytes per batch
FIRST_BATCH_IN = 256 << 20      # the first batch (read and inflated synchronously: the reference key list)
PIPELINE = True                 # BGZF batches after the first: enqueued without host round trips (_Async)
STAGE = 1 << 30                 # pinned staging per CPU sub-batch (two of them)
TRACE = bool(os.environ.get("GRID_INGEST_TRACE"))   # per-batch phase times on stderr
XSTREAM_WAIT = True             # dev's stream waits for the copy stream (False only in a GPU test's control arm)
AFTER_HOST_TEXT = None          # test seam: called (dev, d_text, toff, files) once host text is in HBM
# pipelined BGZF batches: the fraction of each batch's files the host threads
# inflate beside the GPU (every k-th file; 0 = the GPU inflates all).  With 16
# host threads beside the MI355X's 37 GB/s, config-2 ingest (r04y, kept
# staging): 0.15 9.9 s, 0.2 9.5 s, 0.25 9.1-9.25 s, 0.33 9.3-9.6 s
HOST_FRAC = float(os.environ.get("GRID_INGEST_HOST_FRAC", "0.25"))
# the host share is sized from the config's `threads` (the
# reference defaults to 1 thread, its example config uses 4): the host files
# take as long as the GPU's when f / (t H) = (1 - f) / G, so f = t H / (G + t H)
# with H one thread's inflate rate beside the GPU and G the GPU's; 0.25 at 16
# threads (the r04ae optimum) gives H ~ 0.77 GB/s at G ~ 37 GB/s.  Round 5's
# inflate runs at G ~ 63 GB/s (r05ag), where the model's 16 % at 16 threads
# measured slower than none (config 2 ingest 6.34 vs 6.04 s, r05ah: the host
# reads, copies and checks its files beside the batch and they no longer hide
# under the GPU's part); below one file in 5 the share is not used
HOST_RATE_PER_THREAD = 0.77e9
GPU_INFLATE_RATE = 63e9          # r05ag: BGZF members (tools/bench_inflate.py --bgzf --units)
HOST_FRAC_MIN = 0.2


def host_frac(threads):
    """Fraction of a pipelined batch's BGZF files the host threads inflate."""
    t = max(1, int(threads))
    f = t * HOST_RATE_PER_THREAD / (GPU_INFLATE_RATE + t * HOST_RATE_PER_THREAD)
    f = min(f, HOST_FRAC)
    return f if f >= HOST_FRAC_MIN else 0.0


class DeviceIngestUnsupported(Exception):
    """The cohort leaves the device parser's common case (see the module doc)."""


class DeviceIngestKeys(DeviceIngestUnsupported):
    """Strict key mode only: the reference file's keys are not strictly
    increasing, or a file repeats a key -- what the general key mode reads."""


KEY_MODES = ("strict", "general")


def _trace(fmt, *args):
    """Phase times on stderr (GRID_INGEST_TRACE)."""
    if TRACE:
        print("[ingest] " + fmt.format(*args), file=sys.stderr, flush=True)


def _flag_reason(flags):
    """Why a file's parse flags hand the cohort over."""
    if flags & _abi.MD_EXOTIC:
        return "a line outside the mosdepth grammar"
    if flags & _abi.MD_NOTINK:
        return "a key outside K"
    return "more than 2^31 - 3 lines (general keys)"


def _opts(dev, prefix, window, excluded, keep):
    pre = (prefix or "").encode()
    d_pre = dev.upload(np.frombuffer(pre or b"\0", np.uint8))
    names = sorted(excluded or {})
    nb = [n.encode() for n in names]
    noff = np.zeros(len(nb) + 1, np.int32)
    noff[1:] = np.cumsum([len(b) for b in nb]) if nb else []
    kb = [np.unique(np.fromiter(excluded[n], dtype=np.int64, count=len(excluded[n]))) for n in names]
    koff = np.zeros(len(kb) + 1, np.int64)
    koff[1:] = np.cumsum([len(k) for k in kb]) if kb else []
    d_names = dev.upload(np.frombuffer(b"".join(nb) or b"\0", np.uint8))
    d_noff, d_koff = dev.upload(noff), dev.upload(koff)
    d_kb = dev.upload(np.concatenate(kb) if kb and koff[-1] else np.zeros(1, np.int64))
    keep += [d_pre, d_names, d_noff, d_koff, d_kb]
    s, e = window if window else (0, 0)
    return MdOpts(d_pre.ptr, len(pre), 1 if window else 0, int(s), int(e), len(names), 0, d_names.ptr, d_noff.ptr,
                  d_koff.ptr, d_kb.ptr)


class _Split:
    """Which files of a batch the GPU inflates and which the CPU threads do,
    from rates measured on the previous batches (initial values: MI355X with
    16 host threads, tools/bench_inflate.py): the GPU's aggregate text rate
    over BGZF members, one wave's rate on a whole single-member file, and one
    CPU thread's rate.  Greedy, largest file first, to the side that would
    finish sooner."""

    def __init__(self, threads):
        self.threads = max(1, int(threads))
        self.gpu = 18.0e9         # B/s, member-parallel, as seen by a batch (beside its disk reads; learned)
        self.wave = 9.0e6         # B/s, one wave on one whole file
        self.cpu = 0.4e9          # B/s per thread while the GPU inflates too (0.6-0.7 alone)

    def plan(self, files, text, bgzf):
        """BGZF files all go to the GPU: with the member-parallel inflate at
        ~18 GB/s of text the host threads (~10 GB/s alone) only slow both sides
        down when they run beside it -- host memory traffic of their text and
        stage copies (1,024 files: GPU alone 7.1 s, split 8.3 s; config 2:
        split 30.0 s, profiles/r03o_*, r03p_*).  Single-member files (a serial
        stream each) go to whichever side the rates say."""
        if all(bgzf[k] for k in files):
            return sorted(files), []
        g_mem = g_whole = c = 0.0
        gpu, cpu = [], []
        for k in sorted(files, key=lambda k: -int(text[k])):
            s = float(text[k])
            tg = max((g_mem + s) / self.gpu, g_whole) if bgzf[k] else max(g_mem / self.gpu, g_whole, s / self.wave)
            tc = (c + s) / (self.cpu * self.threads)
            cur_g = max(g_mem / self.gpu, g_whole)
            cur_c = c / (self.cpu * self.threads)
            if max(tg, cur_c) <= max(cur_g, tc):
                gpu.append(k)
                if bgzf[k]:
                    g_mem += s
                else:
                    g_whole = max(g_whole, s / self.wave)
            else:
                cpu.append(k)
                c += s
        return sorted(gpu), sorted(cpu)

    def learn(self, g_mem_bytes, g_whole_max, t_gpu, c_bytes, t_cpu):
        a = 0.5                   # moving average over batches
        if t_gpu > 0.05:
            if g_mem_bytes and not g_whole_max:
                self.gpu = (1 - a) * self.gpu + a * g_mem_bytes / t_gpu
            elif g_whole_max and not g_mem_bytes:
                self.wave = (1 - a) * self.wave + a * g_whole_max / t_gpu
        if t_cpu > 0.05 and c_bytes:
            self.cpu = (1 - a) * self.cpu + a * c_bytes / (t_cpu * self.threads)


class _Async:
    """The device ingest's pipelined batches (every file BGZF, all inflated by
    the GPU; after the first batch, which builds the key list K synchronously).
    Per batch, with no host round trip:
      copy stream:  [wait: batch b-2's parse done] compressed input + the batch's
                    tables (member units, files, 16 KiB chunks: one pinned arena)
                    -> HBM (d_in / tables of parity b % 2); event h2d[b % 2];
      main stream:  [wait h2d] grid_gunzip_batch (inflate + CRC) -> grid_file_status
                    (files with a failed member are skipped by the parse, as the
                    reference drops them) -> grid_md_count -> grid_md_parse_map;
                    event done[b % 2].
    So batch b+1's 4 GB copy runs under batch b's inflate, and the host only
    builds tables.  A file's text length is the sum of its members' ISIZEs
    (the inflater checks every member against its ISIZE and CRC).  Statuses,
    lengths, flags and kept counts stay on the device per batch and are read
    once at the end (results)."""

    def __init__(self, dev, cdev, opts, K, nK, kidx, ref_nlines, Q, general=False):
        self.dev, self.cdev, self.opts = dev, cdev, opts
        # general keys: the tag and the resolve pass (one call, two launches back
        # to back on the stream, before `done`: the parity's text is still intact)
        self.parse_map = "grid_md_parse_map_general" if general else "grid_md_parse_map"
        self.K, self.nK, self.kidx, self.ref_nlines, self.Q = K, nK, kidx, ref_nlines, Q
        self.h2d = [_abi.Event(), _abi.Event()]
        self.done = [_abi.Event(), _abi.Event()]
        self.issued = [False, False]
        self.arena_h = [staging("arena0", 64 << 20), staging("arena1", 64 << 20)]
        self.arena_d = [None, None]
        self.scr = [None, None]                 # per parity: member table, chunk counts/lines, file status
        self.out = []                           # per batch: (fs, owner, unit status, unit length, flags, kept, okb)
        self.htext = [_abi.Event(), _abi.Event()]   # host-inflated text of parity p is in HBM
        self.hbad = []                          # host-share files whose text failed its CRC in HBM
        self.one = None                         # page-locked int32 1: a failed host-share file's device status

    def batch(self, bi, fs, buf, off, caps_, gz, members, toff, d_in, d_text, fsizes, hshare=None):
        """hshare: (files, future) -- files of the batch the host threads inflate
        (the future returns per file (status, length, crc, staging, offset));
        their text is copied into d_text once the previous batch's parse is done
        and checked there against its gzip CRC on the copy stream, while the
        GPU inflates the rest; the parse waits for the copy (event htext)."""
        dev, cdev, p = self.dev, self.cdev, bi % 2
        nb = len(fs)
        mu = [k for k in range(nb) if gz[k] and fsizes[k] > 0 and members[k] is not None]
        hset = set(hshare[0]) if hshare else set()
        units = list(member_units(members, off, toff, [k for k in mu if k not in hset]))
        nu = len(units[0])
        tlen = np.zeros(nb, np.int64)               # text of a file that inflates: its members' ISIZEs
        for k in mu:
            tlen[k] = int(members[k][2].astype(np.int64).sum())
        okb = [k for k in mu if tlen[k] > 0]
        cfile, cstart, cfirst, nch = chunk_table(okb, tlen)
        parts = units + [tlen, np.ascontiguousarray(toff[:nb]), np.asarray(fs, np.int32), cfile, cstart, cfirst]
        sz = align(np.array([a.nbytes for a in parts]))       # one arena, every table 256-aligned
        offs, nbytes = (np.cumsum(sz) - sz).tolist(), int(sz.sum())
        # the arena of parity p: its previous copy (batch bi-2) must be done
        if self.issued[p]:
            self.h2d[p].host_wait()
        host = self.arena_h[p].get(nbytes + 256)
        for a, o in zip(parts, offs):
            host[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        if self.arena_d[p] is None or self.arena_d[p].nbytes < nbytes + 256:
            self.drain()
            self.arena_d[p] = None
            self.arena_d[p] = dev.alloc(max(nbytes + 256, 16 << 20) * 5 // 4, np.uint8)
        need = (nu * _abi.GZ_MEMBER_BYTES, nu * 4, nch * 4, nch * 8, nb * 4)
        sc = self.scr[p]
        if sc is None or any(b.nbytes < n + 256 for b, n in zip(sc, need)):
            self.drain()
            self.scr[p] = None
            self.scr[p] = sc = [dev.alloc(max(n + 256, 4096) * 5 // 4, np.uint8) for n in need]
        mem, unm, cnl, cline0, fst = sc
        # per-batch outputs read at the end (small)
        ust, uln = dev.alloc(max(nu, 1), np.int32), dev.alloc(max(nu, 1), np.int64)
        bflags, bk = dev.zeros(nb, np.int32), dev.zeros(nb, np.uint64)
        # copy context: after batch bi-2's parse (same parity buffers), the input
        # and the tables, from pageable staging (the call returns once they are in
        # HBM; it runs while the device inflates batch bi-1)
        if self.issued[p]:
            self.done[p].host_wait()
        call("grid_h2d", cdev.ctx, d_in.ptr, buf.ctypes.data, int(off[-1]))
        call("grid_h2d", cdev.ctx, self.arena_d[p].ptr, host.ctypes.data, nbytes)
        self.h2d[p].put(cdev)
        # main stream
        self.h2d[p].wait(dev)
        A = self.arena_d[p].ptr
        d_uo, d_ul, d_to, d_tc, d_own, d_tl, d_toff, d_qrow, d_cf, d_cs, d_c1 = (A + o for o in offs)
        if nu:
            call("grid_gunzip_batch", dev.ctx, d_in.ptr, d_uo, d_ul, nu, d_text.ptr, d_to, d_tc, mem.ptr, 1,
                 ust.ptr, uln.ptr, unm.ptr)
        hfail = []
        if hset:
            res = hshare[1].result()
            # the previous batch's parse reads d_text: its regions are free once it is done
            q = 1 - p
            if self.issued[q]:
                self.done[q].host_wait()
            hk = []
            for k in sorted(hset):
                st_, ln_, crc_, stage, so = res[k]
                if st_ != 0 or ln_ != tlen[k]:
                    hfail.append(k)              # dropped, as a file with a failed member on the GPU
                    continue
                if ln_:
                    call("grid_h2d", cdev.ctx, d_text.ptr + int(toff[k]), stage.ctypes.data + int(so), int(ln_))
                    hk.append(k)
            self.htext[p].put(cdev)
            self.htext[p].wait(dev)
            if hk and AFTER_HOST_TEXT is not None:
                AFTER_HOST_TEXT(cdev, d_text, toff, hk)
            if hk:
                # the guard, on the copy stream (it wrote the text): a mismatch hands
                # the cohort to the host parser once the batches are done
                got = _abi.text_crc32(cdev, d_text.ptr, toff[hk], tlen[hk])
                for k, c in zip(hk, got):
                    if int(c) != int(res[k][2]):
                        self.hbad.append((fs[k], "its text in HBM does not match its gzip CRC"))
        call("grid_file_status", dev.ctx, ust.ptr, d_own, nu, fst.ptr, nb)
        if hfail:
            # the parse skips them: their device status set after grid_file_status (stream order)
            if self.one is None:
                self.one = _abi.PinnedBuf(64)
                self.one.array[:4] = np.array([1], np.int32).view(np.uint8)
            for k in hfail:
                call("grid_h2d_async", dev.ctx, fst.ptr + 4 * k, self.one.ptr, 4)
        if nch:
            call("grid_md_count", dev.ctx, d_text.ptr, d_toff, d_tl, nch, d_cf, d_cs, d_c1, len(okb), cnl.ptr,
                 cline0.ptr, bflags.ptr, fst.ptr)
            call(self.parse_map, dev.ctx, d_text.ptr, d_toff, d_tl, nch, d_cf, d_cs, cline0.ptr,
                 C.byref(self.opts), bflags.ptr, self.K.ptr, self.nK, self.kidx.ptr, self.ref_nlines, self.Q.ptr,
                 self.nK, d_qrow, bk.ptr, fst.ptr)
        self.done[p].put(dev)
        self.issued[p] = True
        # not gzip at all: dropped (GZ_EHEADER in the synchronous path)
        hdr_bad = [k for k in range(nb) if not gz[k] and fsizes[k] > 0]
        self.out.append((list(fs), units[4], ust, uln, bflags, bk, okb, nu, hdr_bad, hfail))
        return self.h2d[p]

    def drain(self):
        self.dev.sync()
        self.cdev.sync()

    def results(self, paths):
        """(file, status 0/1, kept) per file of the pipelined batches; raises
        DeviceIngestUnsupported for a parse flag, as the synchronous path."""
        if self.hbad:
            f, why = self.hbad[0]
            raise DeviceIngestUnsupported(f"{paths[f]}: {why} ({len(self.hbad)} host-inflated file(s))")
        res = []
        self.kept = []
        for fs, owner, ust, uln, bflags, bk, okb, nu, hdr_bad, hfail in self.out:
            nb = len(fs)
            bad = np.zeros(nb, np.int32)
            bad[hdr_bad] = _abi.GZ_EHEADER
            bad[hfail] = _abi.GZ_EDATA
            if nu:
                np.maximum(bad, fold_members(nb, owner, ust.numpy()[:nu])[0], out=bad)
            bf, bkv = bflags.numpy(), bk.numpy()
            for k in okb:
                if bad[k] == 0 and bf[k]:
                    raise DeviceIngestUnsupported(f"{paths[fs[k]]}: {_flag_reason(int(bf[k]))}")
            for k, f in enumerate(fs):
                res.append((f, 0 if bad[k] == 0 else 1, int(bkv[k])))
            self.kept.append((np.asarray(fs), bkv))
        return res

    def kept_total(self, nfiles):
        tot = np.zeros(max(nfiles, 1), np.uint64)
        for fs, bkv in self.kept:
            tot[fs] += bkv
        return tot

    def close(self):
        try:
            self.drain()
        finally:
            if self.one is not None:
                self.one.free()
                self.one = None
            self.out = []
            self.arena_d = [None, None]
            self.scr = [None, None]


class _Host:
    """The host side of one ingest, shared by its batches: the thread pools,
    the staging, the copy context and the GPU/CPU split."""

    def __init__(self, dev, paths, sizes, batches, threads):
        self.dev, self.paths, self.sizes, self.batches = dev, paths, sizes, batches
        self.pins = [staging("in0", BATCH_IN + 512), staging("in1", BATCH_IN + 512)]
        self.first = staging("first", FIRST_BATCH_IN + 512)        # the (small) first batch: K, quickly
        self.stages = [staging("text0", STAGE + 512, pinned=True), staging("text1", STAGE + 512, pinned=True)]
        nthreads = max(1, min(int(threads or 1), 32))
        self.pool = ThreadPoolExecutor(nthreads)   # host inflate (the host share, non-BGZF files)
        self.iopool = ThreadPoolExecutor(max(1, READ_THREADS))   # file reads + member tables
        self.rpool = ThreadPoolExecutor(1)         # the next batch's read (its files on `iopool`)
        self.hfrac = host_frac(nthreads)
        self.copier = ThreadPoolExecutor(1)        # H2D of CPU-inflated text, on its own stream
        self.waiter = ThreadPoolExecutor(1)        # notes when the GPU's inflate ends
        self.hctl = ThreadPoolExecutor(1)          # pipelined batches: the host share's inflate (its files on `pool`)
        self.hstages = [staging("host0", 8 << 30), staging("host1", 8 << 30)]
        self.cdev = _abi.Device(dev.index)         # its own non-blocking stream
        self.split = _Split(nthreads)
        self.h2d_done = [None] * len(batches)      # per pipelined batch: the event after its copies to HBM

    def close(self):
        for p in (self.rpool, self.iopool, self.pool, self.copier, self.waiter, self.hctl):
            p.shutdown(wait=True)
        self.cdev.close()

    def read(self, bi):
        """Batch bi's files read into staging: (the buffer, the files' offsets in
        it, per file (text size, members) or None, per file its BGZF members or None)."""
        fs, sizes, paths = self.batches[bi], self.sizes, self.paths
        off = np.zeros(len(fs) + 1, np.int64)
        off[1:] = np.cumsum(align(np.maximum(sizes[fs], 1)))
        if bi >= 2 and self.h2d_done[bi - 2] is not None:
            self.h2d_done[bi - 2].host_wait()        # pins[bi % 2] still feeds batch bi-2's copy
        buf = (self.first if bi == 0 else self.pins[bi % 2]).get(int(off[-1]) + 256)

        def one(k):
            f = fs[k]
            with open(paths[f], "rb") as fh:
                n = fh.readinto(memoryview(buf)[off[k]:off[k] + sizes[f]])
            if n != sizes[f]:
                raise DeviceIngestUnsupported(f"{paths[f]} changed while reading")
            if not sizes[f]:
                return (0, 0), None
            v = buf[off[k]:off[k] + sizes[f]]
            return _abi.gz_text_size(v), _abi.gz_members(v)
        info = list(self.iopool.map(one, range(len(fs))))
        return buf, off, [i[0] for i in info], [i[1] for i in info]

    def share(self, bi, todo, buf, off, fs, caps_):
        """A pipelined batch's host share as _Async.batch takes it (None: the GPU
        inflates all): every step-th file to the host threads, which start now,
        beside the GPU's work on the previous batch and this batch's copies."""
        if not (self.hfrac > 0 and len(todo) > 1):
            return None
        step = max(2, int(round(1.0 / self.hfrac)))
        hfiles = todo[step - 1::step]
        so, pos = {}, 0
        for k in hfiles:
            so[k] = pos
            pos += align(int(caps_[k]))
        harr = self.hstages[bi % 2].get(pos + 256)

        def one(k):
            v = buf[off[k]:off[k] + self.sizes[fs[k]]]
            st_, ln_, crc_ = _abi.gunzip_host(v, harr[so[k]:so[k] + int(caps_[k])], with_crc=True)
            return k, (int(st_), int(ln_), int(crc_), harr, so[k])
        return hfiles, self.hctl.submit(lambda: dict(self.pool.map(one, hfiles)))

    def inflate(self, buf, off, fs, caps_, gz, members, toff, d_in, d_text, plan):
        """Inflate the batch's files into d_text + toff[k], the GPU's and the
        CPU's (``plan``) at once; (status, length) per file."""
        dev, cdev, sizes, fsz, nb = self.dev, self.cdev, self.sizes, self.sizes[fs], len(fs)
        # an empty file: no lines (gzip.open reads nothing); not gzip: dropped
        gst = np.where((fsz > 0) & ~gz, _abi.GZ_EHEADER, 0).astype(np.int32)
        tlen, hcrc = np.zeros(nb, np.int64), np.zeros(nb, np.uint32)
        on_gpu, on_cpu = plan
        t0 = time.perf_counter()
        launched = []                                  # (files, each unit's file or None, gpu_inflate's buffers)
        if on_gpu:
            call("grid_h2d", dev.ctx, d_in.ptr, buf.ctypes.data, int(off[-1]))
            mu = [k for k in on_gpu if members[k] is not None]
            wu = [k for k in on_gpu if members[k] is None]
            if wu:                                     # whole files: one wave each, started first
                units, mcap = whole_units(off, fsz, toff, caps_, wu)
                launched.append((wu, None, gpu_inflate(dev, d_in, d_text, units, mcap)))
            if mu:                                     # BGZF: one wave per member
                units = member_units(members, off, toff, mu)
                launched.append((mu, units[4], gpu_inflate(dev, d_in, d_text, units[:4], 1)))
            gpu_done = self.waiter.submit(lambda: (dev.sync(), time.perf_counter())[1])
        # CPU files meanwhile: sub-batches through two pinned stages, each
        # copied to HBM on the copy stream while the next one inflates
        pend = [None, None]
        c_bytes = i = sb = 0
        while i < len(on_cpu):
            grp, room = [], 0
            while i < len(on_cpu) and (not grp or room + align(caps_[on_cpu[i]]) <= STAGE):
                grp.append(on_cpu[i])
                room += align(caps_[on_cpu[i]])
                i += 1
            j = sb % 2
            sb += 1
            if pend[j] is not None:
                pend[j].result()
            stage = self.stages[j].get(room + 256)
            soff = np.zeros(len(grp) + 1, np.int64)
            soff[1:] = np.cumsum(align(caps_[grp]))

            def one(t, grp=grp, stage=stage, soff=soff):
                k = grp[t]
                v = buf[off[k]:off[k] + sizes[fs[k]]]
                return _abi.gunzip_host(v, stage[soff[t]:soff[t] + caps_[k]], with_crc=True)
            res = list(self.pool.map(one, range(len(grp))))
            for t, k in enumerate(grp):
                gst[k], tlen[k], hcrc[k] = res[t]
                c_bytes += int(tlen[k])

            def h2d(grp=grp, stage=stage, soff=soff, res=res):
                for t, k in enumerate(grp):
                    if res[t][0] == 0 and res[t][1]:
                        call("grid_h2d", cdev.ctx, d_text.ptr + int(toff[k]), stage.ctypes.data + int(soff[t]),
                             int(res[t][1]))
            pend[j] = self.copier.submit(h2d)
        t_cpu = time.perf_counter() - t0
        for p_ in filter(None, pend):
            p_.result()
        if on_cpu and XSTREAM_WAIT:
            # the parse kernels on dev's stream read text the copy stream wrote
            # over d_text -- lines the previous batch's kernels had cached: order
            # the stream behind the copies through the runtime (event + wait), not
            # through the host's view of their completion alone
            call("grid_stream_after", dev.ctx, cdev.ctx)
        hk = [k for k in on_cpu if gst[k] == 0 and tlen[k] > 0]
        if hk:
            # the guard: the host-inflated text as it sits in HBM against the CRC
            # of its gzip trailers, read on dev's stream (where the parse runs)
            if AFTER_HOST_TEXT is not None:
                AFTER_HOST_TEXT(dev, d_text, toff, hk)
            got = _abi.text_crc32(dev, d_text.ptr, toff[hk], tlen[hk])
            bad = [fs[k] for k, c in zip(hk, got) if int(c) != int(hcrc[k])]
            if bad:
                raise DeviceIngestUnsupported(f"{self.paths[bad[0]]}: its text in HBM does not match its gzip CRC "
                                              f"({len(bad)} host-inflated file(s))")
        g_mem, g_whole, t_gpu = 0, 0, 0.0
        if launched:
            t_gpu = gpu_done.result() - t0
            for ks, owner, (_d, _mem, st, ln, _nm) in launched:
                ust, uln = st.numpy(), ln.numpy()
                if owner is None:
                    gst[ks], tlen[ks] = ust, uln
                    g_whole = max(g_whole, int(uln.max()))
                else:
                    bad, tot = fold_members(nb, owner, ust, uln)
                    gst[ks], tlen[ks] = bad[ks], tot[ks]
                    g_mem += int(uln.sum())
        self.split.learn(g_mem, g_whole, t_gpu, c_bytes, t_cpu)
        _trace("batch files gpu {} cpu {} text gpu {:.3e} cpu {:.3e} B  t_gpu {:.3f} t_cpu {:.3f} s  rates gpu {:.3e} "
               "cpu/thread {:.3e} B/s", len(on_gpu), len(on_cpu), g_mem + g_whole, c_bytes, t_gpu, t_cpu,
               self.split.gpu, self.split.cpu)
        return gst, tlen


def _reference_keys(dev, opts, general, paths, fs, okb, tlen, toff, chunks, cnl, cline0, d_text, d_toff, d_tl, bflags):
    """(K, kidx, nK, ref_nlines) from the first batch with text.  The reference
    file is the one with the most text (a short or truncated
    file sorted first no longer sends the cohort to the host parser; K must hold
    every later file's keys, which the largest file does).  ``chunks``: the
    batch's chunk_table; cnl, cline0: grid_md_count's lines per chunk."""
    _cfile, cstart, cfirst, _nch = chunks
    ri = int(np.argmax(tlen[okb]))
    r = okb[ri]
    c0, c1 = int(cfirst[ri]), int(cfirst[ri + 1])
    rc_file = np.zeros(c1 - c0, np.int32) + r
    cl, nl = cline0.numpy()[c0:c1], cnl.numpy()[c0:c1]
    tail = np.zeros(1, np.uint8)
    call("grid_d2h", dev.ctx, tail.ctypes.data, d_text.ptr + int(toff[r] + tlen[r] - 1), 1)
    ref_nlines = int(cl[-1] + nl[-1]) + (0 if tail[0] == 10 else 1)
    nr = max(ref_nlines, 1)
    kline, keys_line = dev.alloc(nr, np.uint8), dev.alloc((nr, 2), np.int64)
    K, kidx = dev.alloc((nr, 2), np.int64), dev.alloc(nr, np.int32)
    h_nK, h_uns = C.c_int64(), C.c_int32()
    d_rcf, d_rcs, d_rcl = dev.upload(rc_file), dev.upload(cstart[c0:c1]), dev.upload(cl)
    if general:
        if ref_nlines >= 1 << 31:
            raise DeviceIngestUnsupported(f"{paths[fs[r]]}: {_flag_reason(_abi.MD_LINES)}")
        # K: the kept keys sorted and de-duplicated, any order, any repeats
        call("grid_md_parse_ref_general", dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, c1 - c0, d_rcf.ptr,
             d_rcs.ptr, d_rcl.ptr, C.byref(opts), bflags.ptr, ref_nlines,
             kline.ptr, keys_line.ptr, K.ptr, kidx.ptr, C.byref(h_nK))
    else:
        call("grid_md_parse_ref", dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, c1 - c0, d_rcf.ptr,
             d_rcs.ptr, d_rcl.ptr, C.byref(opts), bflags.ptr, ref_nlines,
             kline.ptr, keys_line.ptr, K.ptr, kidx.ptr, C.byref(h_nK), C.byref(h_uns))
    if h_uns.value:
        raise DeviceIngestKeys("the reference file's keys are not strictly increasing")
    if h_nK.value == 0:
        raise DeviceIngestUnsupported("the reference file keeps no record")
    return K, kidx, h_nK.value, ref_nlines


def _finish(dev, Q, nK, K, kept, status, nfiles, min_depth, max_depth, general, t_start):
    """grid_md_finish over the placed matrix (means, valid columns, empty-sample filter): the full result."""
    rows = np.array([f for f in range(nfiles) if status[f] == 0], np.int32)
    mean, valid, cpos = dev.alloc(nK, np.float64), dev.alloc(nK, np.int32), dev.alloc(nK, np.int64)
    present, nvalid = dev.alloc(max(nfiles, 1), np.uint64), dev.alloc(max(nfiles, 1), np.uint64)
    m = C.c_int64()
    _trace("finish buffers at {:.3f} s", time.perf_counter() - t_start)
    d_rows = dev.upload(rows if rows.size else np.zeros(1, np.int32))
    call("grid_md_finish", dev.ctx, Q.ptr, nK, nK, nfiles, d_rows.ptr, len(rows), float(min_depth),
         float(max_depth), mean.ptr, valid.ptr, cpos.ptr, present.ptr, nvalid.ptr, C.byref(m))
    pres, nval, kh = present.numpy()[:nfiles], nvalid.numpy()[:nfiles], kept.numpy()[:nfiles]
    if np.any(pres[rows] != kh[rows]):
        if general:
            # the integrity guard: every present cell was filled by exactly one line's resolve
            raise DeviceIngestUnsupported("an unresolved cell in a file's row (general keys)")
        raise DeviceIngestKeys("a repeated (start, end) key in a file")
    _trace("finish done at {:.3f} s", time.perf_counter() - t_start)
    return rows, (Q, nK, valid, cpos, K, m.value), nval, status


def ingest_device(dev, paths, prefix, window, excluded, min_depth, max_depth, threads=16, ref=None,
                  keys_only=False, finish=True, keys="strict"):
    """paths: one per individual in file order (None = no file).  Returns
    (ok files in file order, the device state for ``gather``, records in valid
    columns per file, status per file: 0 ok, 1 failed, 3 missing); raises
    DeviceIngestUnsupported.

    The distributed step 4 (dist_step4.py) splits this in two: rank 0 runs
    ``keys_only`` (the first batch only: the reference key list K as host
    arrays (K [nK][2] int64, kidx int32, ref_nlines), or None when no file
    inflates), every rank then parses its slice of the files over that K
    (``ref``) with ``finish=False``: (Q [nfiles][nK] int32 on the device, nK,
    status, records kept per file) -- the population means are a chain over
    the ranks there.

    keys: "strict" (the reference file's keys strictly increasing, no key
    repeated in a file, else DeviceIngestKeys) or "general" (any order, any
    repeats: sorted unique columns, the last kept line of a key wins; see the
    module doc).  ``keys_only`` and ``ref`` work in either mode, and a ``ref``
    from one mode must be parsed in the same mode."""
    if keys not in KEY_MODES:
        raise ValueError(f"keys must be one of {KEY_MODES}, not {keys!r}")
    general = keys == "general"
    parse_map = "grid_md_parse_map_general" if general else "grid_md_parse_map"
    nfiles = len(paths)
    t_start = time.perf_counter()
    keep = []
    opts = _opts(dev, prefix, window, excluded, keep)
    sizes = np.array([os.path.getsize(p) if p else -1 for p in paths], np.int64)
    status = np.where(sizes < 0, 3, 0).astype(np.int32)       # 3: missing (ingest.cpp FS_MISSING)
    kept = dev.zeros(max(nfiles, 1), np.uint64)
    batches, cur, cin = [], [], 0                              # batches in file order
    for f in np.flatnonzero(sizes >= 0).tolist():
        lim = min(FIRST_BATCH_IN, BATCH_IN) if not batches and ref is None else BATCH_IN
        if cur and cin + align(sizes[f]) > lim:
            batches.append(cur)
            cur, cin = [], 0
        cur.append(f)
        cin += align(sizes[f])
    if cur:
        batches.append(cur)
    in_need = 256 + max((int(align(np.maximum(sizes[b], 1)).sum()) for b in batches), default=0)
    host = _Host(dev, paths, sizes, batches, threads)
    K = kidx = Q = None
    nK = ref_nlines = 0
    if ref is not None:                    # the key list of another rank's reference file
        K_h, kidx_h, ref_nlines = ref
        nK = len(K_h)
        K = dev.upload(np.ascontiguousarray(K_h, np.int64).reshape(max(nK, 1), 2) if nK else np.zeros((1, 2), np.int64))
        kidx = dev.upload(np.ascontiguousarray(kidx_h, np.int32) if len(kidx_h) else np.zeros(1, np.int32))
        ref_nlines = int(ref_nlines)
        Q = dev.alloc((max(nfiles, 1), max(nK, 1)), np.int32)
        call("grid_fill_i32", dev.ctx, Q.ptr, max(nfiles, 1) * max(nK, 1), _abi.MISSING)
    d_text, d_ins, pipe = None, [None, None], None
    pending = host.rpool.submit(host.read, 0) if batches else None
    try:
        for bi, fs in enumerate(batches):
            t_w = time.perf_counter()
            buf, off, caps, members = pending.result()
            pending = host.rpool.submit(host.read, bi + 1) if bi + 1 < len(batches) else None
            nb = len(fs)
            caps_ = np.array([c[0] if c else 0 for c in caps], np.int64)
            gz = np.array([c is not None for c in caps])
            toff = np.zeros(nb + 1, np.int64)
            toff[1:] = np.cumsum(align(np.maximum(caps_, 1)))
            if toff[-1] > BATCH_TEXT * 2:
                raise DeviceIngestUnsupported("a batch of files inflates beyond the device text buffer")
            # device buffers sized from the cohort, not from the batch bounds: the
            # compressed bytes of the largest batch (known from the file sizes), the
            # text grown with 1/8 headroom as batches need it
            if d_ins[bi % 2] is None or d_ins[bi % 2].nbytes < off[-1] + 256:
                if pipe is not None:
                    pipe.drain()
                d_ins[bi % 2] = None
                d_ins[bi % 2] = dev.cached(f"ingest_in{bi % 2}", in_need if bi else int(off[-1]) + 256)
            if d_text is None or d_text.nbytes < toff[-1] + 256:
                if pipe is not None:
                    pipe.drain()
                d_text = None
                d_text = dev.cached("ingest_text", int(min(toff[-1] + 256 + toff[-1] // 8, 2 * BATCH_TEXT + 256)))
            d_in = d_ins[bi % 2]
            todo = [k for k in range(nb) if gz[k] and sizes[fs[k]] > 0]
            bgzf = {k: members[k] is not None for k in todo}
            plan = host.split.plan(todo, caps_, bgzf)
            if PIPELINE and K is not None and all(bgzf.values()) and not plan[1]:
                # every file BGZF (what mosdepth writes): the GPU inflates all of
                # them, and the batch is enqueued behind the previous one
                if pipe is None:
                    pipe = _Async(dev, host.cdev, opts, K, nK, kidx, ref_nlines, Q, general=general)
                host.h2d_done[bi] = pipe.batch(bi, fs, buf, off, caps_, gz, members, toff, d_in, d_text,
                                               [sizes[f] for f in fs],
                                               hshare=host.share(bi, todo, buf, off, fs, caps_))
                _trace("batch {}: {} files enqueued, wait read {:.3f} s (at {:.3f})", bi, nb,
                       time.perf_counter() - t_w, time.perf_counter() - t_start)
                continue
            if pipe is not None:
                pipe.drain()
            t_b = time.perf_counter()
            gst, tlen = host.inflate(buf, off, fs, caps_, gz, members, toff, d_in, d_text, plan)
            t_i = time.perf_counter()
            for k, f in enumerate(fs):
                if gst[k] == _abi.GZ_ESPACE:
                    raise DeviceIngestUnsupported(f"{paths[f]}: several gzip members (text size unknown)")
                status[f] = 0 if gst[k] == 0 else 1        # 1: failed (the reference drops the sample)
            okb = [k for k in range(nb) if gst[k] == 0 and tlen[k] > 0]
            chunks = cfile, cstart, cfirst, nch = chunk_table(okb, tlen)
            if nch == 0:
                continue
            d_tl, d_toff = dev.upload(tlen), dev.upload(toff[:nb])
            d_cfile, d_cstart, d_cfirst = dev.upload(cfile), dev.upload(cstart), dev.upload(cfirst)
            cnl, cline0 = dev.alloc(nch, np.int32), dev.alloc(nch, np.int64)
            # flags per batch file, folded into the cohort's afterwards
            bflags = dev.zeros(nb, np.int32)
            call("grid_md_count", dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, nch, d_cfile.ptr, d_cstart.ptr,
                 d_cfirst.ptr, len(okb), cnl.ptr, cline0.ptr, bflags.ptr, None)
            if K is None:
                K, kidx, nK, ref_nlines = _reference_keys(dev, opts, general, paths, fs, okb, tlen, toff, chunks, cnl,
                                                          cline0, d_text, d_toff, d_tl, bflags)
                if keys_only:
                    break
                Q = dev.alloc((nfiles, nK), np.int32)
                call("grid_fill_i32", dev.ctx, Q.ptr, nfiles * nK, _abi.MISSING)
            qrow = dev.upload(np.asarray(fs, np.int32))
            bk = dev.zeros(nb, np.uint64)
            call(parse_map, dev.ctx, d_text.ptr, d_toff.ptr, d_tl.ptr, nch, d_cfile.ptr, d_cstart.ptr,
                 cline0.ptr, C.byref(opts), bflags.ptr, K.ptr, nK, kidx.ptr, ref_nlines, Q.ptr, nK, qrow.ptr, bk.ptr,
                 None)
            bf, bkv = bflags.numpy(), bk.numpy()
            for k in okb:
                if bf[k]:
                    raise DeviceIngestUnsupported(f"{paths[fs[k]]}: {_flag_reason(int(bf[k]))}")
            kept_h = kept.numpy()
            kept_h[np.asarray(fs)] += bkv
            kept.copy_from(kept_h)
            _trace("batch {}: {} files, wait read {:.3f} inflate {:.3f} parse {:.3f} s (at {:.3f})", bi, nb, t_b - t_w,
                   t_i - t_b, time.perf_counter() - t_i, time.perf_counter() - t_start)
        if pipe is not None:
            t_d = time.perf_counter()
            pipe.drain()
            for f, st_, kp in pipe.results(paths):
                status[f] = st_
            kept_h = kept.numpy()
            kept_h += pipe.kept_total(nfiles)
            kept.copy_from(kept_h)
            _trace("pipeline drained in {:.3f} s", time.perf_counter() - t_d)
    finally:
        if pending is not None:
            try:
                pending.result()
            except Exception:
                pass
        if pipe is not None:
            pipe.close()
        host.close()
    _trace("batches done (threads joined, copy context closed) at {:.3f} s", time.perf_counter() - t_start)
    # the batches' device buffers stay cached on the context (Device.cached,
    # names "ingest_*") and the host staging in _STAGING until
    # device.release_ingest_buffers() -- the end of the run or of a standalone
    # step 4 -- since their release holds the HIP runtime for a fraction of a
    # second; here only this function's references go
    d_ins = d_text = d_in = pipe = None
    _trace("input/text buffers freed at {:.3f} s", time.perf_counter() - t_start)
    if keys_only:
        return None if K is None else (K.numpy()[:nK].copy(), kidx.numpy()[:max(ref_nlines, 0)].copy(), ref_nlines)
    if not finish:
        return Q, nK, status, kept.numpy()[:nfiles].copy()
    if K is None:
        return [], [], None, status
    return _finish(dev, Q, nK, K, kept, status, nfiles, min_depth, max_depth, general, t_start)


class Regions(Sequence):
    """The valid columns' (start, end) pairs as a read-only sequence built on
    demand from two int64 arrays (a list of 3 M tuples costs ~1 s, and the
    step itself never needs it)."""

    def __init__(self, starts, ends):
        self.s, self.e = starts, ends

    def __len__(self):
        return len(self.s)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return list(zip(self.s[k].tolist(), self.e[k].tolist()))
        return int(self.s[k]), int(self.e[k])

    def __iter__(self):
        return zip(self.s.tolist(), self.e.tolist())

    def __eq__(self, other):
        try:
            return len(self) == len(other) and list(self) == list(other)
        except TypeError:
            return NotImplemented

    __hash__ = None


def gather(dev, state, row_files, nfiles):
    """The matrix rows of ``row_files`` (file indices, in output order) and
    the valid columns' (start, end)."""
    Q, nK, valid, cpos, K, m = state
    if m == nK and m > 0 and len(row_files) == nfiles and np.array_equal(np.asarray(row_files), np.arange(nfiles)):
        # every key valid and every file a row, already in output order: the
        # placed matrix IS the result (no 38 GB copy at config 2)
        kh = K.numpy()[:m]
        Q.shape = (nfiles, m)
        return Q, Regions(np.ascontiguousarray(kh[:, 0]), np.ascontiguousarray(kh[:, 1]))
    t0 = time.perf_counter()
    dst = np.full(max(nfiles, 1), -1, np.int32)
    dst[np.asarray(row_files, np.int64)] = np.arange(len(row_files), dtype=np.int32)
    out = dev.alloc((max(len(row_files), 1), max(m, 1)), np.int32)
    st, en = dev.alloc(max(m, 1), np.int64), dev.alloc(max(m, 1), np.int64)
    t1 = time.perf_counter()
    d_dst = dev.upload(dst)
    call("grid_md_gather", dev.ctx, Q.ptr, nK, nK, nfiles, valid.ptr, cpos.ptr, d_dst.ptr, out.ptr,
         max(m, 1), K.ptr, st.ptr, en.ptr)
    regions = Regions(st.numpy()[:m], en.numpy()[:m])
    _trace("gather: {} of {} rows, {} of {} columns; alloc {:.3f} s, gather {:.3f} s", len(row_files), nfiles, m, nK,
           t1 - t0, time.perf_counter() - t1)
    out.shape = (len(row_files), m)            # the allocation keeps >= 1 element
    return out, regions
