"""What the drivers of the device inflater share -- the step-4 ingest
(ingest_device.py), the region coverage (coverage_device.py) and step 5's
matrix read (ntext_device.py): the inflater's work list (``member_units``, one
wave per BGZF member; ``whole_units``, one per plain gzip file), its launch
(``gpu_inflate``) and the host fold of its results (``fold_members``); the
parse kernels' ``chunk_table``; ``align``, ``CH``, ``READ_THREADS``; and the
host staging kept between batches and runs.  The tables are NumPy alone.
bench.py (inflate_roofline) keeps a member table of its own: how pull requests
are measured does not change with the code it measures.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _abi
from .._abi import call

CH = 16384                      # parse chunk (mosdepth_dev.hip CH)
# file reads and member tables: a pool of their own, independent of `threads`
READ_THREADS = int(os.environ.get("GRID_INGEST_READ_THREADS", "8"))


def align(x, a=256):
    """x rounded up to a multiple of a: an int, or an int64 array."""
    if isinstance(x, np.ndarray):
        return (x.astype(np.int64) + (a - 1)) // a * a
    return -(-int(x) // a) * a


class _Pinned:
    """Reusable host staging.  Page-locked (grid_host_alloc: no torch in the
    step path -- a first ``import torch`` costs seconds on a fresh host) for
    the asynchronous copies of host-inflated text; PAGEABLE (``pinned=False``)
    for the compressed input: the runtime copies pageable memory to HBM as fast
    as page-locked here (56 vs 52-58 GB/s, profiles/r04i_host_read_h2d.jsonl),
    while page-locking 4 GB costs ~0.65 s that stalls every other HIP call."""

    def __init__(self, bound, pinned=True):
        self.b = None
        self.bound = int(bound)        # the size a request normally stays within
        self.pinned = pinned

    def get(self, n):
        if self.b is None or self.b.nbytes < n:
            if self.b is not None:
                self.b.free()
            # room to grow at once: a buffer re-pinned a few MB larger each
            # batch stalled that batch's copy to HBM by ~1 s (profiles/r03q)
            nb = max(int(n), min(2 * int(n), self.bound), 1)
            self.b = _abi.PinnedBuf(nb) if self.pinned else _Pageable(nb)
        return self.b.array


_libc = C.CDLL(None, use_errno=True)
_libc.mmap.restype = C.c_void_p
_libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
_libc.munmap.argtypes = [C.c_void_p, C.c_size_t]
_libc.madvise.argtypes = [C.c_void_p, C.c_size_t, C.c_int]


class _Pageable:
    """Pageable staging mapped through libc (anonymous, transparent huge pages
    advised, as NumPy does for large arrays) and unmapped through a foreign
    call, so the multi-GB munmap runs without the GIL (a NumPy array's free
    holds it: the staging released on a background thread stalled the step's
    own thread for ~0.5 s at the end of the config-2 ingest)."""

    def __init__(self, nbytes):
        self.nbytes = max(int(nbytes), 1)
        p = _libc.mmap(None, self.nbytes, 3, 0x22, -1, 0)      # PROT_READ|WRITE, MAP_PRIVATE|ANONYMOUS
        if p is None or p == C.c_void_p(-1).value:
            raise MemoryError(f"staging of {self.nbytes} bytes")
        _libc.madvise(p, self.nbytes, 14)                      # MADV_HUGEPAGE (advice only)
        self.ptr = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))
        # its own reference: at interpreter exit the module's globals may be
        # gone before this object's __del__ runs
        self._munmap = _libc.munmap

    def free(self):
        if self.ptr:
            self.array = None
            self._munmap(self.ptr, self.nbytes)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# The host staging of the device readers, kept between the batches and the
# ingests of one run: releasing tens of GB of staging the HIP runtime has
# copied from (page-locked, or pageable pages it has seen) holds the runtime for
# 0.4-0.8 s, and every HIP call of the step after the ingest waited for it (r04y,
# r04ac).  release_staging() frees it: at the end of a pipeline run or of a
# standalone step 4, and when the ingest hands over to the host parser
# (grid_amd/device.py release_ingest_buffers).
_STAGING = {}


def staging(name, bound, pinned=False):
    b = _STAGING.get(name)
    if b is None:
        b = _STAGING[name] = _Pinned(bound, pinned=pinned)
    return b


def staging_bytes():
    return sum(p.b.nbytes for p in _STAGING.values() if p.b is not None)


def release_staging():
    """Free the kept host staging; returns the bytes released."""
    freed = 0
    for p in list(_STAGING.values()):
        if p.b is not None:
            freed += p.b.nbytes
            p.b.free()
            p.b = None
    _STAGING.clear()
    return freed


def member_units(members, in_off, text_off, files):
    """The inflater's units for the BGZF files ``files`` (batch-local indices), one
    per member: (in_off, in_len, out_off, cap, owner), int64 each.  ``members[k]``
    is _abi.gz_members of file k, whose bytes sit at in_off[k]; its members' text
    goes back to back from text_off[k], a member's room its ISIZE; ``owner`` is k."""
    files = np.asarray(files, np.int64)
    if not len(files):
        return tuple(np.zeros(0, np.int64) for _ in range(5))
    tabs = [members[k] for k in files]
    n = np.array([len(t[0]) for t in tabs], np.int64)
    start, length, isize = (np.concatenate([t[i] for t in tabs]).astype(np.int64) for i in range(3))
    run = np.zeros(len(isize) + 1, np.int64)                # text before each member, over the whole list
    np.cumsum(isize, out=run[1:])
    first = np.cumsum(n) - n                                # each file's first member
    base = np.asarray(text_off, np.int64)[files] - run[first]
    return (np.repeat(np.asarray(in_off, np.int64)[files], n) + start, length, np.repeat(base, n) + run[:-1],
            isize, np.repeat(files, n))


def whole_units(in_off, in_len, text_off, cap, files):
    """The plain gzip files ``files``, one wave per file: ((in_off, in_len, out_off, cap), mcap),
    mcap the member records a unit may fill, from the largest file (a member takes >= 4 KiB here)."""
    files = np.asarray(files, np.int64)
    units = tuple(np.asarray(x, np.int64)[files] for x in (in_off, in_len, text_off, cap))
    return units, max(1, int(units[1].max()) // 4096 + 16)


def gpu_inflate(dev, d_in, d_text, units, mcap):
    """Launch grid_gunzip_batch over units (in_off, in_len, out_off, cap);
    returns the device buffers to read after the stream syncs."""
    n = len(units[0])
    d = [dev.upload(np.asarray(u, np.int64)) for u in units]
    mem = dev.alloc(n * mcap * _abi.GZ_MEMBER_BYTES, np.uint8)
    st, ln, nm = dev.alloc(n, np.int32), dev.alloc(n, np.int64), dev.alloc(n, np.int32)
    call("grid_gunzip_batch", dev.ctx, d_in.ptr, d[0].ptr, d[1].ptr, n, d_text.ptr, d[2].ptr, d[3].ptr, mem.ptr,
         mcap, st.ptr, ln.ptr, nm.ptr)
    return d, mem, st, ln, nm


def fold_members(n_files, owner, unit_status=None, unit_len=None):
    """Per-member results -> per file (file_status, file_len): the largest status of a
    file's members and the sum of their lengths, 0 for a file without a unit.  A
    result the caller has not read may be None, and so is its fold."""
    status = None if unit_status is None else np.zeros(n_files, np.int32)
    length = None if unit_len is None else np.zeros(n_files, np.int64)
    if status is not None:
        # a member past its BGZF size is corrupt (dropped), not several members
        np.maximum.at(status, owner, np.where(unit_status == _abi.GZ_ESPACE, _abi.GZ_EDATA, unit_status))
    if length is not None:
        np.add.at(length, owner, unit_len)
    return status, length


def chunk_table(files, tlen):
    """Chunk table of the files (batch-local indices) with text: per chunk its
    file and start; per file its first chunk (cfirst[k], k in file order)."""
    files = np.asarray(files, np.int64)
    n = -(-np.asarray(tlen, np.int64)[files] // CH) if len(files) else np.zeros(0, np.int64)
    cfirst = np.zeros(len(files) + 1, np.int32)
    np.cumsum(n, out=cfirst[1:])
    tot = int(cfirst[-1])
    if tot == 0:
        return np.zeros(1, np.int32), np.zeros(1, np.int64), cfirst, 0
    cfile = np.repeat(files, n).astype(np.int32)
    cstart = (np.arange(tot, dtype=np.int64) - np.repeat(cfirst[:-1].astype(np.int64), n)) * CH
    return cfile, cstart, cfirst, tot
