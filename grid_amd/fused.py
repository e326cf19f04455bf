"""Device-resident chain of steps 4-7 with preallocated HBM buffers.

Same arithmetic as the drop-in step modules, without the text files in
between: the normalised matrix stays in HBM as exact hundredths (int16 codes,
the step-4 output) plus the clipped bf16 panel that step 5 reads, the
neighbour lists feed the dipCN kernel directly, and the dipCN values feed
phasing.  ``bench.py`` and ``__graft_entry__.smoke()`` drive it.

Bin-axis streaming (BASELINE configs 3-4: a 50k x 3M int32 depth matrix is
600 GB, more than one GPU's 288 GB): a rank's columns are processed in
8192-aligned CHUNKS in three passes over the depth source -- (A) row-block
partial sums, (B) column means / variances (after the row means), (D) z
quantisation + the exact Gram of the chunk's panel, accumulated in int64
across chunks (integer sums: any order is exact).  The global median /
selection threshold / sigma2 bound (C) sit between B and D.  Every statistic
is the one-chunk value bit for bit: row sums keep NumPy's 8192-block order,
column statistics are per column.  The source is a resident matrix, a host
array, or the synthetic generator (``SynthSource``: regenerated per pass).

Multi-GPU: the bin (column) axis is sharded in 8192-aligned ranges
(``shard_range``), strong scaling of one cohort.  Exactness across shards:
  * row means: each rank computes 8192-block pairwise sums of its columns;
    blocks are all-gathered and every rank runs the same sequential chain
    (padding blocks are exact zeros, and acc + 0.0 == acc);
  * column statistics need no communication (sequential over all rows,
    locally); the median and the selection threshold come from all-gathered
    ratio vectors, sorted identically on every rank;
  * the Gram matrix is an integer sum over bins (int64 sums: order-free,
    exact).  Its rows are cut into 2W blocks of B; ONE reduce-scatter of the
    upper-triangle SEGMENTS (block b's rows x columns >= b*B) leaves rank r
    the complete segments of blocks r and 2W-1-r -- equal shares, about half
    the bytes of whole rows; the norms G_jj come from an all-reduce of the
    partial diagonals (n int64);
  * every pair lies in one segment (as a row or as a column entry), so the
    per-segment row and column candidates (k+1 each), all-gathered, give
    every rank the exact neighbour lists of all rows (grid_knn_seg_merge);
    above the lists' 16 keys (k + 1 > 16) the segments' transposed tiles move
    in one all-to-all instead, each rank selects from the complete rows of its
    own two blocks, and the lists are all-gathered (Steps47._seg_rows);
    dipCN and phasing are replicated (tiny / sequential per locus).

The chain is written against an ``ops`` object.  The product always uses
``HipOps`` (libgridhip.so kernels); tests substitute a CPU restatement to
check the chunking and sharding logic under torch.distributed/gloo.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import BLOCK, call, ptr
from .engine import pad_to, py_index, qmax_for_zmax

F8, I4, I8, U2, U1 = np.float64, np.int32, np.int64, np.uint16, np.uint8


def shard_range(m: int, rank: int, world: int):
    """Column range [c0, c1) of ``rank``: whole 8192-blocks, balanced."""
    nblk = -(-m // BLOCK)
    b0 = (nblk * rank) // world
    b1 = (nblk * (rank + 1)) // world
    return min(b0 * BLOCK, m), min(b1 * BLOCK, m)


class Depth16:
    """Compact depth matrix on the device (include/grid_abi.h grid_depth16):
    uint16 hundredths [n][ld] (ld % 8 == 0) plus the row-sorted escape table
    for depths above 655.33.  Half the HBM bytes of the int32 matrix in each
    of step 4's four passes; the kernels decode it to the same int32 values."""

    def __init__(self, q16, eoff, ecol, evals, ld):
        self.q16, self.eoff, self.ecol, self.evals, self.ld = q16, eoff, ecol, evals, ld
        self.desc = _abi.Depth16Desc(ptr(q16), ptr(eoff), ptr(ecol), ptr(evals))

    @classmethod
    def synth(cls, alloc, ctx, seed, n, m, col0, ncl, exc_cap=None):
        """The bench cohort (csrc/synth_model.hpp) generated in compact form."""
        ld = -(-max(m, 1) // 8) * 8
        q16 = alloc.empty((max(n, 1), ld), U2)
        eoff = alloc.empty(max(n, 1) + 1, I8)
        cap = exc_cap if exc_cap is not None else n * m // 32768 + 4096
        while True:
            ecol, evals = alloc.empty(max(cap, 1), I4), alloc.empty(max(cap, 1), I4)
            need = C.c_int64()
            rc = _abi.load().grid_synth_depth_q16(ctx, seed, n, m, ld, col0, ncl, ptr(q16), ptr(eoff),
                                                  ptr(ecol), ptr(evals), cap, C.byref(need))
            if rc == 0:
                return cls(q16, eoff, ecol, evals, ld)
            if rc != 5 or need.value <= cap:            # GRID_ERANGE: grow and retry
                _abi.check(rc, "grid_synth_depth_q16")
            cap = need.value


class TorchAlloc:
    """Buffers as torch tensors (device "cuda:i", or "cpu" in tests)."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._dt = {np.dtype(F8): torch.float64, np.dtype(I4): torch.int32, np.dtype(I8): torch.int64,
                    np.dtype(U2): torch.int16, np.dtype(U1): torch.uint8}

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._dt[np.dtype(dtype)], device=self.device)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        src = self.torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr)
        return src.to(self.device).clone()

    @staticmethod
    def read(t, i):
        return t.view(-1)[i].item()


class TorchComm:
    """The collectives the sharded chain needs, over torch.distributed
    (backend "nccl" = RCCL over xGMI on MI355X; "gloo" in CPU tests)."""

    def __init__(self, dist):
        self.dist = dist
        self.rank = dist.get_rank()
        self.world = dist.get_world_size()
        # gloo with device tensors (multi-rank rehearsal on one GPU): stage on host
        self.host = dist.get_backend() == "gloo"

    def all_gather(self, t):
        """[world, *t.shape]: rank r's t at index r.  Device tensors over RCCL
        land in that tensor directly (one collective, no stacking copy); gloo
        stages on the host."""
        import torch
        t = t.contiguous()
        if not (self.host and t.is_cuda) and t.is_cuda:
            out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
            self.dist.all_gather_into_tensor(out, t)
            return out
        src = t.cpu() if t.is_cuda else t
        parts = [torch.empty_like(src) for _ in range(self.world)]
        self.dist.all_gather(parts, src)
        return torch.stack(parts).to(t.device)

    def all_reduce_sum(self, t):
        if self.host and t.is_cuda:
            h = t.cpu()
            self.dist.all_reduce(h)
            t.copy_(h)
            return t
        self.dist.all_reduce(t)
        return t

    def reduce_scatter_sum(self, out, t):
        """out (rank's block) = sum over ranks of t's rank-th equal block."""
        if self.host and t.is_cuda:
            h = out.cpu()
            self.dist.reduce_scatter_tensor(h, t.contiguous().cpu())
            out.copy_(h)
            return out
        self.dist.reduce_scatter_tensor(out, t.contiguous())
        return out

    def all_gather_into(self, out, t, async_op=False):
        """out's first world x t.numel() elements = every rank's t in rank order, as
        raw bytes (int32 words: RCCL has no 16-bit integer type).  Over RCCL
        with async_op the collective runs on the communicator's stream after
        the work queued so far on the current one; the returned handle's
        wait() orders the current stream after it (the cohort split's panel
        pieces: the next piece moves while the Gram of this one runs)."""
        import torch
        src = t.reshape(-1).view(torch.int32)
        dst = out.reshape(-1).view(torch.int32)[: self.world * src.numel()]
        if self.host or not t.is_cuda:
            h = src.cpu() if t.is_cuda else src
            parts = [torch.empty_like(h) for _ in range(self.world)]
            self.dist.all_gather(parts, h)
            dst.copy_(torch.cat(parts).to(dst.device))
            return None
        return self.dist.all_gather_into_tensor(dst, src, async_op=async_op)

    # ---- the distributed drop-in's exchanges (grid_amd/utils/dist_step4.py)
    def _staged(self, t):
        return self.host and t.is_cuda

    def send(self, t, dst):
        """Point-to-point (the population-sum chain over the ranks)."""
        self.dist.send(t.cpu() if self._staged(t) else t, dst)

    def recv(self, t, src):
        if self._staged(t):
            h = t.cpu()
            self.dist.recv(h, src)
            t.copy_(h)
        else:
            self.dist.recv(t, src)
        return t

    def broadcast(self, t, src):
        if self._staged(t):
            h = t.cpu()
            self.dist.broadcast(h, src)
            t.copy_(h)
        else:
            self.dist.broadcast(t, src)
        return t

    def all_to_all(self, out, inp, out_splits, in_splits):
        """out = concat over ranks q of rank q's block for this rank; blocks
        of in_splits / out_splits elements (1-D tensors, any dtype: moved as
        bytes).  RCCL over xGMI: one all-to-all, every pair on its own link."""
        import torch
        es = inp.element_size()
        src = inp.reshape(-1).view(torch.uint8)
        dst = out.reshape(-1).view(torch.uint8)
        osp = [int(x) * es for x in out_splits]
        isp = [int(x) * es for x in in_splits]
        src, dst = src[: sum(isp)], dst[: sum(osp)]
        if self._staged(inp) or self.dist.get_backend() == "gloo":
            # gloo: per-pair sends over host memory
            hs = src.cpu() if src.is_cuda else src
            parts_in = list(torch.split(hs, isp))
            parts_out = [torch.empty(k, dtype=torch.uint8) for k in osp]
            self._a2a_p2p(parts_out, parts_in)
            dst.copy_(torch.cat(parts_out).to(dst.device) if parts_out else dst)
            return out
        self.dist.all_to_all_single(dst, src, osp, isp)
        return out

    def _a2a_p2p(self, parts_out, parts_in):
        """all-to-all as ordered pairwise exchanges (gloo has no all-to-all of
        ragged blocks on every build)."""
        W, r = self.world, self.rank
        parts_out[r].copy_(parts_in[r])
        for k in range(1, W):
            dst, src = (r + k) % W, (r - k) % W
            reqs = []
            if parts_in[dst].numel():
                reqs.append(self.dist.isend(parts_in[dst], dst))
            if parts_out[src].numel():
                reqs.append(self.dist.irecv(parts_out[src], src))
            for q in reqs:
                q.wait()

    def barrier(self):
        self.dist.barrier()


class SimComm:
    """One rank's share of a W-rank run on ONE GPU (per-rank timing,
    ``bench.py --sim-world W --sim-rank r``): every collective does the
    local memory work of the real one -- an all-gather writes W copies of
    this rank's part, a reduce-scatter copies this rank's block -- without
    the other ranks, so the step's device time is rank r's compute and local
    copies; xGMI time is not in it.  ``bytes_in`` counts what the real
    collectives would bring into this rank (per step when reset per step).
    The values are not those of a real run (other ranks' parts are this
    rank's), so results are meaningless; only the work is the same."""

    def __init__(self, world, rank):
        self.world, self.rank, self.host = world, rank, False
        self.bytes_in = {}

    def _count(self, kind, nbytes):
        self.bytes_in[kind] = self.bytes_in.get(kind, 0) + int(nbytes)

    def all_gather(self, t):
        import torch
        t = t.contiguous()
        self._count("all_gather", (self.world - 1) * t.numel() * t.element_size())
        return torch.stack([t] * self.world)

    def all_reduce_sum(self, t):
        self._count("all_reduce", 2 * (self.world - 1) / self.world * t.numel() * t.element_size())
        return t

    def reduce_scatter_sum(self, out, t):
        t = t.contiguous()
        self._count("reduce_scatter", (self.world - 1) * out.numel() * out.element_size())
        out.view(-1).copy_(t.view(self.world, -1)[self.rank])
        return out

    def all_to_all(self, out, inp, out_splits, in_splits):
        """The local block's copy; the other W - 1 blocks are what the real
        all-to-all brings in ((W-1)/W of the bytes at equal splits)."""
        r, es = self.rank, out.element_size()
        self._count("all_to_all", (sum(int(x) for x in out_splits) - int(out_splits[r])) * es)
        o0, i0 = sum(int(x) for x in out_splits[:r]), sum(int(x) for x in in_splits[:r])
        out.reshape(-1)[o0:o0 + int(out_splits[r])].copy_(inp.reshape(-1)[i0:i0 + int(in_splits[r])])
        return out

    def all_gather_into(self, out, t, async_op=False):
        """The W copies; with async_op on a side stream ordered after the work
        queued so far (as RCCL's stream is), the handle's wait() orders the
        current stream after them -- so the copies overlap the next Gram as
        the real collective would."""
        n = t.numel()
        self._count("all_gather_panel", (self.world - 1) * n * t.element_size())
        dst = out.reshape(-1)[: self.world * n].view(self.world, n)
        if not (async_op and t.is_cuda):
            dst.copy_(t.reshape(1, n).expand(self.world, n))
            return None
        import torch
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        ev = torch.cuda.Event()
        ev.record()
        self._side.wait_event(ev)
        with torch.cuda.stream(self._side):
            dst.copy_(t.reshape(1, n).expand(self.world, n))
        done = torch.cuda.Event()
        done.record(self._side)
        return _StreamWait(done)


class _StreamWait:
    """A collective handle: wait() orders the current stream after an event."""

    def __init__(self, ev):
        self.ev = ev

    def wait(self):
        import torch
        torch.cuda.current_stream().wait_event(self.ev)


class HipOps:
    """The chain's compute steps as libgridhip.so kernels (include/grid_abi.h)."""

    def __init__(self, dev):
        self.dev = dev
        self.ctx = dev.ctx
        self.zerodiv = C.c_int32()

    # q: an int32 hundredths buffer, or a Depth16 (compact form, *_q16 entry points)
    def row_blocks(self, q, n, m, ld, bsum, bcnt):
        if isinstance(q, Depth16):
            call("grid_norm_row_blocks_q16", self.ctx, C.byref(q.desc), n, m, q.ld, ptr(bsum), ptr(bcnt))
        else:
            call("grid_norm_row_blocks", self.ctx, ptr(q), n, m, ld, ptr(bsum), ptr(bcnt))

    def row_means(self, bsum, bcnt, n, nblk, rm):
        call("grid_norm_row_means", self.ctx, ptr(bsum), ptr(bcnt), n, nblk, ptr(rm))

    def col_means(self, q, n, m, ld, rm, mu):
        if isinstance(q, Depth16):
            call("grid_norm_col_means_q16", self.ctx, C.byref(q.desc), n, m, q.ld, ptr(rm), ptr(mu))
        else:
            call("grid_norm_col_means", self.ctx, ptr(q), n, m, ld, ptr(rm), ptr(mu))

    def col_vars(self, q, n, m, ld, rm, mu, var, ratio):
        if isinstance(q, Depth16):
            call("grid_norm_col_vars_q16", self.ctx, C.byref(q.desc), n, m, q.ld, ptr(rm), ptr(mu), ptr(var),
                 ptr(ratio))
        else:
            call("grid_norm_col_vars", self.ctx, ptr(q), n, m, ld, ptr(rm), ptr(mu), ptr(var), ptr(ratio))

    def sort_valid(self, v, n, out):
        nv = C.c_int64()
        call("grid_sort_valid", self.ctx, ptr(v), n, ptr(out), C.byref(nv))
        return nv.value

    def count_valid(self, v, n):
        nv = C.c_int64()
        call("grid_count_valid", self.ctx, ptr(v), n, C.byref(nv))
        return nv.value

    def select_kth(self, v, n, ks):
        """The ks-th smallest non-NaN values of v[:n] (grid_sort_valid's order)."""
        kk = (C.c_int64 * len(ks))(*ks)
        out = (C.c_double * len(ks))()
        call("grid_select_kth", self.ctx, ptr(v), n, kk, len(ks), out)
        return list(out)

    def select_gt(self, v, n, thr, idx):
        c = C.c_int64()
        call("grid_select_gt", self.ctx, ptr(v), n, thr, ptr(idx), C.byref(c))
        return c.value

    def gather(self, v, idx, n, out):
        call("grid_gather_f64", self.ctx, ptr(v), ptr(idx), n, ptr(out))

    def round_decimals(self, v, n, dec, out):
        call("grid_round_decimals", self.ctx, ptr(v), n, dec, ptr(out))

    def colmap_range(self, r, n, smin, smax, colmap):
        c = C.c_int64()
        call("grid_colmap_range", self.ctx, ptr(r), n, smin, smax, ptr(colmap), C.byref(c))
        return c.value

    # pass C on the device (include/grid_abi.h grid_sel_*): enqueue only, one read-back
    def sel_stage1(self, rall, rlen, ratio, ml, len_pad, top_frac, sel, r3, st):
        call("grid_sel_stage1", self.ctx, ptr(rall), rlen, ptr(ratio), ml, len_pad, top_frac, ptr(sel), ptr(r3),
             ptr(st))

    def sel_stage2(self, r3all, r3len, r3, ml, frac_r, sigma2_max, colmap, st):
        call("grid_sel_stage2", self.ctx, ptr(r3all), r3len, ptr(r3), ml, frac_r, sigma2_max, ptr(colmap), ptr(st))

    def sel_read(self, st):
        h = np.zeros(_abi.SEL_STATE, np.int64)
        call("grid_sel_read", self.ctx, ptr(st), h.ctypes.data)
        return h

    def zquant(self, q, n, ld, sel, r, rm, mu, scale, zq, ld_zq, colmap, qmax, zb, np_zb):
        """z hundredths + the K-blocked bf16 panel [kpad/32][np_zb][32]."""
        of = C.c_int32()
        if isinstance(q, Depth16):
            call("grid_norm_zquant_kb_q16", self.ctx, C.byref(q.desc), n, q.ld, ptr(sel), r, ptr(rm), ptr(mu), scale,
                 ptr(zq), ld_zq, ptr(colmap), qmax, ptr(zb), np_zb, C.byref(of))
        else:
            call("grid_norm_zquant_kb", self.ctx, ptr(q), n, ld, ptr(sel), r, ptr(rm), ptr(mu), scale, ptr(zq),
                 ld_zq, ptr(colmap), qmax, ptr(zb), np_zb, C.byref(of))
        return of.value

    def zquant16(self, q, n, ld, sel, r, rm, mu, scale, zq16, ld_zq, colmap, qmax, zb, np_zb, esc_idx, esc_val,
                 defer=None):
        """As zquant with the step-4 output as int16 codes plus an escape list
        for the rare values outside them.  Returns (overflow bits, escapes);
        bit 1 = the list overflowed (the caller reruns with int32).  defer: a
        2-slot int64 device tensor that receives (overflow bits, escapes) on the
        stream instead (no synchronisation; returns None)."""
        of, ne = C.c_int32(), C.c_int64()
        h_ne, h_of = (None, None) if defer is not None else (C.byref(ne), C.byref(of))
        cap = 0 if esc_idx is None else esc_idx.numel()
        if isinstance(q, Depth16):
            call("grid_norm_zquant_kb16_q16", self.ctx, C.byref(q.desc), n, q.ld, ptr(sel), r, ptr(rm), ptr(mu),
                 scale, ptr(zq16), ld_zq, ptr(colmap), qmax, ptr(zb), np_zb, ptr(esc_idx), ptr(esc_val), cap,
                 h_ne, h_of)
        else:
            call("grid_norm_zquant_kb16", self.ctx, ptr(q), n, ld, ptr(sel), r, ptr(rm), ptr(mu), scale, ptr(zq16),
                 ld_zq, ptr(colmap), qmax, ptr(zb), np_zb, ptr(esc_idx), ptr(esc_val), cap, h_ne, h_of)
        if defer is not None:
            call("grid_status_copy", self.ctx, ptr(defer))
            return None
        return of.value, ne.value

    def gram(self, zb, np_, kpad, qmax, gram):
        """Exact Gram of the K-blocked panel (first kpad columns)."""
        call("grid_knn_gram_kb", self.ctx, ptr(zb), np_, kpad, qmax, ptr(gram))

    def mirror(self, gram, np_):
        call("grid_knn_mirror", self.ctx, ptr(gram), np_)

    def gram_rows(self, zb, np_, kpad, qmax, row0, nrows, out, ld):
        """Cohort split: rows [row0, row0+nrows) x columns [row0, np) of the
        K-blocked panel's Gram, added into out (stride ld, origin (row0, row0))."""
        call("grid_knn_gram_kb_rows", self.ctx, ptr(zb), np_, kpad, qmax, row0, nrows, ptr(out), ld)

    def mirror_ld(self, buf, n, ld):
        call("grid_knn_mirror_ld", self.ctx, ptr(buf), n, ld)

    def diag(self, gram, np_, n, norms):
        call("grid_knn_diag", self.ctx, ptr(gram), np_, n, ptr(norms))

    def seg_topk(self, seg, ld, nrows, ncols, norms, n, k, r0, c0, rowc, colc):
        call("grid_knn_seg_topk", self.ctx, ptr(seg), ld, nrows, ncols, ptr(norms), n, k, r0, c0, ptr(rowc),
             ptr(colc))

    def seg_pack(self, gram, np_, W, B, send):
        """The segment reduce-scatter's send buffer from the whole Gram, one launch."""
        call("grid_knn_seg_pack", self.ctx, ptr(gram), np_, W, B, ptr(send))

    def seg_merge(self, rowc, colc, ldc, B, n, k, idx, d2, cnt):
        call("grid_knn_seg_merge", self.ctx, ptr(rowc), ptr(colc), ldc, B, n, k, ptr(idx), ptr(d2), ptr(cnt))

    def seg_tiles_pack(self, seg, ld, B, W, b_src, send):
        """Every transposed tile of segment b_src into send [W][2][B][B]."""
        call("grid_knn_seg_tiles_pack", self.ctx, ptr(seg), ld, B, W, b_src, ptr(send))

    def seg_rows_fill(self, seg, ld, recv, B, W, b, rows, ld_rows):
        """Block b's complete rows [B][ld_rows] from its segment and recv [W][2][B][B]."""
        call("grid_knn_seg_rows_fill", self.ctx, ptr(seg), ld, ptr(recv), B, W, b, ptr(rows), ld_rows)

    def topk_rows(self, rows, ld, norms, n, k, row0, nrows, idx, d2, cnt):
        call("grid_knn_topk_rows", self.ctx, ptr(rows), ld, ptr(norms), n, k, row0, nrows, ptr(idx), ptr(d2),
             ptr(cnt))

    def synth(self, seed, n, m, ld, col0, ncl, out):
        call("grid_synth_depth", self.ctx, seed, n, m, ld, col0, ncl, ptr(out))

    def dipcn(self, n, reads, has, scale, nbr, nscale, ncnt, ld, n_nbr, out, valid, defer=None):
        """Returns the zero-division flag; with ``defer`` (a 2-slot int64 device
        tensor) the flag goes there on the stream instead (returns None)."""
        call("grid_dipcn", self.ctx, n, ptr(reads), ptr(has), ptr(scale), ptr(nbr), ptr(nscale), ptr(ncnt), ld,
             n_nbr, ptr(out), ptr(valid), None if defer is not None else C.byref(self.zerodiv))
        if defer is not None:
            call("grid_status_copy", self.ctx, ptr(defer))
            return None
        return self.zerodiv.value

    def phase(self, n, irr, off, nbr, w, min_nbr, iters, sched, hap, imp, mean):
        order, loff, nlev, pk_nbr, pk_w, pk_cnt, flags, max_list = sched
        call("grid_hi_phase", self.ctx, n, ptr(irr), ptr(off), ptr(nbr), ptr(w), min_nbr, iters, ptr(order),
             ptr(loff), nlev, ptr(pk_nbr), ptr(pk_w), ptr(pk_cnt), ptr(hap), ptr(imp), ptr(mean), flags, max_list)

    def schedule(self, off, nbr, w):
        return _abi.hi_schedule(off, nbr, w)


class SynthSource:
    """Depth source: the bench cohort (csrc/synth_model.hpp) regenerated on
    the device for every pass over a chunk -- the stand-in for data arriving
    in HBM when the matrix does not fit (BASELINE configs 3-4).  Local column
    c of the rank is global bin col0 + c."""

    def __init__(self, ops, seed, n, col0, ncl):
        self.ops, self.seed, self.n, self.col0, self.ncl = ops, seed, n, col0, ncl

    def fill(self, a, b, out, ldo):
        self.ops.synth(self.seed, self.n, b - a, ldo, self.col0 + a, self.ncl, out)


class HostSource:
    """Depth source: an int32 hundredths matrix in host memory, copied to the
    device one column slab per chunk (pinned staging, H2D)."""

    def __init__(self, q):
        self.q = q

    def fill(self, a, b, out, ldo):
        import torch
        w = b - a
        slab = torch.from_numpy(np.ascontiguousarray(self.q[:, a:b]))
        dst = out.view(-1)[: self.q.shape[0] * ldo].view(self.q.shape[0], ldo)
        dst[:, :w].copy_(slab.pin_memory() if dst.is_cuda else slab, non_blocking=False)


def chunk_ranges(m_local: int, chunk: int | None):
    """Local column ranges [a, b) of the passes: whole 8192-blocks per chunk."""
    if not chunk or chunk >= m_local:
        return [(0, m_local)]
    assert chunk % BLOCK == 0, "chunk must be a multiple of 8192 columns"
    return [(a, min(a + chunk, m_local)) for a in range(0, m_local, chunk)]


class Steps47:
    """One rank's share of the steps 4-7 chain for an n x m cohort.

    Inputs: the depth matrix of this rank's columns (global offset col0, a
    multiple of 8192) -- resident [n][ld] int32 hundredths, a Depth16, or a
    source with ``fill(a, b, out, ld)`` (``SynthSource``, ``HostSource``) --
    reads [n] f64 for every sample, and the IBS hap-neighbour CSR of the
    cohort (its GS level schedule is derived once).

    ``chunk``: columns per pass chunk (a multiple of 8192; None = the whole
    range in one chunk).  ``keep_z``: keep the whole step-4 output in HBM
    (``zq_int32()``); False writes each chunk's z into a chunk buffer that is
    overwritten by the next chunk (the fused mode of configs 3-4, SURVEY H7;
    ``on_z_chunk(zq16, ld, s0, s1, esc_idx, esc_val)`` may consume it).
    """

    def __init__(self, ops, alloc, n, m_total, col0, m_local, *, k=10, n_nbr=300, top_frac=0.1, zmax=2.0,
                 sigma2_max=1000.0, frac_r=1.0, min_nbr=1, n_iters=100, comm=None, phase_lane=None, zq16=True,
                 chunk=None, keep_z=True, on_z_chunk=None, split="bin", piece_bytes=1 << 31, col_lane=None,
                 step5_wide="auto"):
        """``phase_lane``: optional (ops, torch.cuda.Stream) pair on which step
        7 runs.  Phasing is one workgroup for ~4 ms, so on its own stream it
        overlaps other work instead of idling the other 255 CUs.  It is
        DEFERRED: pass i's phasing is issued during pass i+1, ordered after
        that pass's last Gram launch (an event), so its workgroup never holds
        a CU while the persistent Gram (one workgroup per CU) is resident -- a
        Gram workgroup queued behind it held the whole launch open (the short
        per-rank steps of the multi-GPU runs).  It then overlaps pass i+1's
        top-k / dipCN and pass i+2's statistics and quantisation.  dipCN
        writes alternate buffers; ``finish()`` issues the last pass's phasing
        (call it before reading ``hap`` / ``imp`` or stopping a clock).

        ``split`` (multi-rank runs): how step 5's all-pairs Gram is shared.
        "bin": every rank sums the whole upper triangle over its own bins and
        ONE reduce-scatter of int64 segments completes it.  "cohort" (north
        star's cohort axis, the reference's all-pairs search
        find_neighbors.py:204-213 with the Gram's rows sharded): step 4 stays
        bin-sharded (column statistics local and exact), then the quantised
        bf16 panel moves in pieces of at most ``piece_bytes`` per rank-set by
        an all-gather overlapped with the Gram of the previous piece, and
        every rank computes its own two row segments over ALL bins -- no
        Gram reduce-scatter.  Both give the same segments, bit for bit
        (integer sums), and share the candidate merge.

        ``step5_wide`` (multi-rank runs with k + 1 above the candidate lists'
        16 keys): "auto" exchanges the segments' transposed tiles so that
        every rank selects its own two row blocks from complete rows
        (``row_exchange``, both splits; ops without the two tile operations
        keep the earlier routes); "allreduce" (bin split only) forces the
        earlier route, the all-reduce of the whole Gram (``full_rows``)."""
        if step5_wide not in ("auto", "allreduce"):
            raise ValueError(f"step5_wide must be 'auto' or 'allreduce', not {step5_wide!r}")
        self.ops, self.A, self.comm = ops, alloc, comm
        # col_lane: optional (ops, torch stream) pair for the column-statistics
        # passes of a one-chunk shard -- a stream CU-masked away from the phase
        # lane's CU (bench.py), so the passes' one round of workgroups never
        # shares a CU with the phasing workgroup
        self.col_lane = col_lane
        # one lane, or two: the phasing of _dips[b] then runs on lane b, so the
        # last two passes' phasings (finish()) overlap instead of queueing
        self.phase_lane = phase_lane
        self._lanes = None if phase_lane is None else (list(phase_lane) if isinstance(phase_lane, list)
                                                       else [phase_lane])
        self._ev_phase = {}
        self.rank = comm.rank if comm else 0
        self.world = comm.world if comm else 1
        if split not in ("bin", "cohort"):
            raise ValueError(f"split must be 'bin' or 'cohort', not {split!r}")
        self.split = split if comm is not None else "bin"
        if step5_wide == "allreduce" and self.split != "bin":
            raise ValueError("step5_wide='allreduce' is a bin-split route")
        self.n, self.m, self.col0, self.ml = n, m_total, col0, m_local
        assert col0 % BLOCK == 0
        self.k, self.n_nbr, self.top_frac = k, n_nbr, top_frac
        self.sigma2_max, self.frac_r = sigma2_max, frac_r
        self.min_nbr, self.n_iters = min_nbr, n_iters
        self.qmax = qmax_for_zmax(zmax)
        self.chunks = chunk_ranges(m_local, chunk)
        self.nch = len(self.chunks)
        self.keep_z, self.on_z_chunk = keep_z or self.nch == 1, on_z_chunk
        a = alloc
        n1 = max(n, 1)
        widths = [shard_range(m_total, r, self.world) for r in range(self.world)]
        self.mlmax = max(c1 - c0 for c0, c1 in widths)
        self.nblk_l = -(-m_local // BLOCK)
        self.nblk_max = -(-self.mlmax // BLOCK)
        self.bsum = a.empty((n1, max(self.nblk_l, 1)), F8)
        self.bcnt = a.empty((n1, max(self.nblk_l, 1)), I4)
        cw = max(b - a_ for a_, b in self.chunks)             # widest chunk
        # every rank's chunk count and widest chunk (the cohort split's panel
        # exchange runs the same number of rounds on every rank)
        rchunks = [chunk_ranges(c1 - c0, chunk) for c0, c1 in widths]
        self.nch_x = max(len(rc) for rc in rchunks)
        cw_x = max(max(b - a_ for a_, b in rc) for rc in rchunks)
        if self.nch > 1:
            nbc = -(-cw // BLOCK)
            self.bsum_c, self.bcnt_c = a.empty(n1 * nbc, F8), a.empty(n1 * nbc, I4)
        # chunk buffer of the depth matrix (streamed / chunked sources), ld % 4 == 0
        self.ldc = pad_to(max(cw, 1), 4)
        self.qc = None
        self.qc_holds = None                                  # chunk index the buffer holds
        if comm is not None:                                  # (world 1 too: the collective path itself)
            self.bsum_pad = a.empty((n1, max(self.nblk_max, 1)), F8)
            self.bcnt_pad = a.empty((n1, max(self.nblk_max, 1)), I4)
        self.rm = a.empty(n1, F8)
        ml1 = max(m_local, 1)
        self.mu, self.var = a.empty(ml1, F8), a.empty(ml1, F8)
        self.ratio = a.empty(max(self.mlmax, 1), F8)
        self.sorted = a.empty(max(self.mlmax * self.world, 1), F8)
        self.sel = a.empty(ml1, I4)
        self.r3 = a.empty(max(self.mlmax, 1), F8)
        self.colmap = a.empty(ml1, I4)
        self.sel_st = a.empty(_abi.SEL_STATE, I8)             # pass C's device scalars (grid_sel_*)
        # status blocks read once at the end of a pass (grid_status_copy): slots
        # 0-1 the step-4 output's (overflow bits, escapes), 2-3 dipCN's zero division
        self.dstat = a.empty(4, I8)
        self._zdef = self._ddef = None
        # step-4 output, exact hundredths: int16 codes (GRID_ZQ16_*, half the
        # HBM writes) when the ops support them, int32 otherwise or when a
        # pass has |z| > 327.66 (zq_int32() gives the int32 form either way)
        zw = ml1 if self.keep_z else cw
        self.zq16 = a.empty((n1, zw), U2) if zq16 and hasattr(ops, "zquant16") else None
        self.zq = None if self.zq16 is not None else a.empty((n1, zw), I4)
        self.zq_is16, self.nesc = False, 0
        if self.zq16 is not None:                        # escapes: |z| > 327.65 (rare)
            cap = min(n1 * zw, max(1 << 20, (n1 * zw) >> 10))
            self.esc_idx, self.esc_val = a.empty(cap, I8), a.empty(cap, I4)
        self.np_ = pad_to(n1, 256)
        # multi-GPU step 5 (comm given): the Gram's 2W row blocks of B rows; rank
        # r holds only the upper-triangle segments of blocks r and 2W-1-r
        # (grid_knn_seg_topk), about half of the full rows, equal per rank.  The
        # cohort split computes them with the Gram kernel's 256-row tiles, so
        # there B is a multiple of 256
        self.B = -(-self.np_ // (2 * self.world))
        if self.split == "cohort":
            self.B = pad_to(self.B, 256)
        self.npw = 2 * self.world * self.B
        self.np_rs = self.npw if comm is not None else self.np_
        self.kpad = pad_to(cw_x if self.split == "cohort" else cw, 64)
        # step-5 input panel (bf16), K-blocked [kpad/32][np][32]: one K-step of a
        # row panel is contiguous for the Gram kernel's DMA
        self.zb = a.empty((self.kpad // _abi.KBW, self.np_, _abi.KBW), U2)
        self.zb.zero_()                                  # pad rows stay zero
        # row stride np; rows >= np stay zero (the cohort split has no whole Gram)
        self.gram = a.empty((self.np_rs, self.np_), I8) if self.split == "bin" else None
        self.norms = a.empty(self.np_, I8)
        self.norms.zero_()
        kk = max(k, 1)
        # k + 1 above the segment candidate lists' length (the drop-in's
        # num_neighbors may be the reference's default 500).  row_exchange: the
        # segments' transposed tiles travel in one all-to-all (2 B^2 int64 per
        # rank pair, whatever k is) and every rank selects its own two row
        # blocks from complete rows (_seg_rows).  full_rows (ops without the
        # tile operations, or step5_wide="allreduce"): the bin split sums the
        # whole upper triangle over the ranks (one all-reduce of the np x np
        # int64 Gram) and every rank selects from all n whole rows
        wide = comm is not None and kk + 1 > _abi.SEG_K1
        self.row_exchange = (wide and step5_wide == "auto" and hasattr(ops, "seg_tiles_pack")
                             and hasattr(ops, "seg_rows_fill"))
        self.full_rows = wide and not self.row_exchange
        if self.full_rows and self.split != "bin":
            raise _abi.GridNativeError(f"the cohort split needs k + 1 <= {_abi.SEG_K1}")
        if comm is not None and not self.full_rows:
            W, B = self.world, self.B
            self.my_blocks = (self.rank, 2 * W - 1 - self.rank)
            self.seg_len = B * (2 * W + 1) * B                 # int64 cells of one rank's two segments
            self.seg_recv = a.empty(self.seg_len, I8)
            if self.split == "bin":
                self.seg_send = a.empty(W * self.seg_len, I8)
            else:
                # panel pieces: P K-blocks of every rank (P even: the Gram takes
                # whole 64-column K-steps), two buffers (gather p+1 || Gram p)
                per_blk = W * self.np_ * _abi.KBW * 2
                nkb = max(self.kpad // _abi.KBW, 2)
                self.piece = max(2, min(nkb, int(piece_bytes // per_blk)) // 2 * 2)
                self.gbuf = [a.empty((W * self.piece, self.np_, _abi.KBW), U2) for _ in range(2)]
                self.norms_l = a.empty((2, B), I8)
            if self.row_exchange:
                # tiles out / in [W][2][B][B] (the pair p -> p fills one slot:
                # zeroed once, so no collective moves unwritten memory), this
                # rank's complete rows, and its blocks' lists; rows >= n keep
                # (-1, 0, 0), which the selection never writes
                self.x_send, self.x_recv = a.empty((W, 2, B, B), I8), a.empty((W, 2, B, B), I8)
                self.x_send.zero_()
                self.x_recv.zero_()
                self.rows_l = a.empty((2, B, self.npw), I8)
                self.bidx_l, self.bd2_l = a.empty((2, B, kk), I4), a.empty((2, B, kk), I8)
                self.bcnt_l = a.empty((2, B), I4)
                self.bidx_l.fill_(-1)
                self.bd2_l.zero_()
                self.bcnt_l.zero_()
            else:
                K1 = _abi.SEG_K1
                self.rowc_l = a.empty((2, B, K1), I8)               # packed keys (uint64 bits)
                self.colc_l = a.empty((2, self.npw, K1), I8)
            # gathered lists -> global block order: block b is rank b (slot 0)
            # for b < W, else rank 2W-1-b (slot 1)
            self.blk_src = [(b, 0) if b < W else (2 * W - 1 - b, 1) for b in range(2 * W)]
            self.idx_l = a.empty((n1, kk), I4)
            self.d2_l = a.empty((n1, kk), I8)
            self.cnt_l = a.empty(n1, I4)
        else:
            self.idx_l = a.empty((n1, kk), I4)
            self.d2_l = a.empty((n1, kk), I8)
            self.cnt_l = a.empty(n1, I4)
        self.scale2 = a.empty(n1, F8)
        self.nscale = a.empty((n1, kk), F8)
        # dipCN output, double-buffered: the deferred phasing of pass i reads
        # one buffer while pass i+1's dipCN writes the other
        self._dips = [a.empty(n1, F8), a.empty(n1, F8)]
        self._cur = 0
        self._ev_free = [None, None]        # event: the phasing that read _dips[b] is done
        self._pending = None                 # dipCN buffer whose phasing is not issued yet
        self.valid = a.empty(n1, U1)
        # phasing outputs, double-buffered with the dipCN buffer they come from
        self._haps = [a.empty(2 * n1, F8), a.empty(2 * n1, F8)]
        self._imps = [a.empty(2 * n1, F8), a.empty(2 * n1, F8)]
        self._means = [a.empty(1, F8), a.empty(1, F8)]
        self._out = 0                        # the buffer set of the last issued phasing
        self.marks = None
        self.gram_evs = None

    # ------------------------------------------------------------------ inputs
    def set_phasing_graph(self, off, nbr, w):
        """IBS/IBD hap-neighbour CSR; the GS level schedule and the packed,
        schedule-ordered lists are derived once here (input preparation, like
        parsing the neighbour file)."""
        order, loff, nl, pk_nbr, pk_w, pk_cnt, flags, max_list = self.ops.schedule(off, nbr, w)
        up = self.A.upload
        self.off = up(np.asarray(off, I8))
        self.nbr = up(np.asarray(nbr if len(nbr) else np.zeros(1), I4))
        self.w = up(np.asarray(w if len(w) else np.zeros(1), F8))
        self.nlev = nl
        self.sched = (up(np.asarray(order, I4)), up(np.asarray(loff, I4)), nl, up(pk_nbr), up(pk_w), up(pk_cnt),
                      flags, max_list)

    @property
    def dip(self):
        """dipCN values of the last pass."""
        return self._dips[self._cur]

    @property
    def hap(self):
        """Phased haplotype values of the last pass (after finish())."""
        return self._haps[self._out]

    @property
    def imp(self):
        return self._imps[self._out]

    @property
    def mean(self):
        return self._means[self._out]

    def set_reads(self, reads):
        self.reads = self.A.upload(np.asarray(reads, F8))
        self.has = self.A.upload(np.ones(max(self.n, 1), dtype=U1))

    def zq_int32(self):
        """The step-4 output of the last pass as int32 hundredths
        (GRID_ZQ_NAN / GRID_ZQ_NEG0 sentinels), whichever form it was written
        in (keep_z mode: the whole [n][r] output)."""
        if not self.keep_z:
            raise ValueError("keep_z=False: the step-4 output was streamed chunk by chunk")
        if not self.zq_is16:
            return self.zq
        return zq16_to_int32(self.A.torch, self.zq16, self.esc_idx[: self.nesc], self.esc_val[: self.nesc])

    # ---------------------------------------------------------------- helpers
    def _read(self, b, i):
        return self.A.read(b, i)

    def _gather_padded(self, b, count, maxcount, fill):
        """All-gather the first ``count`` entries of a 1-D f64 buffer from
        every rank (padded with ``fill``); returns (buffer, total length)."""
        if self.comm is None:
            return b, count
        if count < maxcount:
            b.view(-1)[count:maxcount].fill_(fill)
        g = self.comm.all_gather(b.view(-1)[:maxcount])
        return g.view(-1), self.world * maxcount

    def _sum_int(self, v):
        import torch
        t = torch.tensor([v], dtype=torch.int64, device=self.norms.device)
        self.comm.all_reduce_sum(t)
        return int(t.item())

    def _mark(self, name):
        if self.marks is not None:
            import torch
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def stage_ms(self):
        """Per-stage device time of the last run(profile=True) (ms)."""
        out = {}
        for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out

    def gram_ms(self):
        """Device time of the Gram launches of the last run(time_gram=True)
        (ms, summed over chunks) and the launch count."""
        return sum(a.elapsed_time(b) for a, b in self.gram_evs), len(self.gram_evs)

    def _chunk_q(self, q, ld, ci, stage):
        """(buffer, ld) holding the depth of local columns chunks[ci].  With
        profile marks on, a fill from a streamed source is timed as stage
        "source" (the time before it goes to ``stage``)."""
        a, b = self.chunks[ci]
        resident = hasattr(q, "data_ptr") or isinstance(q, Depth16)
        if resident and self.nch == 1:
            return q, ld
        if isinstance(q, Depth16):
            raise _abi.GridNativeError("the compact depth form is resident-only (one chunk)")
        if self.qc_holds == ci:
            return self.qc, self.ldc
        if self.qc is None:
            self.qc = self.A.empty(max(self.n, 1) * self.ldc, I4)
        self._mark(stage)
        if resident:                                     # a resident matrix read in chunks (tests)
            dst = self.qc[: self.n * self.ldc].view(self.n, self.ldc)
            dst[:, : b - a].copy_(q[: self.n, a:b])
        else:
            q.fill(a, b, self.qc, self.ldc)
        self._mark("source")
        self.qc_holds = ci
        return self.qc, self.ldc

    # -------------------------------------------------------------------- run
    def run(self, q, ld=None, time_gram=False, profile=False, upto="step7"):
        """One pass of steps 4-7.  ``q``: the depth source of this shard (see
        the class docstring; ``ld`` = row stride of a resident matrix).
        ``time_gram``: record HIP events around every Gram launch (on the
        stream every kernel here runs on; read with gram_ms()).  ``upto``:
        "step4" ends after the step-4 output (no Gram), "step5" after the
        neighbour lists (the distributed drop-in, dist_step4.py)."""
        if upto not in ("step4", "step5", "step7"):
            raise ValueError(f"upto must be step4, step5 or step7, not {upto!r}")
        o, n, ml = self.ops, self.n, self.ml
        self.marks = [] if profile else None
        self.gram_evs = [] if time_gram else None
        self.qc_holds = None                     # every pass reads its source afresh
        order = list(range(self.nch))
        self._mark("start")
        # ---- pass A: 8192-block pairwise partial sums per row ----
        for ci in order:
            a, b = self.chunks[ci]
            qc, ldc = self._chunk_q(q, ld, ci, "row_means")
            if self.nch == 1:
                o.row_blocks(qc, n, b - a, ldc, self.bsum, self.bcnt)
            else:
                nb, b0 = -(-(b - a) // BLOCK), a // BLOCK
                o.row_blocks(qc, n, b - a, ldc, self.bsum_c, self.bcnt_c)
                self.bsum[:n, b0:b0 + nb].copy_(self.bsum_c[: n * nb].view(n, nb))
                self.bcnt[:n, b0:b0 + nb].copy_(self.bcnt_c[: n * nb].view(n, nb))
        nblk_tot, bsum, bcnt = self.nblk_l, self.bsum, self.bcnt
        if self.comm is not None:
            self.bsum_pad.zero_()
            self.bcnt_pad.zero_()
            self.bsum_pad[:, : self.nblk_l].copy_(self.bsum)
            self.bcnt_pad[:, : self.nblk_l].copy_(self.bcnt)
            rows = self.bsum_pad.shape[0]
            bsum = self.comm.all_gather(self.bsum_pad).permute(1, 0, 2).reshape(rows, -1).contiguous()
            bcnt = self.comm.all_gather(self.bcnt_pad).permute(1, 0, 2).reshape(rows, -1).contiguous()
            nblk_tot = self.world * self.nblk_max
        o.row_means(bsum, bcnt, n, nblk_tot, self.rm)
        self._mark("row_means")
        # ---- pass B: column statistics (local, exact); the chunk the buffer
        # still holds goes first ----
        if self.col_lane is not None and self.nch == 1:
            import torch
            cops, cstream = self.col_lane
            ev = torch.cuda.Event()
            ev.record()
            cstream.wait_event(ev)
            qc, ldc = self._chunk_q(q, ld, 0, "col_stats")
            cops.col_means(qc, n, ml, ldc, self.rm, self.mu[:ml])
            cops.col_vars(qc, n, ml, ldc, self.rm, self.mu[:ml], self.var[:ml], self.ratio[:ml])
            done = torch.cuda.Event()
            done.record(cstream)
            torch.cuda.current_stream().wait_event(done)
        else:
            for ci in reversed(order):
                a, b = self.chunks[ci]
                qc, ldc = self._chunk_q(q, ld, ci, "col_stats")
                o.col_means(qc, n, b - a, ldc, self.rm, self.mu[a:b])
                o.col_vars(qc, n, b - a, ldc, self.rm, self.mu[a:b], self.var[a:b], self.ratio[a:b])
        self._mark("col_stats")
        # ---- pass C: median -> scale; sorted(...)[int(top_frac*n)] -> selection;
        # step 5's region filter on the "%.3f" ratios (find_neighbors.py:148-171)
        # and the panel column map -- on the device (grid_sel_stage1/2), with
        # one read-back of the scalars the later grids need ----
        rall, rlen = self._gather_padded(self.ratio, ml, self.mlmax, float("nan"))
        st = self.sel_st
        pad = self.mlmax if self.comm is not None else ml
        o.sel_stage1(rall, rlen, self.ratio, ml, pad, self.top_frac, self.sel, self.r3, st)
        if self.comm is not None:
            r3all = self.comm.all_gather(self.r3.view(-1)[: self.mlmax]).view(-1)
            r3len = self.world * self.mlmax
            self.comm.all_reduce_sum(st[_abi.SEL_RTOT:_abi.SEL_RTOT + 1])
        else:
            r3all, r3len = self.r3, ml
        o.sel_stage2(r3all, r3len, self.r3, ml, self.frac_r, float(self.sigma2_max), self.colmap, st)
        h = o.sel_read(st)
        if h[_abi.SEL_ERR] == 1:
            raise IndexError("list index out of range")
        if h[_abi.SEL_ERR]:
            raise _abi.GridNativeError("sigma^2 rank out of range (frac_r > 1)")
        f = h.view(np.float64)
        nvalid, r_loc = int(h[_abi.SEL_NVALID]), int(h[_abi.SEL_RLOC])
        scale = 1.0
        if nvalid:
            med = float(f[_abi.SEL_V0]) if nvalid % 2 else (float(f[_abi.SEL_V0]) + float(f[_abi.SEL_V0 + 1])) / 2.0
            if med > 0:
                scale = 1.0 / math.sqrt(med / 100.0)
        self.scale, self.r_loc = scale, r_loc
        self.r_tot = int(h[_abi.SEL_RTOT])
        self.ruse_loc = int(h[_abi.SEL_RUSE])
        sb, kb = self._chunk_bounds(r_loc)
        if self.split == "cohort":
            self._cohort_plan(kb)
        self._mark("select_sort")
        # ---- pass D: z (step-4 output) + clipped bf16 panel per chunk, the
        # exact Gram accumulated over chunks (MFMA); the cohort split instead
        # all-gathers each chunk's panel in pieces and adds every piece's
        # product into this rank's two row segments (the same number of
        # exchange rounds on every rank: a rank out of chunks sends zeros) ----
        if self.gram is not None:
            self.gram.zero_()
        else:
            self.seg_recv.zero_()
        self.nesc, self.zq_is16 = 0, self.zq16 is not None
        self.chunk_used = []
        self._gslot = 0
        self.exec_flops = 0.0                    # cohort split: MFMA work its Gram launches executed
        for ci in range(self.nch_x if self.split == "cohort" else self.nch):
            if ci >= self.nch:
                self._cohort_gram(ci, 0)
                continue
            a, b = self.chunks[ci]
            s0, s1 = sb[ci], sb[ci + 1]
            used = kb[ci + 1] - kb[ci]
            self.chunk_used.append(used)
            qc, ldc = self._chunk_q(q, ld, ci, "zquant_gram")
            if self.nch == 1:
                sel_c, cm_c = self.sel, self.colmap
            else:
                sel_c = (self.sel[s0:s1] - a).to(self.sel.dtype)
                cmv = self.colmap[s0:s1]
                cm_c = self.A.torch.where(cmv >= 0, cmv - kb[ci], cmv).to(self.colmap.dtype)
            # what on_z_chunk may inspect: the chunk's depth buffer, its
            # chunk-local selection / panel map, and the panel columns it fills
            self.cur = {"ci": ci, "a": a, "b": b, "s0": s0, "s1": s1, "q": qc, "ld": ldc, "sel": sel_c,
                        "colmap": cm_c, "k0": kb[ci], "used": used}
            self._zquant(q, qc, ldc, a, b, s0, s1, sel_c, cm_c)
            kpad_c = pad_to(used, 64)
            if used and n and kpad_c > used:
                # columns colmap did not write this chunk (all in its last K-block)
                b0 = used // _abi.KBW
                if used % _abi.KBW:
                    self.zb[b0, :n, used % _abi.KBW:].zero_()
                    b0 += 1
                self.zb[b0:kpad_c // _abi.KBW, :n].zero_()
            if upto == "step4":
                continue
            if self.split == "cohort":
                self._cohort_gram(ci, used)
                continue
            if used == 0 or n == 0:
                continue
            if self.gram_evs is not None:
                import torch
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            o.gram(self.zb, self.np_, kpad_c, self.qmax, self.gram)
            if self.gram_evs is not None:
                ev[1].record()
                self.gram_evs.append(ev)
        self._mark("zquant_gram")
        if upto == "step4":
            self._check_deferred()
            return
        # the previous pass's deferred phasing starts once this pass's Gram is done
        if not profile:
            self._issue_pending()
        self._step5()
        idx, self.d2, cnt = self.idx_l, self.d2_l, self.cnt_l
        self._mark("topk")
        if upto == "step5":
            self.idx_out, self.cnt_out = idx, cnt
            self._check_deferred()
            return
        # ---- step 6: dipCN (scales as printed "%.2f", neighbour gather) ----
        lane = None if profile else self._lanes
        if lane is None:
            self.finish()                     # a deferred phasing of an earlier pass first
        b = self._cur ^ 1 if lane is not None else self._cur
        if self._ev_free[b] is not None:
            import torch
            torch.cuda.current_stream().wait_event(self._ev_free[b])   # the phasing that read it is done
            self._ev_free[b] = None
        o.round_decimals(self.rm, n, 2, self.scale2)
        o.gather(self.scale2, idx, n * max(self.k, 1), self.nscale)
        if hasattr(o, "sel_read"):
            o.dipcn(n, self.reads, self.has, self.scale2, idx, self.nscale, cnt, max(self.k, 1), self.n_nbr,
                    self._dips[b], self.valid, defer=self.dstat[2:4])
            self._ddef = True
        elif o.dipcn(n, self.reads, self.has, self.scale2, idx, self.nscale, cnt, max(self.k, 1), self.n_nbr,
                     self._dips[b], self.valid):
            raise ZeroDivisionError("float division by zero")
        self._cur = b
        self._mark("dipcn")
        # ---- step 7: level-scheduled Gauss-Seidel phasing + imputation ----
        if lane is not None:
            self._pending = b                 # issued by the next pass after its Gram, or by finish()
        else:
            o.phase(n, self._dips[b], self.off, self.nbr, self.w, self.min_nbr, self.n_iters, self.sched,
                    self._haps[b], self._imps[b], self._means[b])
            self._out = b
        self._mark("phase")
        self.idx_out, self.cnt_out = idx, cnt
        self._check_deferred()

    def _check_deferred(self):
        """The statuses of this pass's zquant and dipCN, read once everything is
        queued (the host waits for dipCN; the phasing may still run): |z| out
        of range raises, an overflowed int16 escape list reruns the step-4
        output as int32 (the panel and the Gram are already right), a zero
        division raises as the reference does."""
        zdef, ddef = self._zdef, self._ddef
        self._zdef = self._ddef = None
        if zdef is None and ddef is None:
            return
        h = self.dstat.cpu().numpy()
        if zdef is not None:
            of, ne = int(h[0]) & 0xFFFFFFFF, int(h[1])
            if of & 1:
                raise _abi.GridNativeError("z-score outside the int32 hundredths range")
            if of & 2:
                q, qc, ldc, a, b, s0, s1, sel_c, cm_c = zdef
                self._zquant32(q, qc, ldc, a, b, s0, s1, sel_c, cm_c)
            else:
                self.nesc = ne
        if ddef is not None and int(h[2]) & 0xFFFFFFFF:
            raise ZeroDivisionError("float division by zero")

    def _step5(self):
        """Step 5's tail, from the accumulated Gram (the cohort split: from
        this rank's two segments) to the neighbour lists idx_l / d2_l / cnt_l:
        full rows (mirror), reduce-scatter by row blocks, top-k."""
        o, n = self.ops, self.n
        if self.split == "cohort":
            self._step5_cohort()
        elif self.full_rows:
            self.comm.all_reduce_sum(self.gram[: self.np_])
            o.mirror(self.gram, self.np_)
            o.diag(self.gram, self.np_, n, self.norms)
            o.topk_rows(self.gram, self.np_, self.norms, n, self.k, 0, n, self.idx_l, self.d2_l, self.cnt_l)
        elif self.comm is not None:
            o.mirror(self.gram, self.np_)
            o.diag(self.gram, self.np_, n, self.norms)
            self.comm.all_reduce_sum(self.norms)
            self._step5_segments()
        else:
            o.mirror(self.gram, self.np_)
            o.diag(self.gram, self.np_, n, self.norms)
            o.topk_rows(self.gram, self.np_, self.norms, n, self.k, 0, n, self.idx_l, self.d2_l, self.cnt_l)

    def _step5_segments(self):
        """Sharded step 5: reduce-scatter the upper-triangle segments (each
        rank sends W segment pairs, receives its own two, summed over ranks),
        then, for k + 1 <= 16, row and column candidates per segment, an
        all-gather of the candidate lists, and the exact merge into every
        row's neighbours on every rank (grid_knn_seg_topk /
        grid_knn_seg_merge); above that, the row exchange (_seg_rows)."""
        o, n, W, B, npw, np_ = self.ops, self.n, self.world, self.B, self.npw, self.np_
        tail = self._seg_rows if self.row_exchange else self._seg_candidates
        if hasattr(o, "seg_pack"):
            o.seg_pack(self.gram, np_, W, B, self.seg_send)
            self.comm.reduce_scatter_sum(self.seg_recv, self.seg_send)
            self._mark("reduce_scatter")
            tail()
            return
        send = self.seg_send.view(W, self.seg_len)
        for q in range(W):                       # rank q's slot: its blocks q and 2W-1-q
            off = 0
            for b in (q, 2 * W - 1 - q):
                nc = (2 * W - b) * B
                dst = send[q, off:off + B * nc].view(B, nc)
                r0, r1 = b * B, min((b + 1) * B, np_)
                cv = max(min(np_, npw) - b * B, 0)
                if r1 > r0 and cv > 0:
                    dst[: r1 - r0, :cv].copy_(self.gram[r0:r1, b * B:b * B + cv])
                    if cv < nc:
                        dst[: r1 - r0, cv:].zero_()
                if r1 - r0 < B:
                    dst[max(r1 - r0, 0):].zero_()
                off += B * nc
        self.comm.reduce_scatter_sum(self.seg_recv, self.seg_send)
        self._mark("reduce_scatter")
        tail()

    def _cohort_plan(self, kb):
        """The cohort split's exchange rounds: per chunk index, the most
        K-blocks any rank fills (one small all-gather of every rank's used
        panel columns per chunk; the chunk bounds are known after pass C)."""
        torch = self.A.torch
        used = [kb[c + 1] - kb[c] for c in range(self.nch)] + [0] * (self.nch_x - self.nch)
        g = self.comm.all_gather(torch.tensor(used, dtype=torch.int64, device=self.zb.device)).cpu()
        g = g.view(self.world, self.nch_x)
        self.xkb = [pad_to(int(g[:, c].max()), 64) // _abi.KBW for c in range(self.nch_x)]
        self.ruse_tot = int(g.sum())

    def _cohort_gram(self, ci, used):
        """Chunk ci's panel across all ranks, piece by piece: the all-gather of
        piece p+1 is issued before the Gram of piece p, so the two overlap
        (RCCL runs on its own stream).  K-blocks this rank did not fill in the
        round's range are zeroed first (exact zeros in the integer sums)."""
        nkb = self.xkb[ci]
        if nkb == 0:
            return
        own = pad_to(used, 64) // _abi.KBW if used and self.n else 0
        if own < nkb:
            self.zb[own:nkb].zero_()
        pend = None
        for p0 in range(0, nkb, self.piece):
            pp = min(self.piece, nkb - p0)
            buf = self.gbuf[self._gslot]
            self._gslot ^= 1
            h = self.comm.all_gather_into(buf, self.zb[p0:p0 + pp], async_op=True)
            if pend is not None:
                self._gram_piece(*pend)
            pend = (buf, pp, h)
        self._gram_piece(*pend)

    def _gram_piece(self, buf, pp, h):
        """Both row segments of this rank over one gathered piece: W ranks' pp
        K-blocks each, a K-blocked panel of W * pp blocks (buf's first ones)."""
        if h is not None:
            h.wait()
        W, B, np_ = self.world, self.B, self.np_
        if self.gram_evs is not None:
            import torch
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        off = 0
        for b in self.my_blocks:
            nc = (2 * W - b) * B
            if b * B < np_:
                nr = min(B, np_ - b * B)
                self.ops.gram_rows(buf, np_, W * pp * _abi.KBW, self.qmax, b * B, nr,
                                   self.seg_recv[off:off + B * nc], nc)
                # MFMA work executed: the range's 256x128 tiles (j >= 2I) over W pp K-blocks
                ti0, nt = b * B // 256, np_ // 128
                tiles = sum(nt - 2 * i for i in range(ti0, ti0 + nr // 256))
                self.exec_flops += 2.0 * tiles * 256 * 128 * W * pp * _abi.KBW
            off += B * nc
        if self.gram_evs is not None:
            ev[1].record()
            self.gram_evs.append(ev)

    def _step5_cohort(self):
        """The cohort split's segments are complete on their rank: mirror their
        diagonal blocks, take the norms G_jj of their rows, all-gather the
        norms (2B int64 per rank), then the shared candidate path."""
        o, W, B, np_ = self.ops, self.world, self.B, self.np_
        self.norms_l.zero_()
        off = 0
        for slot, b in enumerate(self.my_blocks):
            nc = (2 * W - b) * B
            if b * B < np_:
                seg, nr = self.seg_recv[off:off + B * nc], min(B, np_ - b * B)
                o.mirror_ld(seg, nr, nc)
                o.diag(seg, nc, nr, self.norms_l[slot])
            off += B * nc
        torch = self.A.torch
        ng = self.comm.all_gather(self.norms_l)                 # [W][2][B]
        sel_q = torch.tensor([q for q, _ in self.blk_src], device=ng.device)
        sel_s = torch.tensor([s_ for _, s_ in self.blk_src], device=ng.device)
        self.norms.copy_(ng[sel_q, sel_s].reshape(-1)[:np_])
        self._mark("gram_rows")
        if self.row_exchange:
            self._seg_rows()
        else:
            self._seg_candidates()

    def _seg_rows(self):
        """k + 1 above the candidate lists: complete rows instead.  Row block
        b's segment lacks columns [0, b B), which are transposed tiles of the
        segments b' < b (include/grid_abi.h states the exchange rule): pack
        this rank's two segments' tiles, one all-to-all of 2 B^2 int64 per
        rank pair, fill this rank's two row blocks, select from them with the
        row kernels, all-gather the lists and order them by global row.  Every
        rank issues the same collectives, whatever its blocks hold."""
        o, n, W, B, npw = self.ops, self.n, self.world, self.B, self.npw
        torch = self.A.torch
        kk, n1 = max(self.k, 1), max(n, 1)
        segs, off = [], 0
        for b in self.my_blocks:
            nc = (2 * W - b) * B
            segs.append((b, self.seg_recv[off:off + B * nc], nc))
            off += B * nc
        for b, seg, nc in segs:
            o.seg_tiles_pack(seg, nc, B, W, b, self.x_send)
        self.comm.all_to_all(self.x_recv, self.x_send, [2 * B * B] * W, [2 * B * B] * W)
        self._mark("row_exchange")
        for slot, (b, seg, nc) in enumerate(segs):
            o.seg_rows_fill(seg, nc, self.x_recv, B, W, b, self.rows_l[slot], npw)
            nr = min(max(n - b * B, 0), B)
            if nr:                                      # a padding block's lists keep (-1, 0, 0)
                o.topk_rows(self.rows_l[slot], npw, self.norms, n, self.k, b * B, nr, self.bidx_l[slot],
                            self.bd2_l[slot], self.bcnt_l[slot])
        ig = self.comm.all_gather(self.bidx_l)              # [W][2][B][k]
        dg = self.comm.all_gather(self.bd2_l)
        cg = self.comm.all_gather(self.bcnt_l)              # [W][2][B]
        sel_q = torch.tensor([q for q, _ in self.blk_src], device=ig.device)
        sel_s = torch.tensor([s_ for _, s_ in self.blk_src], device=ig.device)
        self.idx_l.copy_(ig[sel_q, sel_s].reshape(-1, kk)[:n1])     # [2W][B][k] = global row order
        self.d2_l.copy_(dg[sel_q, sel_s].reshape(-1, kk)[:n1])
        self.cnt_l.copy_(cg[sel_q, sel_s].reshape(-1)[:n1])

    def _seg_candidates(self):
        """Row and column candidates of this rank's two (complete) segments,
        their all-gather, and the exact merge into every row's neighbours."""
        o, n, W, B, npw = self.ops, self.n, self.world, self.B, self.npw
        torch = self.A.torch
        off = 0
        for slot, b in enumerate(self.my_blocks):
            nc = (2 * W - b) * B
            o.seg_topk(self.seg_recv[off:off + B * nc], nc, B, nc, self.norms, n, self.k, b * B, b * B,
                       self.rowc_l[slot], self.colc_l[slot])
            off += B * nc
        rg = self.comm.all_gather(self.rowc_l)              # [W][2][B][K1]
        cg = self.comm.all_gather(self.colc_l)              # [W][2][npw][K1]
        sel_q = torch.tensor([q for q, _ in self.blk_src], device=rg.device)
        sel_s = torch.tensor([s_ for _, s_ in self.blk_src], device=rg.device)
        rowc = rg[sel_q, sel_s].contiguous()                # [2W][B][K1] = global row order
        colc = cg[sel_q, sel_s].contiguous()                # [2W][npw][K1]
        o.seg_merge(rowc, colc, npw, B, n, self.k, self.idx_l, self.d2_l, self.cnt_l)

    def _issue_pending(self):
        """Issue the deferred phasing of _dips[_pending] on the phase lane,
        after everything issued so far on the main stream."""
        if self._pending is None:
            return
        import torch
        b, self._pending = self._pending, None
        pops, pstream = self._lanes[b % len(self._lanes)]
        ev = torch.cuda.Event()
        ev.record()
        pstream.wait_event(ev)
        pops.phase(self.n, self._dips[b], self.off, self.nbr, self.w, self.min_nbr, self.n_iters, self.sched,
                   self._haps[b], self._imps[b], self._means[b])
        done = torch.cuda.Event()
        done.record(pstream)
        self._ev_free[b] = done
        self._ev_phase[b] = done
        self._out = b

    def finish(self):
        """Issue the last pass's deferred phasing and order the main stream
        after every phasing still running (hap / imp / mean are then the last
        pass's once the stream syncs)."""
        self._issue_pending()
        if self._ev_phase:
            import torch
            for ev in self._ev_phase.values():
                torch.cuda.current_stream().wait_event(ev)
            self._ev_phase = {}

    def _chunk_bounds(self, r_loc):
        """Per chunk: the range [sb[c], sb[c+1]) of selected indices whose
        columns lie in it (sel ascends) and kb[c] = panel columns used before
        it (colmap ranks ascend)."""
        if self.nch == 1:
            return [0, r_loc], [0, self.ruse_loc]
        torch = self.A.torch
        sel = self.sel[:r_loc]
        cuts = torch.tensor([a for a, _ in self.chunks[1:]], dtype=sel.dtype, device=sel.device)
        inner = torch.searchsorted(sel, cuts) if r_loc else torch.zeros_like(cuts, dtype=torch.int64)
        used = torch.cumsum((self.colmap[:r_loc] >= 0).to(torch.int64), 0) if r_loc else None
        kin = used[(inner - 1).clamp(min=0)] * (inner > 0) if r_loc else torch.zeros_like(inner)
        sb = [0] + [int(x) for x in inner.tolist()] + [r_loc]
        kb = [0] + [int(x) for x in kin.tolist()] + [self.ruse_loc]
        return sb, kb

    def _zquant(self, q, qc, ldc, a, b, s0, s1, sel_c, cm_c):
        """z of the chunk's selected columns [s0, s1): the step-4 output (int16
        codes + escapes, or int32) and the bf16 panel columns colmap says."""
        o, n, rc = self.ops, self.n, s1 - s0
        if rc == 0:
            return
        mu_c = self.mu[a:b]
        if self.keep_z:
            zcol, ld_zq = s0, max(self.ml, 1)
        else:
            zcol, ld_zq = 0, rc
        if self.zq_is16 and (isinstance(q, Depth16) or ldc % 4 == 0):
            # keep_z: the escapes of every chunk accumulate (flat indices into
            # the whole output); streamed: each chunk's list is consumed by
            # on_z_chunk before the next, so every chunk starts at 0 and the
            # capacity (sized for one chunk's cells) applies per chunk
            e0 = self.nesc if self.keep_z else 0
            cap = self.esc_idx.numel() - e0
            zt = self.zq16.view(-1)[zcol:]
            if self.nch == 1 and self.on_z_chunk is None and hasattr(o, "sel_read"):
                # one chunk, nobody consumes the codes before the pass ends: the
                # status is read at the end of the pass (_check_deferred), so the
                # Gram and the rest of the pass queue behind zquant without a sync
                o.zquant16(qc, n, ldc, sel_c, rc, self.rm, mu_c, self.scale, zt, ld_zq, cm_c, self.qmax, self.zb,
                           self.np_, self.esc_idx[e0:], self.esc_val[e0:], defer=self.dstat[0:2])
                self._zdef = (q, qc, ldc, a, b, s0, s1, sel_c, cm_c)
                return
            of, ne = o.zquant16(qc, n, ldc, sel_c, rc, self.rm, mu_c, self.scale, zt, ld_zq, cm_c, self.qmax, self.zb,
                                self.np_, self.esc_idx[e0:], self.esc_val[e0:])
            if of & 1:
                raise _abi.GridNativeError("z-score outside the int32 hundredths range")
            if not of & 2:
                if ne and zcol:
                    self.esc_idx[e0:e0 + ne] += zcol             # flat index in the whole output
                self.nesc = e0 + ne
                if not self.keep_z and self.on_z_chunk is not None:
                    self.on_z_chunk(self.zq16, ld_zq, s0, s1, self.esc_idx[e0:e0 + ne], self.esc_val[e0:e0 + ne])
                return
            if self.nch > 1:
                raise _abi.GridNativeError(f"more than {cap} int16 escapes (|z| > 327.65) in chunk [{s0}, {s1})")
        self._zquant32(q, qc, ldc, a, b, s0, s1, sel_c, cm_c)

    def _zquant32(self, q, qc, ldc, a, b, s0, s1, sel_c, cm_c):
        o, n, rc = self.ops, self.n, s1 - s0
        mu_c = self.mu[a:b]
        zcol, ld_zq = (s0, max(self.ml, 1)) if self.keep_z else (0, rc)
        self.zq_is16 = False            # int32 output: no int16 codes (unaligned input, or too many escapes)
        if self.zq is None:
            self.zq = self.A.empty(tuple(self.zq16.shape), I4)
        of = o.zquant(qc if not isinstance(q, Depth16) else q, n, ldc, sel_c, rc, self.rm, mu_c, self.scale,
                      self.zq.view(-1)[zcol:], ld_zq, cm_c, self.qmax, self.zb, self.np_)
        if of & 1:
            raise _abi.GridNativeError("z-score outside the int32 hundredths range")


def zq16_to_int32(torch, zq16, esc_idx, esc_val):
    """int16 step-4 codes (+ escapes) -> int32 hundredths with the
    GRID_ZQ_NAN / GRID_ZQ_NEG0 sentinels."""
    z = zq16.to(torch.int32)
    z[zq16 == _abi.ZQ16_NAN] = _abi.ZQ_NAN
    z[zq16 == _abi.ZQ16_NEG0] = _abi.ZQ_NEG0
    if esc_idx.numel():
        z.view(-1)[esc_idx] = esc_val
    return z
