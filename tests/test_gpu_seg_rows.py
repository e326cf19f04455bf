"""The row exchange of the sharded step 5 above 16 keys (MI355X only), through
the C ABI: grid_knn_seg_tiles_pack / grid_knn_seg_rows_fill on the round-trip
shapes of tests/wide_ops.py (the all-to-all done as a host permutation),
grid_knn_topk_rows on the assembled row blocks against topk_cases.ref_topk,
and the route Steps47 picks with HipOps."""
import numpy as np
import pytest

from tests import topk_cases as tc
from tests import wide_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from grid_amd._abi import Device
    d = Device(0)
    yield d
    d.close()


def _pack(dev):
    def pack(seg, ld, B, W, b_src, send):
        from grid_amd._abi import call
        ds, dx = dev.upload(seg), dev.upload(send)
        call("grid_knn_seg_tiles_pack", dev.ctx, ds.ptr, ld, B, W, b_src, dx.ptr)
        send[...] = dx.numpy()
    return pack


def _fill(dev):
    def fill(seg, ld, recv, B, W, b, rows, ld_rows):
        from grid_amd._abi import call
        ds, dr, do = dev.upload(seg), dev.upload(recv), dev.upload(rows)
        call("grid_knn_seg_rows_fill", dev.ctx, ds.ptr, ld, dr.ptr, B, W, b, do.ptr, ld_rows)
        rows[...] = do.numpy()
    return fill


@pytest.mark.parametrize("W,B", wide_ops.SHAPES)
def test_pack_exchange_fill_equals_definition(dev, W, B):
    """Every cell of every row block: its own row right of the block's first
    column, the transposed cell left of it (partial 32 x 32 sub-tiles in both
    directions at B = 1, 31, 33, 43; int64 values that a 32-bit move breaks)."""
    mat = wide_ops.exchange_matrix(W, B, seed=W * 100 + B)
    got = wide_ops.round_trip(mat, W, B, _pack(dev), _fill(dev), junk=0x5555555555555555)
    for b in range(2 * W):
        assert np.array_equal(got[b], wide_ops.expected_rows(mat, B, b)), b


def test_pack_equals_the_numpy_restatement(dev):
    """The send buffer itself, tile by tile and slot by slot (W = 3, B = 43)."""
    W, B = 3, 43
    mat = wide_ops.exchange_matrix(W, B, seed=9)
    for b in range(2 * W):
        seg, ld = wide_ops.segment(mat, W, B, b), (2 * W - b) * B
        exp, got = np.zeros((W, 2, B, B), np.int64), np.zeros((W, 2, B, B), np.int64)
        wide_ops.tiles_pack(seg, ld, B, W, b, exp)
        _pack(dev)(seg, ld, B, W, b, got)
        assert np.array_equal(got, exp), b


def test_bad_arguments_are_refused(dev):
    from grid_amd._abi import GridNativeError, call
    W, B = 2, 8
    seg, buf = dev.zeros((B, 4 * B), np.int64), dev.zeros((W, 2, B, B), np.int64)
    rows = dev.zeros((B, 4 * B), np.int64)
    for args in [(seg.ptr, 4 * B - 1, B, W, 0, buf.ptr), (seg.ptr, 4 * B, B, W, 4, buf.ptr),
                 (seg.ptr, 4 * B, 0, W, 0, buf.ptr), (seg.ptr, 4 * B, B, 0, 0, buf.ptr),
                 (None, 4 * B, B, W, 0, buf.ptr)]:
        with pytest.raises(GridNativeError):
            call("grid_knn_seg_tiles_pack", dev.ctx, *args)
    for args in [(seg.ptr, 4 * B - 1, buf.ptr, B, W, 0, rows.ptr, 4 * B),
                 (seg.ptr, 4 * B, buf.ptr, B, W, 0, rows.ptr, 4 * B - 1),
                 (seg.ptr, 4 * B, buf.ptr, B, W, -1, rows.ptr, 4 * B),
                 (seg.ptr, 4 * B, None, B, W, 0, rows.ptr, 4 * B)]:
        with pytest.raises(GridNativeError):
            call("grid_knn_seg_rows_fill", dev.ctx, *args)


# ---- selection from the assembled rows ----
N, W_SEL, B_SEL = 100, 3, 22          # 2WB = 132 > np = 128; block 4 holds 12 samples, block 5 none


def _symmetric(name):
    gram, norms, D = tc.INT_CASES[name](N)
    if name == "wide":                # its distances are drawn per cell: mirror the upper triangle
        gram = np.triu(gram) + np.triu(gram, 1).T
        D = np.triu(D) + np.triu(D, 1).T
        assert np.array_equal(D, norms[:, None] + norms[None, :] - 2 * gram[:N, :N])
    assert np.array_equal(gram, gram.T) and np.array_equal(D, D.T)
    return gram, norms, D


@pytest.mark.parametrize("name", ["ties", "dups", "all_equal", "wide"])
def test_selection_from_assembled_rows(dev, name):
    """Steps47._seg_rows through the C ABI: tiles of the 2W segments packed
    and permuted, each block's rows filled and grid_knn_topk_rows run on them
    (the 32-key kernel at k = 16 and 31, the radix kernel from 32, k + 1 > n
    at 105); every block's lists equal ref_topk's rows of that block."""
    from grid_amd._abi import call
    W, B, npw = W_SEL, B_SEL, 2 * W_SEL * B_SEL
    gram, norms, D = _symmetric(name)
    segs = tc.segments(gram, norms, N, W, B)
    sends = []
    for p in range(W):
        send = np.zeros((W, 2, B, B), np.int64)
        for b in (p, 2 * W - 1 - p):
            _pack(dev)(segs[b]["seg"], segs[b]["ld"], B, W, b, send)
        sends.append(send)
    recvs = wide_ops.host_all_to_all(sends)
    dn = dev.upload(norms)
    order = tc.row_orders(D)
    for b in range(2 * W):
        rows = np.full((B, npw), 0x5555555555555555, np.int64)
        _fill(dev)(segs[b]["seg"], segs[b]["ld"], np.ascontiguousarray(recvs[wide_ops.own(b, W)]), B, W, b, rows, npw)
        nr = min(max(N - b * B, 0), B)
        assert np.array_equal(rows[:nr, :N], gram[b * B:b * B + nr, :N]), b
        if nr == 0:                   # a padding block: Steps47 selects nothing from it
            continue
        dr = dev.upload(rows)
        for k in (16, 31, 32, 40, 99, 105):
            idx = dev.alloc((B, k), np.int32).fill_bytes(0x55)
            d2 = dev.alloc((B, k), np.int64).fill_bytes(0x55)
            cnt = dev.alloc(B, np.int32).fill_bytes(0x55)
            call("grid_knn_topk_rows", dev.ctx, dr.ptr, npw, dn.ptr, N, k, b * B, nr, idx.ptr, d2.ptr, cnt.ptr)
            e_idx, e_d2, e_cnt = tc.ref_topk(D, k, rows=np.arange(b * B, b * B + nr), order=order[b * B:b * B + nr])
            assert np.array_equal(idx.numpy()[:nr], e_idx), (b, k)
            assert np.array_equal(d2.numpy()[:nr], e_d2), (b, k)
            assert np.array_equal(cnt.numpy()[:nr], e_cnt), (b, k)


def test_steps47_takes_the_row_exchange_with_hipops():
    import torch

    from grid_amd._abi import Device
    from grid_amd.fused import HipOps, SimComm, Steps47, TorchAlloc
    dev = Device(0)
    dev.set_stream(torch.cuda.current_stream())
    mk = lambda **kw: Steps47(HipOps(dev), TorchAlloc(0), 48, 8192, 0, 8192, k=20, comm=SimComm(2, 0), **kw)  # noqa: E731
    st = mk()
    assert st.row_exchange and not st.full_rows
    assert tuple(st.x_send.shape) == (2, 2, st.B, st.B) and tuple(st.rows_l.shape) == (2, st.B, st.npw)
    st = mk(split="cohort")
    assert st.row_exchange and st.B % 256 == 0
    st = mk(step5_wide="allreduce")
    assert st.full_rows and not st.row_exchange
    assert not Steps47(HipOps(dev), TorchAlloc(0), 48, 8192, 0, 8192, k=10, comm=SimComm(2, 0)).row_exchange
