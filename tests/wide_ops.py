"""``NumpyOps`` plus the two operations of the sharded step 5's row exchange
(k + 1 above the 16-key candidate lists): NumPy restatements of
grid_knn_seg_tiles_pack / grid_knn_seg_rows_fill written from the exchange
rule of include/grid_abi.h, and the rule's slot function in Python.
TEST INFRASTRUCTURE ONLY.

The rule: 2W blocks of B rows, own(b) = b if b < W else 2W-1-b holds segment
b (rows of block b x columns >= b B).  Row block b lacks columns [0, b B):
for b' < b that part is the tile T(b', b)[u][c] = seg_b'[c][(b - b') B + u].
The pair p = own(b') -> q = own(b) carries, in slots 0 and 1,
p < q: T(p, q), T(p, 2W-1-q); p > q: T(p, 2W-1-q), T(2W-1-p, 2W-1-q);
p = q: T(p, 2W-1-p) alone."""
import numpy as np

from tests.cpu_ops import NumpyOps


def own(b, W):
    return b if b < W else 2 * W - 1 - b


def tile_slot(bs, b, W):
    """Slot (0 or 1) of tile T(bs, b), bs < b, in the pair own(bs) -> own(b)."""
    assert 0 <= bs < b < 2 * W
    p, q = own(bs, W), own(b, W)
    if p < q:                      # both tiles come from block p: the low target block first
        return 0 if b == q else 1
    if p > q:                      # both go to block 2W-1-q: the low source block first
        return 0 if bs == p else 1
    return 0


def _a(t):
    return t if isinstance(t, np.ndarray) else t.numpy()


def tiles_pack(seg, ld, B, W, b_src, send):
    s = _a(seg).reshape(-1)[: B * ld].reshape(B, ld)
    out = _a(send).reshape(W, 2, B, B)
    for b in range(b_src + 1, 2 * W):
        out[own(b, W), tile_slot(b_src, b, W)] = s[:, (b - b_src) * B:(b - b_src + 1) * B].T


def rows_fill(seg, ld, recv, B, W, b, rows, ld_rows):
    s = _a(seg).reshape(-1)[: B * ld].reshape(B, ld)
    rv = _a(recv).reshape(W, 2, B, B)
    out = _a(rows).reshape(-1)[: B * ld_rows].reshape(B, ld_rows)
    out[:, b * B:2 * W * B] = s[:, : (2 * W - b) * B]
    for bs in range(b):
        out[:, bs * B:(bs + 1) * B] = rv[own(bs, W), tile_slot(bs, b, W)]


def exchange_matrix(W, B, seed=0):
    """A non-symmetric int64 matrix [2WB][2WB] for the pack / exchange / fill
    checks: values up to 2^62 in magnitude, negatives too, so a 32-bit
    truncation or a swapped transpose shows in every cell."""
    rng = np.random.default_rng(seed)
    return rng.integers(-(2 ** 62), 2 ** 62, (2 * W * B, 2 * W * B), dtype=np.int64)


def segment(mat, W, B, b):
    """Segment b of ``mat``: rows of block b x columns [b B, 2WB), contiguous."""
    return np.ascontiguousarray(mat[b * B:(b + 1) * B, b * B:])


def expected_rows(mat, B, b):
    """Block b's complete rows by the definition: its own row right of the
    block's first column, the transposed cell left of it."""
    rows = mat[b * B:(b + 1) * B].copy()
    rows[:, : b * B] = mat[: b * B, b * B:(b + 1) * B].T
    return rows


def host_all_to_all(sends):
    """recv[q][p] = send[p][q] for per-rank buffers [W][2][B][B]."""
    W = len(sends)
    return [np.stack([sends[p][q] for p in range(W)]) for q in range(W)]


# (W, B) of the round-trip checks: B = 1, B off the 32-cell sub-tile on both
# sides, one and several sub-tiles, W = 1 (one pair, one tile) up to 8
SHAPES = [(1, 1), (1, 33), (2, 31), (3, 43), (2, 64), (8, 32)]


def round_trip(mat, W, B, pack, fill, junk=-1):
    """All W ranks in one process: pack both segments of every rank into its
    send buffer (zeroed once, as Steps47 allocates it), permute on the host,
    fill both blocks of every rank into rows preset to ``junk``; returns
    {block: rows [B][2WB]}.  ``pack`` / ``fill`` take NumPy arrays with the
    operations' own argument lists and write send / rows in place."""
    npw = 2 * W * B
    sends = []
    for p in range(W):
        send = np.zeros((W, 2, B, B), np.int64)
        for b in (p, 2 * W - 1 - p):
            pack(segment(mat, W, B, b), (2 * W - b) * B, B, W, b, send)
        sends.append(send)
    recvs = host_all_to_all(sends)
    got = {}
    for q in range(W):
        for b in (q, 2 * W - 1 - q):
            rows = np.full((B, npw), junk, np.int64)
            fill(segment(mat, W, B, b), (2 * W - b) * B, np.ascontiguousarray(recvs[q]), B, W, b, rows, npw)
            got[b] = rows
    return got


class WideOps(NumpyOps):
    def seg_tiles_pack(self, seg, ld, B, W, b_src, send):
        tiles_pack(seg, ld, B, W, b_src, send)

    def seg_rows_fill(self, seg, ld, recv, B, W, b, rows, ld_rows):
        rows_fill(seg, ld, recv, B, W, b, rows, ld_rows)

    def topk_rows(self, rows, ld, norms, n, k, row0, nrows, idx, d2, cnt):
        # grid_knn_topk_rows refuses a row block outside the samples (a padding block starts beyond n)
        assert n > 0 and ld >= n and row0 >= 0 and nrows >= 0 and row0 + nrows <= n
        super().topk_rows(rows, ld, norms, n, k, row0, nrows, idx, d2, cnt)
