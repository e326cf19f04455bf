"""Shared cases and a plain reference for the neighbour-selection tests
(tests/test_topk_cases_cpu.py, tests/test_gpu_topk.py): the step-5 rule on
rows of exact distances, with ties, duplicate samples and the multi-GPU
segment layout.  Written independently of tests/cpu_ops.py.

The rule (find_neighbors.py:216-225, oracle/steps.py:knn_exact): order row i
by (d2, j), take the first min(k + 1, n), drop i only if it is among them,
keep the first k.
"""
import numpy as np

K1 = 16                     # GRID_SEG_K1: keys per candidate list of the segment path
KEY_TOP = 2 ** 44 - 2       # the largest even distance the packed (d2 << 20 | j) key holds


def pad_to(x, a):
    return -(-x // a) * a


def row_orders(D, rows=None):
    """lexsort((j, D[i])) of the given rows of D: [len(rows)][n]."""
    D = np.asarray(D)
    n = D.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    sub = D[rows]
    return np.lexsort((np.broadcast_to(np.arange(n), sub.shape), sub))


def ref_topk(D, k, rows=None, order=None):
    """Neighbours of ``rows`` (default: all) of the n x n distances D (int64
    or float64): (idx [rows][k] int32, d2 [rows][k] of D's dtype, cnt [rows]
    int32).  Unused slots hold idx = -1 and d2 = 0 (topk_emit's convention).
    ``order``: row_orders(D, rows), when a caller runs several k on one D."""
    D = np.asarray(D)
    n = D.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    if order is None:
        order = row_orders(D, rows)
    idx = np.full((len(rows), k), -1, dtype=np.int32)
    d2 = np.zeros((len(rows), k), dtype=D.dtype)
    cnt = np.zeros(len(rows), dtype=np.int32)
    for t, i in enumerate(rows):
        take = order[t, : min(k + 1, n)]
        if i in take:
            take = take[take != i]
        take = take[:k]
        idx[t, : len(take)] = take
        d2[t, : len(take)] = D[i, take]
        cnt[t] = len(take)
    return idx, d2, cnt


# ---- integer cases: (gram int64 [np][np], norms int64 [n], D int64 [n][n]) ----
def _finish(g, norms, n):
    """Pad the n x n Gram block to np = pad_to(n, 64) with cells that would win
    if a kernel read them as samples (d2 = 0 or 1 against a zero norm), and
    check D[i][j] = norms[i] + norms[j] - 2 gram[i][j] >= 0."""
    np_ = pad_to(n, 64)
    gram = np.empty((np_, np_), dtype=np.int64)
    gram[:n, :n] = g
    gram[:n, n:] = (norms // 2)[:, None]
    gram[n:, :n] = (norms // 2)[None, :]
    gram[n:, n:] = 0
    D = norms[:, None] + norms[None, :] - 2 * gram[:n, :n]
    assert D.min() >= 0 and D.max() <= KEY_TOP
    return gram, np.ascontiguousarray(norms, dtype=np.int64), D


def from_matrix(q):
    """Samples q [n][r] (small ints): the Gram q q^T and its diagonal."""
    q = np.asarray(q, dtype=np.int64)
    g = q @ q.T
    return _finish(g, np.diag(g).copy(), q.shape[0])


def from_distances(D, norms=None):
    """A Gram that yields the distances D exactly: gram = -D // 2 with zero
    norms (D even), or, given norms, gram = -(D - norms_i - norms_j) // 2 (the
    parity of D[i][j] must then be that of norms_i + norms_j).  D need not be
    symmetric: the row kernels read rows only."""
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[0]
    norms = np.zeros(n, dtype=np.int64) if norms is None else np.asarray(norms, dtype=np.int64)
    e = D - norms[:, None] - norms[None, :]
    assert not (e & 1).any()
    gram, norms, D2 = _finish(-(e // 2), norms, n)
    assert np.array_equal(D2, D)
    return gram, norms, D


def tie_cohort(n, seed=1):
    """r = 3 columns of values in [-2, 2]: 125 distinct samples at most, d2 in
    [0, 48], so nearly every distance ties and every sample has exact copies."""
    return from_matrix(np.random.default_rng(seed).integers(-2, 3, size=(n, 3)))


def dup_cohort(n, seed=2, copies=40):
    """tie_cohort with ``copies`` rows, spread over the whole index range, equal
    to one row: a copy has up to copies - 1 (and more) neighbours at d2 = 0 with
    smaller index, so self is not first and (k + 1 < copies) often not in the
    list at all."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, size=(n, 3))
    c = min(copies, n)
    at = np.sort(rng.choice(n, c, replace=False))
    q[at] = q[at[0]]
    return from_matrix(q)


def all_equal(n, d=6):
    """Every distance (the diagonal too) equal: keys differ in the index bits only."""
    return from_distances(np.full((n, n), d, dtype=np.int64))


def wide(n, seed=3):
    """Distances over the whole key width.  Each cell draws a width s from
    {4, 12, ..., 44} and then a value below 2^s, so the k smallest of a row
    cluster at every scale (the radix select's digits all decide).  Odd columns
    have norm 1 (D[i][j] has the parity of i + j).  In every row, column 1
    differs from column 0 in bit 0 only and column 2 in bit 43 only; the
    largest value KEY_TOP is present."""
    rng = np.random.default_rng(seed)
    s = rng.choice(np.arange(4, 45, 8), size=(n, n))
    D = rng.integers(0, 2 ** 62, size=(n, n)) >> (62 - s)
    ij = np.add.outer(np.arange(n), np.arange(n)) & 1
    D = (D & ~np.int64(1)) | ij
    if n > 2:
        D[:, 0] = (D[:, 0] & (2 ** 43 - 4)) | (np.arange(n) & 1)
        D[:, 1] = D[:, 0] ^ 1
        D[:, 2] = D[:, 0] ^ (1 << 43)
    if n > 4:
        D[np.arange(n), 3 + ((np.arange(n) + 1) & 1)] = KEY_TOP
    D = np.minimum(D, KEY_TOP - ij)                  # odd cells <= KEY_TOP - 1
    return from_distances(D, norms=np.arange(n) & 1)


def paired(n, seed=4):
    """Every row a random permutation of 0, 0, 2, 2, 4, 4, ...: the k-th and the
    (k + 1)-th distances tie for every other k, the (k + 1)-th and the (k + 2)-th
    (the selection boundary) for the rest."""
    rng = np.random.default_rng(seed)
    D = np.stack([2 * (rng.permutation(n) // 2) for _ in range(n)]).astype(np.int64)
    return from_distances(D)


INT_CASES = {"ties": tie_cohort, "dups": dup_cohort, "all_equal": all_equal, "wide": wide, "paired": paired}


# ---- the multi-GPU segment layout ----
def segments(gram, norms, n, W, B):
    """The 2W upper-triangle row segments of the Gram as Steps47._step5_segments
    / _seg_candidates lay them out: block b is rows [bB, (b+1)B) x columns
    [bB, 2WB), row stride ld = (2W - b) B, cells outside the Gram zero.
    Returns a list of dicts with the arguments of one seg_topk call each
    (seg, ld, nrows, ncols, r0, c0); the caller writes block b's lists to
    rowc[b] of [2W][B][K1] and colc[b] of [2W][2WB][K1], then merges once with
    seg_merge(rowc, colc, 2WB, B, n, k, ...)."""
    np_ = gram.shape[0]
    npw = 2 * W * B
    assert npw >= n and norms.shape[0] == n
    full = np.zeros((npw, npw), dtype=np.int64)
    m = min(np_, npw)
    full[:m, :m] = gram[:m, :m]
    out = []
    for b in range(2 * W):
        ld = (2 * W - b) * B
        seg = np.ascontiguousarray(full[b * B:(b + 1) * B, b * B:])
        assert seg.shape == (B, ld)
        out.append(dict(seg=seg, ld=ld, nrows=B, ncols=ld, r0=b * B, c0=b * B))
    return out
