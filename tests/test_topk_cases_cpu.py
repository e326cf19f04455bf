"""The neighbour-selection cases of tests/topk_cases.py on the CPU: the NumPy
restatement of the kernels (tests/cpu_ops.NumpyOps.topk_rows, seg_topk,
seg_merge) through every case and the segment helper, equal to ref_topk.
Proves the helper and the reference before tests/test_gpu_topk.py runs them
against the HIP kernels, and pins NumpyOps (the sharded chain's CPU ops) to
the tie rule."""
import numpy as np
import pytest
import torch

from oracle import steps
from tests import topk_cases as tc
from tests.cpu_ops import NumpyOps

KS = [1, 6, 15, 16, 17, 31, 32, 40]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rows(gram, norms, n, k, row0=0, nrows=None):
    nrows = n - row0 if nrows is None else nrows
    np_ = gram.shape[0]
    idx = torch.full((nrows, k), 77, dtype=torch.int32)
    d2 = torch.full((nrows, k), 77, dtype=torch.int64)
    cnt = torch.full((nrows,), 77, dtype=torch.int32)
    NumpyOps().topk_rows(_t(gram[row0:]), np_, _t(norms), n, k, row0, nrows, idx, d2, cnt)
    return idx.numpy(), d2.numpy(), cnt.numpy()


def _segs(gram, norms, n, W, B, k):
    o = NumpyOps()
    npw = 2 * W * B
    rowc = torch.zeros((2 * W, B, tc.K1), dtype=torch.int64)
    colc = torch.zeros((2 * W, npw, tc.K1), dtype=torch.int64)
    tn = _t(norms)
    for b, s in enumerate(tc.segments(gram, norms, n, W, B)):
        o.seg_topk(_t(s["seg"]), s["ld"], s["nrows"], s["ncols"], tn, n, k, s["r0"], s["c0"], rowc[b], colc[b])
    idx = torch.full((n, k), 77, dtype=torch.int32)
    d2 = torch.full((n, k), 77, dtype=torch.int64)
    cnt = torch.full((n,), 77, dtype=torch.int32)
    o.seg_merge(rowc, colc, npw, B, n, k, idx, d2, cnt)
    return idx.numpy(), d2.numpy(), cnt.numpy()


def _same(got, exp):
    for g, e, what in zip(got, exp, ("idx", "d2", "cnt")):
        assert np.array_equal(g, e), what


def test_ref_topk_equals_oracle_knn_exact():
    """ref_topk against the oracle's own restatement, on samples with ties."""
    q = np.random.default_rng(9).integers(-2, 3, size=(70, 3))
    _, _, D = tc.from_matrix(q)
    for k in (1, 7, 69, 80):
        idx, d2, cnt = tc.ref_topk(D, k)
        exp = steps.knn_exact(q, k)
        for i in range(70):
            assert idx[i, : cnt[i]].tolist() == [j for j, _ in exp[i]]
            assert d2[i, : cnt[i]].tolist() == [s for _, s in exp[i]]
            assert (idx[i, cnt[i]:] == -1).all() and (d2[i, cnt[i]:] == 0).all()


def test_ref_topk_self_rule():
    """Self is dropped only if it is among the first k + 1 by (d2, j)."""
    D = np.zeros((5, 5), dtype=np.int64)
    idx, d2, cnt = tc.ref_topk(D, 2)
    assert idx.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]]     # rows 3, 4: self not among 0, 1, 2
    assert cnt.tolist() == [2] * 5
    idx, _, cnt = tc.ref_topk(D, 7)
    assert idx[4].tolist() == [0, 1, 2, 3, -1, -1, -1] and cnt.tolist() == [4] * 5


def test_cases_are_what_they_claim():
    gram, norms, D = tc.wide(130)
    assert gram.shape == (192, 192) and norms.shape == (130,)
    assert np.array_equal(D, norms[:, None] + norms[None, :] - 2 * gram[:130, :130])
    assert ((D[:, 0] ^ D[:, 1]) == 1).all() and ((D[:, 0] ^ D[:, 2]) == 1 << 43).all()
    assert D.max() == tc.KEY_TOP and (D & 1).any()
    # pad columns would win: d2 <= 1 against a zero norm
    assert (norms[:, None] - 2 * gram[:130, 130:]).max() <= 1
    _, _, D = tc.dup_cohort(300)
    assert ((D == 0).sum(axis=1) >= 40).sum() >= 40
    _, _, D = tc.paired(100)
    assert (np.sort(D, axis=1)[:, 0::2] == np.sort(D, axis=1)[:, 1::2]).all()
    _, _, D = tc.tie_cohort(300)
    assert len(np.unique(D)) <= 49


@pytest.mark.parametrize("case", sorted(tc.INT_CASES))
@pytest.mark.parametrize("n", [1, 2, 17, 70])
def test_numpy_topk_rows(case, n):
    gram, norms, D = tc.INT_CASES[case](n)
    order = tc.row_orders(D)
    for k in KS:
        _same(_rows(gram, norms, n, k), tc.ref_topk(D, k, order=order))


def test_numpy_topk_rows_band():
    gram, norms, D = tc.dup_cohort(90)
    rows = np.arange(31, 31 + 40)
    _same(_rows(gram, norms, 90, 9, 31, 40), tc.ref_topk(D, 9, rows=rows))


# W = 16 at B = 4: 32 row blocks (the thread-per-row merge's range on the GPU);
# n leaves the last block partial, at W = 3 a block of pure padding too
@pytest.mark.parametrize("case", ["ties", "dups"])
@pytest.mark.parametrize("W,B,n", [(1, 64, 100), (2, 16, 61), (3, 12, 58), (16, 4, 126), (20, 4, 157)])
def test_numpy_segments(case, W, B, n):
    gram, norms, D = tc.INT_CASES[case](n)
    order = tc.row_orders(D)
    for k in (1, 6, 15):
        exp = tc.ref_topk(D, k, order=order)
        _same(_segs(gram, norms, n, W, B, k), exp)
        _same(_rows(gram, norms, n, k), exp)
