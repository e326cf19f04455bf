"""The kernels that pick the neighbours out of distance rows (MI355X only),
called directly through the C ABI on the cases of tests/topk_cases.py:

* grid_knn_topk_rows: k_topk_small<16>, k_topk_small<32>, k_topk_radix at both
  edges of every k range, row lengths on both sides of the unrolled loop and
  off the 256 stride, k >= n, row bands, ld > np, the last admitted k;
* grid_knn_topk_d2: the same lists from fp64 rows, and engine.knn_values on
  fp64 inputs whose distances differ far below the largest one;
* grid_knn_seg_topk + grid_knn_seg_merge in the layout of the sharded chain:
  the wave-per-row merge up to its 31 lists, the thread-per-row merge beyond.

Every comparison is np.array_equal on idx, d2 and cnt against
topk_cases.ref_topk (or oracle.steps.knn_direct_f64): ties, duplicate
samples and all-equal rows are ordered by (d2, j), nothing is approximate.
"""
import numpy as np
import pytest

from oracle import steps
from tests import topk_cases as tc

pytestmark = pytest.mark.gpu

KS = [1, 14, 15, 16, 17, 30, 31, 32, 63, 64, 255, 256, 500]
NS = [1, 2, 17, 33, 255, 256, 257, 1023, 1024, 1025, 1300]
N_CASE = 700                 # > 501: k = 500 selects 501 keys (the radix kernel's 512-key sort)


@pytest.fixture(scope="module")
def dev():
    from grid_amd._abi import Device
    d = Device(0)
    yield d
    d.close()


_cases = {}


def case(name, n):
    """(gram, norms, D, row orders) of a topk_cases case, built once."""
    if (name, n) not in _cases:
        gram, norms, D = tc.INT_CASES[name](n)
        _cases[name, n] = (gram, norms, D, tc.row_orders(D))
    return _cases[name, n]


def _outs(dev, nrows, k, d2_dtype):
    """Output buffers holding a pattern no result has (an unwritten slot shows)."""
    kk = max(k, 1)
    return (dev.alloc((nrows, kk), np.int32).fill_bytes(0x55), dev.alloc((nrows, kk), d2_dtype).fill_bytes(0x55),
            dev.alloc(max(nrows, 1), np.int32).fill_bytes(0x55))


def _get(bufs, nrows, k):
    idx, d2, cnt = (b.numpy() for b in bufs)
    return idx[:, :k], d2[:, :k], cnt[:nrows]


def topk_rows(dev, d_rows, ld, d_norms, n, k, row0=0, nrows=None):
    """grid_knn_topk_rows on rows [row0, row0 + nrows) of an uploaded Gram."""
    from grid_amd._abi import call
    nrows = n - row0 if nrows is None else nrows
    bufs = _outs(dev, nrows, k, np.int64)
    call("grid_knn_topk_rows", dev.ctx, d_rows.ptr + row0 * ld * 8, ld, d_norms.ptr, n, k, row0, nrows,
         *(b.ptr for b in bufs))
    return _get(bufs, nrows, k)


def topk_d2(dev, d_rows, ld, n, k, row0=0, nrows=None, key_scale=1.0):
    from grid_amd._abi import call
    nrows = n - row0 if nrows is None else nrows
    bufs = _outs(dev, nrows, k, np.float64)
    call("grid_knn_topk_d2", dev.ctx, d_rows.ptr + row0 * ld * 8, ld, key_scale, n, k, row0, nrows,
         *(b.ptr for b in bufs))
    return _get(bufs, nrows, k)


def same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("idx", "d2", "cnt")):
        if not np.array_equal(g, e):
            bad = np.nonzero((g != e).reshape(len(g), -1).any(axis=1))[0]
            r = int(bad[0])
            raise AssertionError(f"{what} {name}: {len(bad)} of {len(g)} rows differ, first row {r}:\n"
                                 f"got {g[r].tolist()}\nexp {e[r].tolist()}")


# ---- grid_knn_topk_rows ----
@pytest.mark.parametrize("name", sorted(tc.INT_CASES))
def test_topk_rows_every_case_every_k_range(dev, name):
    """k + 1 = 15, 16, 17 and 31, 32, 33: both edges of k_topk_small<16> and
    <32>; beyond, k_topk_radix with its bitonic stage at 64, 256 and 512 keys,
    on both sides of the powers of two."""
    gram, norms, D, order = case(name, N_CASE)
    dg, dn = dev.upload(gram), dev.upload(norms)
    for k in KS:
        same(topk_rows(dev, dg, gram.shape[0], dn, N_CASE, k), tc.ref_topk(D, k, order=order), f"{name} k={k}")


@pytest.mark.parametrize("n", NS)
def test_topk_rows_row_lengths(dev, n):
    """Rows on both sides of k_topk_small's 4x-unrolled loop (n >= 769), off the
    256 stride, and of one or two keys; every kernel at each length."""
    for name in ("ties", "wide"):
        gram, norms, D, order = case(name, n)
        dg, dn = dev.upload(gram), dev.upload(norms)
        for k in (6, 15, 17, 31, 33, 300):
            same(topk_rows(dev, dg, gram.shape[0], dn, n, k), tc.ref_topk(D, k, order=order), f"{name} n={n} k={k}")


@pytest.mark.parametrize("n,k", [(20, 25), (40, 45), (12, 30)])
@pytest.mark.parametrize("name", ["dups", "paired"])
def test_topk_rows_k_at_least_n(dev, name, n, k):
    """k >= n clamps k + 1 to n: the 32-key kernel at n = 20, radix at n = 40,
    the 16-key kernel at n = 12; every row lists all others, self dropped."""
    gram, norms, D, order = case(name, n)
    got = topk_rows(dev, dev.upload(gram), gram.shape[0], dev.upload(norms), n, k)
    same(got, tc.ref_topk(D, k, order=order))
    assert (got[2] == n - 1).all()


@pytest.mark.parametrize("k", [9, 20, 70])
def test_topk_rows_band_and_wide_stride(dev, k):
    """row0 > 0 with nrows < n, on a Gram whose row stride exceeds np (the extra
    cells hold Gram values that would win)."""
    n = 300
    gram, norms, D, _ = case("dups", n)
    np_ = gram.shape[0]
    ld = np_ + 24
    wide = np.empty((np_, ld), dtype=np.int64)
    wide[:, :np_] = gram
    wide[:, np_:] = gram[:, n:n + 1]
    dg, dn = dev.upload(wide), dev.upload(norms)
    rows = np.arange(37, 37 + 64)
    same(topk_rows(dev, dg, ld, dn, n, k, 37, 64), tc.ref_topk(D, k, rows=rows))
    same(topk_rows(dev, dg, ld, dn, n, k), tc.ref_topk(D, k))


def test_topk_rows_k0(dev):
    gram, norms, _, _ = case("ties", 33)
    _, _, cnt = topk_rows(dev, dev.upload(gram), gram.shape[0], dev.upload(norms), 33, 0)
    assert (cnt == 0).all()


def _band_case(n, row0, nrows, seed):
    """Distances of rows [row0, row0 + nrows) only (the other rows of D stay
    zero and are never read): half the rows over a range narrow enough for ties
    at every rank, half over the key width.  (gram band [nrows][np], norms, D)."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n), dtype=np.int64)
    band = 2 * rng.integers(0, n // 3, size=(nrows, n))
    band[1::2] = 2 * rng.integers(0, 2 ** 43 - 1, size=band[1::2].shape)
    D[row0:row0 + nrows] = band
    g = np.zeros((nrows, tc.pad_to(n, 64)), dtype=np.int64)          # pad columns: d2 = 0 would win
    g[:, :n] = -(band // 2)
    return g, np.zeros(n, dtype=np.int64), D


def test_topk_rows_last_admitted_k(dev):
    """k + 1 = 4096 fills the radix kernel's selection buffer: n = 4200, a
    64-row band; k = 4096 is refused."""
    from grid_amd._abi import GridNativeError, call
    n, k, row0, nrows = 4200, 4095, 4100, 64
    g, norms, D = _band_case(n, row0, nrows, 6)
    dg, dn = dev.upload(g), dev.upload(norms)            # the band's rows only: dg is row row0
    bufs = _outs(dev, nrows, k, np.int64)
    call("grid_knn_topk_rows", dev.ctx, dg.ptr, g.shape[1], dn.ptr, n, k, row0, nrows, *(b.ptr for b in bufs))
    same(_get(bufs, nrows, k), tc.ref_topk(D, k, rows=np.arange(row0, row0 + nrows)))
    with pytest.raises(GridNativeError):
        call("grid_knn_topk_rows", dev.ctx, dg.ptr, g.shape[1], dn.ptr, n, k + 1, row0, nrows,
             *(b.ptr for b in bufs))


# ---- grid_knn_topk_d2 ----
@pytest.mark.parametrize("name", sorted(tc.INT_CASES))
def test_topk_d2_integer_rows(dev, name):
    """Integer distances below 2^44 as fp64 rows at key_scale = 1: the lists of
    the integer kernels, the distances as fp64.  Pad columns hold 0 (would win)."""
    _, _, D, order = case(name, N_CASE)
    ld = tc.pad_to(N_CASE, 64)
    rows = np.zeros((N_CASE, ld))
    rows[:, :N_CASE] = D
    dr = dev.upload(rows)
    for k in KS:
        idx, d2, cnt = tc.ref_topk(D, k, order=order)
        same(topk_d2(dev, dr, ld, N_CASE, k), (idx, d2.astype(np.float64), cnt), f"{name} k={k}")
    rb = np.arange(100, 164)
    idx, d2, cnt = tc.ref_topk(D, 40, rows=rb)
    same(topk_d2(dev, dr, ld, N_CASE, 40, 100, 64), (idx, d2.astype(np.float64), cnt), f"{name} band")


def test_topk_d2_rejects_k_4096(dev):
    from grid_amd._abi import GridNativeError
    dr = dev.upload(np.zeros((64, 64)))
    with pytest.raises(GridNativeError):
        topk_d2(dev, dr, 64, 50, 4096)


def _fp64_input(which):
    if which == "normal":                  # tests/test_gpu_general_knn.py's input
        return np.random.default_rng(1).normal(size=(90, 200)) * 1.7
    if which == "tiny":                    # distances ~1e-11 under a bound of 4 m^2 r + 1
        return np.random.default_rng(1).normal(size=(90, 5)) * 1e-6
    rng = np.random.default_rng(2)         # near-copies: distances ~1e-13 beside ones of ~80
    base = rng.normal(size=40)
    return np.concatenate([base[None, :] + 1e-7 * rng.normal(size=(64, 40)), rng.normal(size=(30, 40))])


@pytest.mark.parametrize("k", [9, 20, 40])
@pytest.mark.parametrize("which", ["normal", "tiny", "near_copies"])
def test_knn_values_fp64_order(dev, which, k):
    """engine.knn_values on values that are not hundredths: neighbours ordered
    by (d2 as fp64, j) however small the distances are beside the largest, the
    distances bit for bit."""
    from grid_amd import engine
    x = _fp64_input(which)
    n = len(x)
    idx, d2, cnt = engine.knn_values(dev, x, k)
    exp = steps.knn_direct_f64(x, k)
    wrong = [i for i in range(n) if cnt[i] != len(exp[i]) or idx[i, : cnt[i]].tolist() != [j for j, _ in exp[i]]]
    assert not wrong, f"{len(wrong)} of {n} rows with wrong neighbours, first {wrong[0]}"
    for i in range(n):
        assert d2[i, : cnt[i]].tolist() == [s for _, s in exp[i]], i


def test_topk_d2_close_doubles(dev):
    """Rows of doubles that agree in their leading 44 and more bits, exact
    ties among them: order (d2, j), under any key_scale."""
    rng = np.random.default_rng(8)
    n, ld = 300, 320
    D = 1.0 + rng.integers(0, 40, size=(n, n)) * 2.0 ** -52          # 40 adjacent doubles: ties everywhere
    D[::3] = rng.integers(0, 50, size=(len(D[::3]), n)) * 5e-324     # subnormals
    D[1::7] *= 2.0 ** 900
    rows = np.zeros((n, ld))
    rows[:, :n] = D
    dr = dev.upload(rows)
    order = tc.row_orders(D)
    for k in (9, 20, 40, 299):
        for scale in (1.0, 2.0 ** 30):
            same(topk_d2(dev, dr, ld, n, k, key_scale=scale), tc.ref_topk(D, k, order=order), f"k={k} scale={scale}")


# ---- segments ----
def _upload_segments(dev, gram, norms, n, W, B):
    return [dict(s, d=dev.upload(s["seg"])) for s in tc.segments(gram, norms, n, W, B)]


def run_segments(dev, segs, d_norms, n, W, B, k):
    """grid_knn_seg_topk per block into rowc[2W][B][K1] / colc[2W][2WB][K1],
    then one grid_knn_seg_merge, as Steps47._seg_candidates does."""
    from grid_amd._abi import call
    npw = 2 * W * B
    rowc = dev.alloc((2 * W, B, tc.K1), np.uint64).fill_bytes(0x55)
    colc = dev.alloc((2 * W, npw, tc.K1), np.uint64).fill_bytes(0x55)
    for b, s in enumerate(segs):
        call("grid_knn_seg_topk", dev.ctx, s["d"].ptr, s["ld"], s["nrows"], s["ncols"], d_norms.ptr, n, k, s["r0"],
             s["c0"], rowc.ptr + b * B * tc.K1 * 8, colc.ptr + b * npw * tc.K1 * 8)
    bufs = _outs(dev, n, k, np.int64)
    call("grid_knn_seg_merge", dev.ctx, rowc.ptr, colc.ptr, npw, B, n, k, *(b.ptr for b in bufs))
    return _get(bufs, n, k)


@pytest.mark.parametrize("name", ["ties", "dups"])
@pytest.mark.parametrize("W,B,n", [(1, 64, 100), (2, 64, 200), (3, 64, 300), (8, 64, 1000), (15, 64, 1900),
                                   (16, 64, 2040), (20, 32, 1270)])
def test_segments_equal_full_rows(dev, name, W, B, n):
    """The sharded chain's candidate lists and merge against ref_topk and the
    row kernel on the same Gram.  W = 15: k_seg_merge_w with every register of
    its 8 keys per lane in use; W = 16 and 20 (32 and 40 row blocks): the
    thread-per-row k_seg_merge.  The last sample block is partial; at W = 3
    a block is padding only.  A pair of one diagonal block is a candidate
    twice (row and column list) and must be listed once."""
    gram, norms, D, order = case(name, n)
    dn = dev.upload(norms)
    segs = _upload_segments(dev, gram, norms, n, W, B)
    dg = dev.upload(gram)
    for k in (1, 6, 15):
        exp = tc.ref_topk(D, k, order=order)
        same(run_segments(dev, segs, dn, n, W, B, k), exp, f"segments k={k}")
        same(topk_rows(dev, dg, gram.shape[0], dn, n, k), exp, f"rows k={k}")


def test_segments_reject_k16(dev):
    from grid_amd._abi import GridNativeError, call
    gram, norms, _, _ = case("ties", 100)
    segs = _upload_segments(dev, gram, norms, 100, 1, 64)
    with pytest.raises(GridNativeError):
        run_segments(dev, segs[:1], dev.upload(norms), 100, 1, 64, 16)
    rowc = dev.alloc((2, 64, tc.K1), np.uint64).fill_bytes(0xFF)
    colc = dev.alloc((2, 128, tc.K1), np.uint64).fill_bytes(0xFF)
    bufs = _outs(dev, 100, 16, np.int64)
    with pytest.raises(GridNativeError):
        call("grid_knn_seg_merge", dev.ctx, rowc.ptr, colc.ptr, 128, 64, 100, 16, *(b.ptr for b in bufs))
