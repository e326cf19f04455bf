"""The device reader of the normalised matrix file, without a GPU: the host
restatement of its kernels (grid_ntext_parse_host runs the same
ntext_core.hpp count / scan / parse serially) against the host reader
(_abi.read_normalized_gz) on hand-framed files; every malformed text sets
its flag; the member index; the batch planner."""
import numpy as np
import pytest

from grid_amd import _abi
from grid_amd.utils import ntext_device
from tests import ntext_cases as nc

P = _abi.NT_PREFIX_BYTES


def host_restatement(path, texts, n, r):
    """What the device path computes, on the host: zq, ids, scales; the flags."""
    zq = np.full((n, r + 3), 12345, np.int32)          # a row stride wider than r
    rowoff = np.full(n, -1, np.int64)
    flags, rows, pre = 0, [], np.zeros((n, P), np.uint8)
    for text, first in texts:
        fl, nr = _abi.ntext_parse_host(text, first, n, r, zq, rowoff)
        flags |= fl
        rows.append(nr)
        for row in range(first, min(n, first + nr)):       # grid_ntext_prefix
            b = np.frombuffer(text[rowoff[row]:rowoff[row] + P], np.uint8)
            pre[row, :len(b)] = b
    ids, scales, rfl = _abi.ntext_rows(pre)
    return zq, ids, scales, flags | int(np.bitwise_or.reduce(rfl)) if n else flags, rows


@pytest.mark.parametrize("n,r,rows_per_member,id_len", [
    (9, 37, [4, 5], None),
    (12, 1, [12], None),                  # R = 1
    (5, 40, [2, 3], 1),                   # 1-byte IDs
    (4, 40, [1, 3], 200),                 # 200-byte IDs
    (7, 5003, [3, 4], None),              # rows longer than a chunk: cells straddle segments and chunks
])
def test_host_restatement_equals_host_reader(tmp_path, n, r, rows_per_member, id_len):
    data, texts, exp = nc.case(n, r, seed=n * 100 + r, rows_per_member=rows_per_member, id_len=id_len)
    f = tmp_path / "m.tsv.gz"
    f.write_bytes(data)
    ids, scales, means, ratios, zq = _abi.read_normalized_gz(str(f))
    assert np.array_equal(zq, exp)                     # the cases' own expectation
    if r > 100:
        assert any(len(t) > 2 * 16384 for t, _ in texts)
    got_zq, got_ids, got_scales, flags, rows = host_restatement(f, texts, n, r)
    assert flags == 0
    assert rows == rows_per_member
    assert got_ids == ids
    assert got_scales.tobytes() == scales.tobytes()    # bit-identical, NaN included
    assert np.array_equal(got_zq[:, :r], zq)
    assert np.all(got_zq[:, r:] == 12345)
    ix = _abi.ntext_index(str(f))
    assert (ix["n"], ix["r"]) == (n, r)
    assert ix["first_row"].tolist() == [fr for _, fr in texts]
    assert ix["isize"].tolist() == [len(t) for t, _ in texts]
    assert int(ix["off"][0] + ix["len"].sum()) == len(data)
    assert ix["means"].tobytes() == means.tobytes() and ix["ratios"].tobytes() == ratios.tobytes()
    table = _abi.ntext_index(str(f), header=False)        # the member table alone (the cost rule's input)
    assert (table["n"], table["r"]) == (-1, -1)
    assert all(np.array_equal(table[k], ix[k]) for k in ("off", "len", "first_row", "isize"))


def test_every_chunk_and_segment_offset():
    """A 12-byte cell (an int32 extreme) at every offset across a segment and
    a chunk boundary: the ID's length slides the row through them."""
    r = 2800                                            # ~ 16.8 KB per row
    toks = [["-21474836.47", "21474836.47", "NA", "-0.00", "7.05"][c % 5] for c in range(r)]
    exp = np.array([[-nc.IMAX, nc.IMAX, nc.MISSING, 0, 705][c % 5] for c in range(r)], np.int32)
    for pad in range(0, 80, 3):
        text = b"".join(nc.row_text("I" * (1 + pad), "1.00", toks) for _ in range(3))
        zq, rowoff = np.zeros((3, r), np.int32), np.full(3, -1, np.int64)
        fl, nr = _abi.ntext_parse_host(text, 0, 3, r, zq, rowoff)
        assert (fl, nr) == (0, 3)
        assert np.array_equal(zq, np.tile(exp, (3, 1)))
        assert rowoff.tolist() == [k * len(text) // 3 for k in range(3)]


def _flags(text, n=3, r=3, first=0):
    zq, rowoff = np.zeros((n, r), np.int32), np.full(n, -1, np.int64)
    return _abi.ntext_parse_host(text, first, n, r, zq, rowoff)[0]


GOOD = b"a\t1.00\t1.00\t2.00\t3.00\nb\t1.00\tNA\t-0.00\t21474836.47\n"


@pytest.mark.parametrize("bad,flag", [
    (GOOD.replace(b"2.00", b"3e1"), _abi.NT_BADCELL),
    (GOOD.replace(b"2.00", b"1.234"), _abi.NT_BADCELL),
    (GOOD.replace(b"2.00", b"123456789.00"), _abi.NT_BADCELL),       # nine integer digits
    (GOOD.replace(b"2.00", b"000000002.00"), _abi.NT_BADCELL),       # nine digits the host reader takes
    (GOOD.replace(b"21474836.47", b"21474836.48"), _abi.NT_BADCELL),  # past int32
    (GOOD.replace(b"2.00", b""), _abi.NT_BADCELL),                   # an empty cell
    (GOOD.replace(b"2.00", b".00"), _abi.NT_BADCELL),
    (GOOD.replace(b"2.00", b"+2.00"), _abi.NT_BADCELL),
    (GOOD.replace(b"2.00", b"2.0"), _abi.NT_BADCELL),
    (GOOD.replace(b"NA", b"na"), _abi.NT_BADCELL),
    (GOOD.replace(b"\t2.00", b""), _abi.NT_BADROW),                   # a row one cell short
    (GOOD.replace(b"\t2.00", b"\t2.00\t2.50"), _abi.NT_BADROW),       # a row one cell long
    (GOOD.replace(b"\nb", b"\n\nb"), _abi.NT_BADROW),                 # an empty line
    (b"\t" + GOOD, _abi.NT_LEADWS),
    (b" " + GOOD, _abi.NT_LEADWS),
    (GOOD.replace(b"\nb", b"\n b"), _abi.NT_LEADWS),
    (GOOD.replace(b"\n", b"\r\n"), _abi.NT_CR),
    (GOOD[:-1], _abi.NT_NOEOL),
    (GOOD + GOOD, _abi.NT_ROWRANGE),                                  # four rows, N = 3
])
def test_malformed_text_sets_its_flag(bad, flag):
    assert _flags(GOOD) == 0
    assert _flags(bad) & flag
    # the same defect after a chunk boundary and a segment boundary
    lead = b"".join(nc.row_text(f"r{i}", "1.00", ["1.00"] * 3) for i in range(1400))   # ~ 30 KB
    assert _flags(lead + GOOD, n=1500, first=0) == 0
    assert _flags(lead + bad, n=1402 if flag == _abi.NT_ROWRANGE else 1500) & flag


def test_first_row_outside_n_is_flagged():
    assert _flags(GOOD, n=3, first=2) & _abi.NT_ROWRANGE
    assert _flags(GOOD, n=3, first=-1) & _abi.NT_ROWRANGE


def test_second_tab_beyond_the_prefix_is_flagged():
    pre = np.zeros((3, P), np.uint8)
    rows = [b"id\t30.25\t1.00\n", b"x" * 600 + b"\t1.00\t1.00\n", b"y" * 300 + b"\t" + b"9" * 300 + b".00\t1.00\n"]
    for k, t in enumerate(rows):
        pre[k, :min(P, len(t))] = np.frombuffer(t[:P], np.uint8)
    ids, scales, fl = _abi.ntext_rows(pre)
    assert ids[0] == "id" and scales[0] == 30.25 and fl[0] == 0
    assert fl[1] & _abi.NT_PREFIX and fl[2] & _abi.NT_PREFIX
    bad = np.zeros((2, P), np.uint8)
    for k, t in enumerate([b"id\t3x\t1.00\n", b"id\t\t1.00\n"]):
        bad[k, :len(t)] = np.frombuffer(t, np.uint8)
    assert np.all(_abi.ntext_rows(bad)[2] & _abi.NT_BADSCALE)


def test_index_refuses_a_single_stream_file(tmp_path):
    import gzip
    f = tmp_path / "ref.tsv.gz"
    with gzip.open(f, "wb") as g:
        g.write(nc.header_text(2, np.ones(3), np.ones(3)) + GOOD)
    with pytest.raises(_abi.GridNativeError) as e:
        _abi.ntext_index(str(f))
    assert e.value.code == _abi.GRID_EUNSUPPORTED
    assert len(_abi.read_normalized_gz(str(f))[0]) == 2    # the host reader reads it


def test_batch_planner():
    clen = [1000, 300, 300, 5000, 10, 10, 10]
    tlen = [3000, 900, 900, 900, 40, 7000, 40]
    b = ntext_device.plan_batches(clen, tlen, batch_in=2048, batch_text=4096)
    assert [m for x in b for m in x] == list(range(7))              # order kept, every member once
    al = lambda v: -(-v // 256) * 256
    for x in b:
        if len(x) > 1:
            assert sum(al(clen[m]) for m in x) <= 2048 and sum(al(tlen[m]) for m in x) <= 4096
    assert [3] in b and [5] in b                                    # larger than a bound: alone
    assert b == [[0, 1], [2], [3], [4], [5], [6]]
    assert ntext_device.plan_batches(clen, tlen, batch_in=1 << 20, batch_text=1 << 20) == [list(range(7))]
    assert ntext_device.plan_batches([], []) == []


def test_cost_rule(monkeypatch):
    """Few huge members are serial on the GPU; many small ones are not."""
    monkeypatch.setattr(ntext_device, "AUTO_DEVICE", True)
    monkeypatch.setattr(ntext_device, "WAVE_RATE", 10e6)
    monkeypatch.setattr(ntext_device, "HOST_RATE_PER_THREAD", 125e6)
    assert ntext_device.prefer_device(3202, 13.5e6, 43e9, 16, 256)          # 1.35 s against 21.5 s
    assert not ntext_device.prefer_device(2, 2e9, 4e9, 16, 256)             # 200 s against 2 s
    assert not ntext_device.prefer_device(20000, 13.5e6, 270e9, 1024, 256)  # three rounds of waves
    monkeypatch.setattr(ntext_device, "AUTO_DEVICE", False)
    assert not ntext_device.prefer_device(3202, 13.5e6, 43e9, 16, 256)
