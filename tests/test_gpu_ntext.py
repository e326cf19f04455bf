"""Step 5's read on the device (_abi.read_normalized_gz_dev: grid_gunzip_batch
+ ntext_dev.hip) against the host reader (_abi.read_normalized_gz): ids,
scales, means, ratios and every cell equal, on hand-framed files that choose
the member count, rows per member and deflate block type, on files the device
writer wrote, across batches; every file outside its reach hands over
(DeviceReadUnsupported) and the host path then gives what it always gave;
`grid wgs` step 5 alone on the golden cohort through either reader."""
import gzip
import os
import struct

import numpy as np
import pytest

from tests import ntext_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from grid_amd import _abi
    return _abi.Device(0)


def _same(dev, path, timings=None):
    """The device reader's result (a hand-over raises: no silent fall-back)
    equals the host reader's, everything."""
    from grid_amd import _abi
    ids, sc, mu, ra, zq = _abi.read_normalized_gz(str(path))
    got = _abi.read_normalized_gz_dev(dev, str(path), timings=timings)
    assert isinstance(got[4], _abi.DevBuf) and got[4].shape == zq.shape and got[4].dtype == np.int32
    assert got[0] == ids
    assert got[1].tobytes() == sc.tobytes()            # bit-identical scales, NaN included
    assert got[2].tobytes() == mu.tobytes() and got[3].tobytes() == ra.tobytes()
    assert np.array_equal(got[4].numpy(), zq)
    return zq


@pytest.mark.parametrize("n,r,rows_per_member,level", [
    (7, 5003, [7], 6),                                 # cells straddle segments and chunks, rows straddle chunks
    (79, 300, [1 + k % 3 for k in range(39)] + [1], 6),   # 40 members of 1-3 rows
    (6, 700, [3, 3], 0),                               # stored blocks
    (5, 1, [1, 1, 1, 1, 1], 6),                        # members of a few bytes: fixed Huffman
    (4, 6000, [4], 6),                                 # > 64 KiB of text: several dynamic blocks
], ids=["straddle", "members40", "stored", "fixed", "dynamic"])
def test_hand_framed_files(dev, tmp_path, n, r, rows_per_member, level):
    data, texts, exp = nc.case(n, r, seed=n + r, rows_per_member=rows_per_member, level=level)
    if len(rows_per_member) == 40:
        assert any(len(t) % 16 for t, _ in texts)
    f = tmp_path / "m.tsv.gz"
    f.write_bytes(data)
    assert np.array_equal(_same(dev, f), exp)


def _matrix(n, r, seed, wide):
    rng = np.random.default_rng(seed)
    zq = np.clip(np.rint(rng.normal(0, 120, (n, r))), -2 ** 31 + 2, 2 ** 31 - 1).astype(np.int32)
    if wide:
        zq.flat[rng.integers(0, n * r, 50)] = rng.integers(-2 ** 31 + 2, 2 ** 31 - 1, 50)
        zq.flat[0], zq.flat[-1] = 2 ** 31 - 1, -2 ** 31 + 2
    zq.flat[rng.integers(0, n * r, 30)] = -(2 ** 31)            # NA
    zq.flat[rng.integers(0, n * r, 30)] = -(2 ** 31) + 1        # -0.00
    raw = rng.uniform(5, 90, n)
    raw[0] = 1e300
    mu, ra = rng.uniform(10, 60, r), rng.uniform(0, 9, r)
    mu[0] = np.nan
    return [f"SAMPLE_{i:05d}" for i in range(n)], raw, mu, ra, zq


@pytest.mark.parametrize("n,r,batch,wide", [(33, 3001, 40000, True), (2, 1_500_001, 0, False)],
                         ids=["wide", "one-row-members"])
def test_device_writer_files(dev, tmp_path, n, r, batch, wide):
    """Members as gzwrite.hip codes them (one dynamic block each); a row of
    more than 8 MB of text is a member of its own."""
    from grid_amd import _abi
    ids, raw, mu, ra, zq = _matrix(n, r, seed=n + r, wide=wide)
    f = tmp_path / "d.tsv.gz"
    _abi.write_normalized_gz_dev(dev, str(f), ids, raw, mu, ra, dev.upload(zq), n, r, r, level=1, batch_bytes=batch)
    got = _same(dev, f)
    assert np.array_equal(got, np.where(zq == -(2 ** 31) + 1, 0, zq))
    if r > 10 ** 6:
        assert len(_abi.ntext_index(str(f))["first_row"]) == n


def test_batches_reuse_both_staging_buffers(dev, tmp_path, monkeypatch):
    from grid_amd.utils import ntext_device
    data, texts, exp = nc.case(60, 300, seed=5, rows_per_member=[2] * 30)
    f = tmp_path / "m.tsv.gz"
    f.write_bytes(data)
    monkeypatch.setattr(ntext_device, "BATCH_IN", 12000)
    monkeypatch.setattr(ntext_device, "BATCH_TEXT", 30000)
    tm = {}
    assert np.array_equal(_same(dev, f, timings=tm), exp)
    assert tm["batches"] >= 5 and tm["members"] == 30


def _outcome(path):
    """What the host path of step 5 gives for the file: its values or its error."""
    from grid_amd.utils import find_neighbors as fn
    try:
        ids, scales, zq, ratios = fn._read_normalized_q(str(path))
    except Exception as e:                             # noqa: BLE001 -- whatever it raises is the outcome
        return "error", type(e).__name__
    return ("ok", ids, sorted((k, repr(v)) for k, v in scales.items()), np.asarray(zq).tolist(),
            np.asarray(ratios, np.float64).tobytes())


def _handover_files(tmp_path):
    data, texts, exp = nc.case(6, 40, seed=9, rows_per_member=[2, 2, 2])
    sizes = []
    p = 0
    while p < len(data):
        sizes.append(struct.unpack_from("<Q", data, p + 16)[0])
        p += sizes[-1]
    m2 = sizes[0] + sizes[1]                           # start of the second row member
    out = {}
    out["single-stream"] = gzip.compress(gzip.decompress(data))
    flip = bytearray(data)
    flip[m2 + 32 + (sizes[2] - 40) // 2] ^= 0x55
    out["deflate-byte"] = bytes(flip)
    crc = bytearray(data)
    crc[m2 + sizes[2] - 8] ^= 0x01
    out["crc"] = bytes(crc)
    means, ratios = np.ones(40), np.ones(40)
    ids, sc = [f"S{i}" for i in range(4)], ["1.00"] * 4
    good = [["1.00"] * 40 for _ in range(4)]
    e31 = [list(r) for r in good]
    e31[2][7] = "3e1"
    out["3e1"] = nc.build(ids, sc, e31, [2, 2], means, ratios)[0]
    short = [list(r) for r in good]
    short[1] = short[1][:-1]
    out["short-row"] = nc.build(ids, sc, short, [2, 2], means, ratios)[0]
    head = nc.member(nc.header_text(4, means, ratios), -1)
    a = b"".join(nc.row_text(ids[i], sc[i], good[i]) for i in (0, 1))
    b = b"".join(nc.row_text(ids[i], sc[i], good[i]) for i in (2, 3))
    out["swapped-first-rows"] = head + nc.member(a, 2) + nc.member(b, 0)
    paths = {}
    for k, v in out.items():
        paths[k] = tmp_path / f"{k}.tsv.gz"
        paths[k].write_bytes(v)
    return paths


@pytest.mark.parametrize("kind", ["single-stream", "deflate-byte", "crc", "3e1", "short-row", "swapped-first-rows"])
def test_hand_overs(dev, tmp_path, kind):
    from grid_amd import _abi
    from grid_amd.utils import ntext_device
    f = _handover_files(tmp_path)[kind]
    before = _outcome(f)
    with pytest.raises(ntext_device.DeviceReadUnsupported):
        _abi.read_normalized_gz_dev(dev, str(f))
    assert _outcome(f) == before
    assert before[0] == ("ok" if kind in ("single-stream", "3e1", "swapped-first-rows") else "error")


def test_step5_alone_on_golden(tmp_path, capsys, monkeypatch):
    """`grid wgs` with only step 5 on a file this project wrote: the golden's
    neighbour file through the device reader (no hand-over) and through the
    host reader, by the config key and by the cost rule; afterwards no ingest
    buffer is left cached."""
    from tests.test_gpu_e2e import G, _content, _stage
    from grid_amd.device import get_device
    from grid_amd.utils import handoff, ingest_device, ntext_device
    from grid_amd.utils.find_neighbors import find_neighbors
    from grid_amd.utils.normalize_mosdepth import normalize_mosdepth
    c, _ = _stage("g1b", tmp_path)
    out, nb = c["output_dir"], "neighbors.zMax2.0.tsv.gz"
    exp = _content(os.path.join(G, "g1b", "expected", nb))
    normalize_mosdepth(c, None)
    handoff.clear()
    calls = []
    real = ntext_device.read
    monkeypatch.setattr(ntext_device, "read", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # key true / false; key absent: the rule keeps a file of one small member on
    # the host, and takes the device once the host's rate is made hopeless
    for want, host_rate, ncalls in ((True, None, 1), (False, None, 1), (None, None, 1), (None, 1.0, 2)):
        c["mosdepth"]["neighbors"].pop("device_read", None)
        if want is not None:
            c["mosdepth"]["neighbors"]["device_read"] = want
        if host_rate is not None:
            monkeypatch.setattr(ntext_device, "HOST_RATE_PER_THREAD", host_rate)
        capsys.readouterr()
        find_neighbors(c, None)
        assert "handed over" not in capsys.readouterr().out
        assert _content(os.path.join(out, nb)) == exp
        os.remove(os.path.join(out, nb))
        assert len(calls) == ncalls
        dev = get_device(c)
        assert dev.cached_bytes() == 0 and ingest_device.staging_bytes() == 0
