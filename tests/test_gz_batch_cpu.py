"""The batch layer the device ingest, the region coverage and step 5's read
share (grid_amd/utils/gz_batch.py): the inflater's member-unit table against a
per-member restatement, the host fold of member results, ``align`` -- host
library only -- and one launch of the table through the shared helper on the
GPU.  The chunk table and the staging are tested in test_ingest_cpu.py through
the names ingest_device keeps for them."""
import functools
import gzip

import numpy as np
import pytest

from grid_amd import _abi
from grid_amd.utils import gz_batch as gb
from tests.cover_cases import bgzf

BLOCK = 65280                       # the text of a full BGZF member


@functools.lru_cache(maxsize=None)
def _files():
    """Four BGZF files: the EOF block alone; one data member; exactly one full
    member; three data members, the first two full."""
    rng = np.random.default_rng(17)
    line = lambda k: b"chr1\t%d\t%d\t%d.%02d\n" % (1000 * k, 1000 * k + 1000, rng.integers(0, 90), rng.integers(0, 100))
    body = b"".join(line(k) for k in range(6000))
    assert len(body) > 2 * BLOCK + 1234
    texts = (b"", body[:3000], body[:BLOCK], body[:2 * BLOCK + 1234])
    blobs = tuple(bgzf(t) for t in texts)
    assert len(blobs[0]) == 28 and [gzip.decompress(b) for b in blobs] == list(texts)
    return blobs, texts


@functools.lru_cache(maxsize=None)
def _members():
    mem = [_abi.gz_members(np.frombuffer(b, np.uint8)) for b in _files()[0]]
    assert [len(m[0]) for m in mem] == [1, 2, 2, 4]
    assert mem[0][2].tolist() == [0] and mem[3][2].tolist() == [BLOCK, BLOCK, 1234, 0]
    return mem


def _offsets(base_in=0, base_text=0):
    blobs, texts = _files()
    in_off = base_in + np.concatenate([[0], np.cumsum([gb.align(max(len(b), 1)) for b in blobs])]).astype(np.int64)
    text_off = base_text + np.concatenate([[0], np.cumsum([gb.align(max(len(t), 1)) for t in texts])]).astype(np.int64)
    return in_off, text_off


def _restated(members, in_off, text_off, files):
    """member_units, one member at a time."""
    rows = []
    for k in files:
        starts, lengths, isizes = members[k]
        at = int(text_off[k])
        for j in range(len(starts)):
            rows.append((int(in_off[k]) + int(starts[j]), int(lengths[j]), at, int(isizes[j]), k))
            at += int(isizes[j])
    return [np.array([r[i] for r in rows], np.int64) for i in range(5)]


@pytest.mark.parametrize("base", [(0, 0), (256, 1024), (7 * 256, 3 * 256)])
@pytest.mark.parametrize("files", [[0, 1, 2, 3], [0], [1], [3], [1, 3], [0, 2], [3, 1], []])
def test_member_units_equal_the_per_member_loop(base, files):
    mem = _members()
    in_off, text_off = _offsets(*base)
    got = gb.member_units(mem, in_off, text_off, files)
    exp = _restated(mem, in_off, text_off, files)
    assert len(got) == 5
    for g, e in zip(got, exp):
        assert g.dtype == np.int64 and g.shape == e.shape and np.array_equal(g, e)
    if not files:
        assert all(len(g) == 0 for g in got)


def test_member_units_skip_files_without_a_table():
    """A batch's plain gzip and non-gzip files have no member table (None):
    only ``files`` is looked at, as the host share and the split leave it."""
    mem = list(_members())
    mem[1] = None
    in_off, text_off = _offsets(512, 256)
    got = gb.member_units(mem, in_off, text_off, [0, 2, 3])
    for g, e in zip(got, _restated(mem, in_off, text_off, [0, 2, 3])):
        assert g.dtype == np.int64 and np.array_equal(g, e)


def test_whole_units():
    in_off, in_len = np.array([0, 256, 4096 * 40], np.int64), [100, 4096 * 30 + 5, 7]
    text_off, cap = np.array([0, 512, 1 << 20], np.int64), np.array([900, 1 << 19, 64], np.int64)
    units, mcap = gb.whole_units(in_off, in_len, text_off, cap, [1, 2])
    assert [u.tolist() for u in units] == [[256, 4096 * 40], [4096 * 30 + 5, 7], [512, 1 << 20], [1 << 19, 64]]
    assert all(u.dtype == np.int64 for u in units)
    assert mcap == (4096 * 30 + 5) // 4096 + 16
    assert gb.whole_units(in_off, in_len, text_off, cap, [2])[1] == 16


def test_fold_members():
    E = _abi
    # file 0: a member past its BGZF size is bad data; file 1: clean; file 2: no unit; owner not sorted
    owner = np.array([1, 0, 3, 0, 1, 0, 3], np.int64)
    status = np.array([0, 0, E.GZ_EDATA, E.GZ_ESPACE, 0, 0, E.GZ_EHEADER], np.int32)
    length = np.array([10, 1, 100, 2, 20, 4, 1000], np.int64)
    fst, fln = gb.fold_members(4, owner, status, length)
    assert fst.tolist() == [E.GZ_EDATA, 0, 0, max(E.GZ_EDATA, E.GZ_EHEADER)] and fst.dtype == np.int32
    assert fln.tolist() == [7, 30, 0, 1100] and fln.dtype == np.int64
    assert gb.fold_members(1, np.zeros(3, np.int64), np.array([0, E.GZ_ESPACE, 0], np.int32),
                           np.ones(3, np.int64))[0].tolist() == [E.GZ_EDATA]
    assert gb.fold_members(1, np.zeros(2, np.int64), np.zeros(2, np.int32), np.ones(2, np.int64))[0].tolist() == [0]
    # a result the caller did not read is not folded
    assert gb.fold_members(4, owner, status)[1] is None and gb.fold_members(4, owner, unit_len=length)[0] is None
    assert gb.fold_members(4, owner, unit_len=length)[1].tolist() == [7, 30, 0, 1100]
    none = gb.fold_members(2, np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert none[0].tolist() == [0, 0] and none[1].tolist() == [0, 0]


def test_align():
    vals = [0, 1, 255, 256, 257]
    for x in vals:
        assert gb.align(x) == -(-x // 256) * 256 and isinstance(gb.align(x), int)
        assert gb.align(np.int64(x)) == -(-x // 256) * 256
    a = gb.align(np.array(vals, np.int64))
    assert a.dtype == np.int64 and a.tolist() == [-(-x // 256) * 256 for x in vals]
    assert gb.align(np.array(vals, np.int64), 64).tolist() == [-(-x // 64) * 64 for x in vals]
    assert gb.align(65, 64) == 128


def test_the_old_names_are_the_shared_objects():
    """What device.py, the tools and the tests reach through ingest_device is
    the shared module's, not a copy."""
    from grid_amd.utils import coverage_device, ingest_device, ntext_device
    assert ingest_device._chunks is gb.chunk_table and ingest_device._staging is gb.staging
    assert ingest_device._STAGING is gb._STAGING and ingest_device.CH == gb.CH == 16384
    assert ingest_device.staging_bytes is gb.staging_bytes and ingest_device.release_staging is gb.release_staging
    assert ingest_device.READ_THREADS == coverage_device.READ_THREADS == ntext_device.READ_THREADS == gb.READ_THREADS
    assert coverage_device._gpu_inflate is gb.gpu_inflate


@pytest.mark.gpu
def test_member_units_through_the_launch_helper():
    """The four files at their aligned offsets, every member a unit of
    grid_gunzip_batch (one member record each): each member inflates, the fold
    gives each file's text length, and the text sits at text_off[k]."""
    import torch
    dev = _abi.Device(0)
    dev.set_stream(torch.cuda.current_stream())
    (blobs, texts), mem = _files(), _members()
    in_off, text_off = _offsets(256, 512)
    src = np.zeros(int(in_off[-1]) + 256, np.uint8)
    for k, b in enumerate(blobs):
        src[in_off[k]:in_off[k] + len(b)] = np.frombuffer(b, np.uint8)
    d_in, d_text = dev.upload(src), dev.alloc(int(text_off[-1]) + 256, np.uint8).fill_bytes(0xEE)
    *units, owner = gb.member_units(mem, in_off, text_off, range(len(blobs)))
    # every unit inside both buffers before anything is launched
    assert (units[0] >= 0).all() and (units[0] + units[1] <= src.size).all()
    assert (units[2] >= 0).all() and (units[2] + units[3] <= d_text.nbytes).all()
    _d, _mem, st, ln, _nm = gb.gpu_inflate(dev, d_in, d_text, units, 1)
    dev.sync()
    ust, uln = st.numpy(), ln.numpy()
    assert (ust == 0).all(), ust
    fst, fln = gb.fold_members(len(blobs), owner, ust, uln)
    assert fst.tolist() == [0] * 4 and fln.tolist() == [len(gzip.decompress(b)) for b in blobs]
    out = d_text.numpy()
    for k, t in enumerate(texts):
        assert bytes(out[text_off[k]:text_off[k] + len(t)]) == t, k
