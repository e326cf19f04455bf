"""The hand-built DEFLATE cases (tests/inflate_cases.py) on the CPU: zlib's
verdict on every case must be the one the case was built for (this guards the
writer: a writer bug cannot turn the suite into "both reject"), the families
must hold what they claim, and the host build of the decoding core
(grid_amd/csrc/inflate_core.hpp; tests/native/inflate_core_host.cpp) at
literal/length fast tables of 2^8 and 2^10 entries must agree with zlib on
every case, with equal text where the stream is accepted.  The device's own
loop runs the same cases in tests/test_gpu_inflate.py."""
import gzip
import os
import re
import shutil

import pytest

from tests import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_DATA, E_SPACE = 1, 3


def zlib_verdict(blob):
    try:
        return gzip.decompress(blob)
    except Exception:
        return None


@pytest.fixture(scope="module")
def texts():
    return {name: zlib_verdict(blob) for name, blob, _ in ic.CASES}


@pytest.fixture(scope="module", params=[8, 10])
def core(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not present")
    return ic.host_core(request.param, tmp_path_factory.mktemp(f"icases{request.param}"))


def test_constants_are_the_kernels():
    """The cases aim at the kernel's constants: they must be today's."""
    hip = open(os.path.join(ROOT, "grid_amd", "csrc", "inflate.hip")).read()
    core = open(os.path.join(ROOT, "grid_amd", "csrc", "inflate_core.hpp")).read()
    m = re.search(r"constexpr int RING = (\d+), RMASK = RING - 1, FLUSH = (\d+), NEAR = RING - 258;", hip)
    assert m and (int(m.group(1)), int(m.group(2))) == (ic.RING, ic.FLUSH)
    assert f"const int room = cap - {ic.ROOM};" in hip
    assert f"if (ip + {ic.TAIL} > nin) break;" in hip
    assert re.search(r"#define GRID_INFLATE_LFAST %d\b" % ic.LFAST, core)
    assert re.search(r"#define GRID_INFLATE_DFAST %d\b" % ic.DFAST, core)


@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_zlib_verdict_is_the_expected_one(texts, fam):
    n = 0
    for name, blob, expect in ic.CASES:
        if ic.family(name) != fam:
            continue
        n += 1
        t = texts[name]
        assert ("ok" if t is not None else "reject") == expect, name
        if t is not None:
            assert len(t) == ic.SIZE[name], name
    assert n


def test_families_hold_what_they_claim(texts):
    assert len(ic.FAMILIES) == 11
    by = {f: [e for n, _, e in ic.CASES if ic.family(n) == f] for f in ic.FAMILIES}
    both = ("f04_mstart", "f06_illegal", "f07_header", "f08_stored", "f11_crc")
    for f, es in by.items():
        assert "ok" in es, f
        assert ("reject" in es) == (f in both), f
    # family 1: every overlapping pair and the two no-division distances, on >= 16 streams
    want = {(d, ln) for ln in range(3, 259) for d in range(1, ln + 2)}
    assert ic.overlap_pairs() == want
    assert len(ic.F1_TOKENS) >= 16
    # the incomplete sets are there, as rejects; flipped CRCs are otherwise sound
    expect = {n: e for n, _, e in ic.CASES}
    assert all(expect[n] == "reject" for n in ic.INCOMPLETE)
    for name in ic.CRC_FLIPPED:
        assert expect[name] == "reject" and texts[name[: -len("_crcflip")]] is not None
    # family 4 has its later-member files
    assert sum(ic.MEMBERS[n] == 2 and ic.family(n) == "f04_mstart" for n in ic.SIZE) >= 8


@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_core_agrees_with_zlib(core, texts, fam):
    """Status zero and zlib's text where zlib accepts, nonzero where it
    rejects, at every capacity of the case; E_SPACE one byte short."""
    for name, blob, expect in ic.CASES:
        if ic.family(name) != fam:
            continue
        for extra in ic.CAP_EXTRA[name]:
            rc, got, _ = ic.host_gunzip(core, blob, ic.SIZE[name] + extra)
            if extra < 0:
                assert rc == E_SPACE, (name, extra, rc)
            elif expect == "ok":
                assert rc == 0, (name, extra, rc)
                assert got == texts[name], (name, extra)
            else:
                assert rc != 0, (name, extra)
