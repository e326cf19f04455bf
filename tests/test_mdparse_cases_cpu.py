"""What the inputs of the device parse tests mean (tests/mdparse_cases.py),
settled without a GPU: ``device_accepts`` (the documented limits of
mosdepth_dev.hip's md_line and MAXLINE) classifies every file as its case
expects; ``ingest()`` on the host equals the line-by-line restatement of the
reference on every case, so the GPU tests' expected matrices are the
reference's; the geometry each case claims -- record offsets at the chunk
seams, residues covered, file lengths -- is computed from the text; and the
cases do what they are there for (a declined line changes the reference's
result the way its table says, a window or mask edge keeps or drops its bin,
the newline count of k_md_count's former word expression is wrong on the
0x0B case)."""
import numpy as np
import pytest

from grid_amd import _abi
from grid_amd.utils import normalize_mosdepth as nm
from tests import mdparse_cases as mc

CASES = {**mc.device_cases(), **mc.handover_cases()}


def _write(tmp_path, case):
    # plain gzip, written here: a file's text is its lines, byte for byte
    import gzip
    d = tmp_path / "md"
    d.mkdir()
    for name, lines in case["files"].items():
        (d / f"{name}.regions.bed.gz").write_bytes(gzip.compress(mc.text_of(lines), 1))
    m = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
    return d, {k: m[k] for k in case["files"]}


def _args(case, d, inds):
    return (inds, d, case["chrom"], case["start"], case["end"], case["excluded"], case["lo"], case["hi"], 2)


def _values(q):
    """The matrix by value: hundredths / 100 with MISSING as NaN, or the fp64 matrix itself."""
    q = np.asarray(q)
    if q.dtype == np.float64:
        return q
    return np.where(q == _abi.MISSING, np.nan, q / 100.0)


def _prefix(case):
    return nm.norm_chrom(case["chrom"]) if case["chrom"] else None


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_accepts_classifies_the_case(name):
    """expect="device": every file is inside the documented limits;
    "hands_over": at least one file is outside (and in the one-bad-line cases
    exactly the file that holds it)."""
    case = CASES[name]
    ok = {s: mc.device_accepts(mc.text_of(lines), _prefix(case)) for s, lines in case["files"].items()}
    if case["expect"] == "device":
        assert all(ok.values()), [s for s in ok if not ok[s]]
    else:
        assert not all(ok.values())
        if "bad" in case:
            assert [s for s in ok if not ok[s]] == [case["bad"]]


def test_device_accepts_limits():
    acc = lambda line, pre=None: mc.device_accepts(line, pre)  # noqa: E731
    assert acc(b"") and acc(b"c\t1\t2\t3") and acc(b"c\t1\t2\t3\n") and not acc(b"c\t1\t2\t3\n\n")
    assert acc(b"x" * 256 + b"\n", "chr1") and not acc(b"x" * 257 + b"\n", "chr1") and not acc(b"x" * 257, "chr1")
    assert acc(b"#\xc3\xa9\n".replace(b"\xc3\xa9", b"e"), "chr1") and not acc(b"#\xc3\xa9\n", "chr1")
    assert acc(b"c\t" + b"9" * 18 + b"\t0\t0") and not acc(b"c\t" + b"9" * 19 + b"\t0\t0")
    assert acc(b"c\t1\t2\t" + b"0" * 15) and not acc(b"c\t1\t2\t" + b"0" * 16)
    assert acc(b"c\t1\t2\t21474836.47") and not acc(b"c\t1\t2\t21474836.48")
    assert mc.parse_line(b"c\t01\t2\t7.5") == (b"c", 1, 2, 750) and mc.parse_line(b"c\t1\t2\t7.") == (b"c", 1, 2, 700)
    assert acc(b"chr1", "chr10") and not acc(b"chr1", "chr1") and acc(b"\n", "chr1") and not acc(b"\n")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_ingest_equals_the_reference(tmp_path, name):
    """ingest() without a device against ingest_py: exact where both give
    int32, by value where the restatement takes its fp64 route."""
    case = CASES[name]
    d, inds = _write(tmp_path, case)
    got, exp = nm.ingest(*_args(case, d, inds)), nm.ingest_py(*_args(case, d, inds))
    assert got[0] == exp[0] and list(got[1]) == list(exp[1])
    if np.asarray(exp[2]).dtype == np.float64:
        assert case.get("by_value") or case["expect"] == "hands_over", "only the named cases take the fp64 route"
        assert np.array_equal(_values(got[2]), _values(exp[2]), equal_nan=True)
    else:
        assert np.asarray(got[2]).dtype == np.int32 and np.array_equal(got[2], exp[2])
    if case["expect"] == "device":
        # the device tests compare with ingest_native: it reads every such case itself
        nat = nm.ingest_native(*_args(case, d, inds))
        assert nat[0] == exp[0] and list(nat[1]) == list(exp[1])
        assert np.array_equal(_values(nat[2]), _values(exp[2]), equal_nan=True)
        assert len(exp[0]) >= 2 and len(exp[1]) >= 2


# ------------------------------------------------------------------ geometry --
@pytest.mark.parametrize("name", ["chunk_sweep", "chunk_sweep_records"])
def test_chunk_sweep_places_a_record_at_every_offset(name):
    case = CASES[name]
    want = {(24, o) for o in range(-27, 3)}
    want |= {(n, o) for n in (64, 65) for o in (-66, -65, -64, -63, -62, -1, 0, 1)}
    want |= {(n, o) for n in (255, 256) for o in (-258, -257, -256, -255, -254, -129, -128, -1, 0, 1)}
    assert set(mc.SWEEP) == want and len(mc.SWEEP) == len(want)
    texts = [mc.text_of(lines) for lines in case["files"].values()]
    assert len(texts) == 3 and len({len(t) for t in texts}) == 1 and len(set(texts)) == 3
    for t in texts:
        assert len(t) <= 1200 * 1024
        starts = set(mc.line_starts(t))
        for b, (n, off) in enumerate(mc.SWEEP, 1):
            at = mc.CH * b + off
            assert at in starts and t.index(b"\n", at) - at == n
            rec = mc.parse_line(t[at:at + n])
            assert rec is not None and (name == "chunk_sweep_records" or t[at:at + 4] == b"chr1")
        lines = mc.split_lines(t)
        assert max(map(len, lines)) == mc.MAXLINE
        if name == "chunk_sweep":
            # the rest is filler: skipped by the prefix test, whatever its grammar
            assert sum(ln.startswith(b"chr1") for ln in lines) == len(mc.SWEEP)
            assert any(mc.parse_line(ln) is None for ln in lines)
        else:
            # every line is a record with a key of its own, names up to ~230 bytes
            recs = [mc.parse_line(ln) for ln in lines]
            assert all(recs) and len({(r[1], r[2]) for r in recs}) == len(recs) > 8000
            assert max(len(r[0]) for r in recs) >= 200 and min(len(r[0]) for r in recs) == 1


def test_segment_sweep_covers_every_residue():
    case = CASES["segment_sweep"]
    for lines in case["files"].values():
        t = mc.text_of(lines)
        assert {len(ln) for ln in mc.split_lines(t)} == set(range(17, 91))
        starts = mc.line_starts(t)
        assert {p % mc.SEG for p in starts} == set(range(mc.SEG))
        assert {i % mc.WORD for i, b in enumerate(t) if b == 10} == set(range(mc.WORD))
        assert len(t) > 3 * mc.CH


def test_file_tails_lengths_and_ends():
    case = CASES["file_tails"]
    text = {s: mc.text_of(lines) for s, lines in case["files"].items()}
    assert all(len(text[s]) == n for s, n in case["lengths"].items()) and 70 <= len(text) <= 80
    tails = case["tail_files"]
    assert len(tails) == 68
    assert {len(text[s]) % 64 for s in tails} == set(range(64)) and {len(text[s]) % 16 for s in tails} == set(range(16))
    # with and without a final newline in turn, inside the first chunk and in the second
    assert [text[s].endswith(b"\n") for s in tails] == [t % 2 == 0 for t in range(68)]
    for nl in (True, False):
        sizes = [len(text[s]) for s in tails if text[s].endswith(b"\n") == nl]
        assert min(sizes) < mc.CH < max(sizes)
    assert {mc.CH, mc.CH + 1, 2 * mc.CH - 1, 2 * mc.CH} <= {len(t) for t in text.values()}
    assert max(len(t) for t in text.values()) == 2 * mc.CH          # the device's reference file holds every key
    for n in (mc.CH, mc.CH + 1, 2 * mc.CH - 1, 2 * mc.CH):
        t = next(t for t in text.values() if len(t) == n)
        last = mc.split_lines(t)[-1]
        assert last.startswith(b"chr1\t") and mc.parse_line(last) and t.endswith(b"\n") == (n % mc.CH == 0)
    t = text[case["record_unterminated"]]
    assert not t.endswith(b"\n") and mc.parse_line(mc.split_lines(t)[-1])
    t = text[case["tiny"]]
    assert len(t) < 16 and mc.parse_line(t) and t.startswith(b"chr1")
    assert not any(ln.startswith(b"chr1") for ln in mc.split_lines(text[case["filler_only"]]))
    t = text[case["leading_newline"]]
    assert t.startswith(b"\nchr1\t")
    assert all(t.startswith(b"chr1\t") for s, t in text.items() if s in tails)     # a first record at byte 0
    keys = {s: {r[1:3] for r in map(mc.parse_line, mc.split_lines(t)) if r and r[0].startswith(b"chr1")}
            for s, t in text.items()}
    big = max(text, key=lambda s: len(text[s]))
    assert all(k <= keys[big] for k in keys.values())


def test_maxline_cases_are_one_byte_over():
    cases = mc.maxline_declines()
    longest = {k: max(map(len, mc.split_lines(mc.text_of(c["files"]["M000"])))) for k, c in cases.items()}
    assert longest == {"record_257": 257, "filler_257": 257, "unterminated_257": 257, "across_chunks_300": 300}
    t = mc.text_of(cases["across_chunks_300"]["files"]["M000"])
    at = t.index(b"#yyy")
    assert at < mc.CH < at + 300 and len(t) > mc.CH + 150
    assert not mc.text_of(cases["unterminated_257"]["files"]["M000"]).endswith(b"\n")
    assert mc.parse_line(mc.split_lines(mc.text_of(cases["record_257"]["files"]["M000"]))[10])


# ------------------------------------------------------- what the cases show --
@pytest.mark.parametrize("name", sorted(mc.grammar_declines()))
def test_declined_line_in_the_reference(tmp_path, name):
    """What the reference does with the bad line -- keeps its record, skips
    it, or drops the whole sample: the result a silent skip on the device
    would change."""
    case = mc.grammar_declines()[name]
    d, inds = _write(tmp_path, case)
    ids, regions, q = nm.ingest_py(*_args(case, d, inds))
    bad, key, does = case["bad"], case["bad_key"], case["reference"]
    other = next(s for s in case["files"] if s != bad)
    assert other in ids
    if does in ("drops", "empties"):
        assert bad not in ids
        return
    assert bad in ids
    v = _values(q)[ids.index(bad)]
    have = key is not None and key in list(regions) and not np.isnan(v[list(regions).index(key)])
    assert have == (does == "keeps")


@pytest.mark.parametrize("name", sorted(mc.window_mask_edges()))
def test_window_and_mask_edges_in_the_reference(tmp_path, name):
    case = mc.window_mask_edges()[name]
    d, inds = _write(tmp_path, case)
    ids, regions, q = nm.ingest_py(*_args(case, d, inds))
    assert len(ids) == 3 and sorted(regions) == sorted(case["kept"])
    assert case["dropped"] and not set(case["dropped"]) & set(regions)


def test_accepted_forms_reach_the_matrix(tmp_path):
    case = mc.grammar_accepts()["forms"]
    d, inds = _write(tmp_path, case)
    ids, regions, q = nm.ingest_py(*_args(case, d, inds))
    col = {r: j for j, r in enumerate(regions)}
    exp = {"7": 700, "7.": 700, "7.5": 750, "7.50": 750, "007.5": 750, "000000000000007.25": 725,
           "21474835.47": 2147483547}
    for j, text in enumerate(mc.ACCEPT_DEPTHS):
        key = (1000 * (j + 1), 1000 * (j + 2))
        if text in exp:
            assert (q[:, col[key]] == exp[text]).all()
        else:
            assert key not in col                    # depth 0: no record
    assert (200000, 201000) in col and (300000, 301000) in col and (400000, 401000) in col
    assert regions[-1] == (10 ** 18 - 2, 10 ** 18 - 1) and len(regions) == 7 + 3 + 7 + 3


def test_vt_after_newline_miscounts_in_the_word_expression():
    """The case does what it is for: on its text the per-word expression
    k_md_count used -- popcount((x - 0x01010101) & ~x & 0x80808080) with
    x = word ^ 0x0A0A0A0A -- counts more newlines than there are (a borrow
    out of a newline's zero byte makes a following 0x0B look like one), in
    the first chunk and in later ones; the exact per-byte mask does not."""
    case = CASES["vt_after_newline"]
    t = mc.text_of(case["files"]["V000"])
    for p in case["pairs"]:
        assert t[p] == 10 and t[p + 1] == 11 and p % 4 < 3 and t[p - 24:p - 20] == b"chr1"
    assert {p // mc.CH for p in case["pairs"]} == set(mc.VT_CHUNKS) and len(mc.VT_CHUNKS) >= 2
    pad = t + b"\0" * (-len(t) % 4)
    w = np.frombuffer(pad, "<u4") ^ np.uint32(0x0A0A0A0A)
    borrow = (w - np.uint32(0x01010101)) & ~w & np.uint32(0x80808080)
    exact = ~(((w & np.uint32(0x7F7F7F7F)) + np.uint32(0x7F7F7F7F)) | w | np.uint32(0x7F7F7F7F))
    pop = lambda a: int(np.unpackbits(a.view(np.uint8)).sum())  # noqa: E731
    assert pop(exact) == t.count(b"\n")
    assert pop(borrow) == t.count(b"\n") + sum(3 if t[p + 1:p + 4] == b"\x0b" * 3 else 2 if t[p + 2] == 11 else 1
                                                for p in case["pairs"])
    n, kept = mc.ref_lines(t, "chr1")
    assert n == t.count(b"\n") and len(kept) > 4 * len(case["pairs"])
