"""Region coverage without a GPU: the host restatement (grid_amd/utils/
mosdepth.py) against what the reference's compute_region_coverage returned or
raised on the g7_cover fixture (tests/golden/make_golden_cover.py), the case
builder's own claims (tests/cover_cases.py: where its lines sit, the exact
rounding ties, the order-sensitive sum), the files the step writes, and the
pipeline gate."""
import gzip
import json
import os

import pytest
import yaml

from grid_amd.utils import mosdepth as md
from tests import cover_cases as cc

G7 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_cover")


@pytest.fixture(scope="module")
def expected():
    return json.load(open(os.path.join(G7, "expected.json")))


def _cell(v):
    return f"Error:{type(v).__name__}" if isinstance(v, Exception) else v


def _fixture_files():
    return [(d, f.split(".")[0], os.path.join(G7, d, f)) for d in ("edge", "handover", "main")
            for f in sorted(os.listdir(os.path.join(G7, d)))]


def test_fixture_loci_are_the_builders():
    from grid_amd.utils.hi_inference import read_loci_file
    loci = read_loci_file(os.path.join(G7, "loci.txt"))
    assert [(lc["chrom"], lc["start"], lc["end"]) for lc in loci] == cc.LOCI and len(loci) == 70


def test_fixture_files_are_the_builders_text():
    for cohort, c in cc.cases().items():
        for s, text in c["texts"].items():
            raw = open(os.path.join(G7, cohort, f"{s}.regions.bed.gz"), "rb").read()
            assert gzip.decompress(raw) == text, (cohort, s)
            assert raw == c["pack"][s](text), (cohort, s)


def test_restatement_equals_the_reference_on_every_cell(expected):
    """All loci in one walk (region_coverages), Error cells with the class the
    reference raised."""
    n = 0
    for cohort, sample, path in _fixture_files():
        got = [_cell(v) for v in md.region_coverages(path, cc.LOCI)]
        assert got == expected[cohort][sample], (cohort, sample)
        n += len(got)
    assert n == 18 * 70


def test_single_region_entry_has_the_references_semantics(expected):
    """compute_region_coverage(regions_file, chrom, start, end): one region per
    call, raising what the reference raises."""
    for cohort, sample in (("main", "M0"), ("main", "M2"), ("main", "M4"), ("handover", "H4"), ("handover", "H6"),
                           ("handover", "H2"), ("edge", "Z0"), ("edge", "Z1")):
        path = os.path.join(G7, cohort, f"{sample}.regions.bed.gz")
        for i in (0, 1, 3, 9, 13, 14, 15, 16, 40):
            exp = expected[cohort][sample][i]
            try:
                got = md.compute_region_coverage(path, *cc.LOCI[i])
            except Exception as e:
                got = _cell(e)
            assert got == exp, (cohort, sample, i)


def test_prefixes_of_the_table_give_the_same_cells(expected):
    path = os.path.join(G7, "main", "M0.regions.bed.gz")
    for n in cc.N_LOCI_CASES:
        assert md.region_coverages(path, cc.LOCI[:n]) == expected["main"]["M0"][:n]


# ---- the builder's own claims ----
def test_geometry_lines_sit_where_the_builder_says():
    t = cc.cases()["main"]["texts"]
    m0 = t["M0"]
    for s in t:
        assert s == "M4" or 2 * cc.CH < len(t[s]) <= 3 * cc.CH, s         # three chunks
    a = m0.index(cc.G_LAST_SEG.encode())
    assert cc.CH - cc.SEG <= a < cc.CH and a + len(cc.G_LAST_SEG) <= cc.CH
    b = m0.index(cc.G_CHUNK_EDGE.encode())
    assert b < cc.CH < b + len(cc.G_CHUNK_EDGE) - 1
    c = m0.index(cc.G_SEG_EDGE.encode())
    assert c // cc.SEG != (c + len(cc.G_SEG_EDGE) - 2) // cc.SEG and c % cc.SEG == cc.SEG - 9
    for x in (a, b, c):
        assert x in cc.line_starts(m0)
    # locus 9's lines lie in chunks 0 and 1
    starts = [p for p, ln in zip(cc.line_starts(m0), cc.split_lines(m0)) if ln.startswith(b"chr1\t")]
    assert min(starts) < cc.CH < max(starts) and len(starts) == cc.NBIN1
    assert t["M1"].endswith(cc.G_LAST_LINE.encode()) and not t["M1"].endswith(b"\n")
    assert t["M4"] == b""
    lines2 = [ln for ln in cc.split_lines(t["M2"]) if ln.startswith(b"chr1\t")]
    keys2 = [int(ln.split(b"\t")[1]) for ln in lines2]
    assert keys2 != sorted(keys2) and len(keys2) == len(set(keys2)) + 1
    assert cc.bgzf(m0)[12:14] == b"BC" and cc.plain_gzip(t["M5"])[3] == 0    # no extra field: one plain member


def test_rounding_ties_are_exact_halves():
    """Two 1-bp overlaps: 100 * (region_cov / 2) is exactly k + 0.5 in fp64, so
    only round-half-to-even gives 12 and 38."""
    path = os.path.join(G7, "main", "M0.regions.bed.gz")
    cov, bp, err = md.region_sums(path, cc.TIE_LOCI)
    assert err == [None, None] and bp == [2, 2]
    assert [100 * (c / b) for c, b in zip(cov, bp)] == [12.5, 37.5]
    assert [md.coverage_value(c, b) for c, b in zip(cov, bp)] == cc.TIE_VALUES == [12, 38]


def test_order_sensitive_locus_is_order_sensitive():
    terms = cc.order_terms()
    assert cc._sum(terms).hex() != cc._sum(terms[::-1]).hex()
    loc = [cc.order_locus()]
    fwd = md.region_sums(os.path.join(G7, "main", "M0.regions.bed.gz"), loc)
    rev = md.region_sums(os.path.join(G7, "main", "M3.regions.bed.gz"), loc)
    assert fwd[0][0].hex() == cc._sum(terms).hex() and rev[0][0].hex() == cc._sum(terms[::-1]).hex()
    assert fwd[0][0].hex() != rev[0][0].hex() and fwd[1] == rev[1]


def test_handover_lines_are_outside_the_device_grammar():
    from tests.mdparse_cases import MAXLINE, parse_line
    for name, (_, line) in cc.HANDOVER_KINDS.items():
        body = line[:-1]
        assert parse_line(body) is None or len(body) > MAXLINE, name
    for s, text in cc.cases()["handover"]["texts"].items():
        bad = [ln for ln in cc.split_lines(text) if parse_line(ln) is None or len(ln) > MAXLINE]
        assert len(bad) == (1 if s in cc.HANDOVER_KINDS else 0), s
    for text in cc.cases()["main"]["texts"].values():
        assert all(parse_line(ln) is not None and len(ln) <= MAXLINE for ln in cc.split_lines(text))


# ---- the step's files and the gate ----
class _Console:
    def __init__(self):
        self.lines = []

    def print(self, msg, style=None):
        self.lines.append(str(msg))


def _config(tmp_path, cohort, coverage=None, **mosdepth):
    samples = list(cc.cases()[cohort]["texts"])
    (tmp_path / "samples.txt").write_text("\n".join(samples + ["NOFILE"]) + "\n")
    cfg = {"samples_file": str(tmp_path / "samples.txt"), "output_dir": str(tmp_path / "out"),
           "output_file_type": "tsv", "chrom": "chr1", "start_bp": cc.LOCI[0][1], "end_bp": cc.LOCI[0][2],
           "index": {"run": None}, "count_reads": {"run": False, "output_file_prefix": "counts"},
           "mosdepth": dict({"run": False, "work_dir": os.path.join(G7, cohort), "output_file_prefix": "cov",
                             "normalize": {"run": False}, "neighbors": {"run": False}}, **mosdepth),
           "compute_diploid_genotypes": {"run": False}, "compute_haploid_genotypes": {"run": False}}
    if coverage is not None:
        cfg["mosdepth"]["coverage"] = coverage
    return cfg


def test_single_region_file_has_the_references_header_and_rows(tmp_path, expected):
    cfg = _config(tmp_path, "handover", coverage={"run": True, "device": False})
    con = _Console()
    record = md.compute_region_coverages(cfg, con)
    chrom, s, e = cc.LOCI[0]
    exp = expected["handover"]
    rows = [f"{k}\t{exp[k][0]}" for k in cc.cases()["handover"]["texts"] if isinstance(exp[k][0], int)]
    assert len(rows) == 7                                            # H2, H3 (unreadable lines) and H6 (nan) left out
    assert (tmp_path / "out" / "cov.tsv").read_text() == "\n".join([f"Sample\t{chrom}:{s}-{e}"] + rows) + "\n"
    assert set(record.values()) == {"host"} and list(record) == list(cc.cases()["handover"]["texts"])
    log = "\n".join(con.lines)
    assert "NOFILE" in log and all(f"{k} failed" in log for k in ("H2", "H3", "H6")) and "H4 failed" not in log


def test_loci_mode_writes_one_file_per_region(tmp_path, expected):
    from grid_amd.utils.compute_dipcn import _read_counts
    (tmp_path / "loci.txt").write_text(cc.loci_file_text())
    cfg = _config(tmp_path, "main", coverage={"run": True, "device": False, "loci_file": str(tmp_path / "loci.txt")})
    md.compute_region_coverages(cfg, _Console())
    out = sorted(os.listdir(tmp_path / "out"))
    assert len(out) == 70
    for i, (chrom, s, e) in enumerate(cc.LOCI):
        p = tmp_path / "out" / f"cov.{chrom}_{s}_{e}_L{i:02d}.tsv"
        lines = p.read_text().splitlines()
        assert lines[0] == f"Sample\t{chrom}:{s}-{e}"
        assert lines[1:] == [f"{k}\t{expected['main'][k][i]}" for k in cc.cases()["main"]["texts"]]
        assert _read_counts(p) == {k: expected["main"][k][i] for k in cc.cases()["main"]["texts"]}   # step 6 reads it
    # a template of the caller's own
    cfg["mosdepth"]["coverage"]["loci_output"] = "{output_dir}/by_index/{index}.{type}"
    md.compute_region_coverages(cfg, _Console())
    assert sorted(os.listdir(tmp_path / "out" / "by_index")) == sorted(f"{i}.tsv" for i in range(70))


def _pipeline(tmp_path, cfg):
    from grid_amd import pipeline
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    con = _Console()
    pipeline._run(con, str(p))
    return con.lines


def test_gate_absent_key_changes_nothing(tmp_path):
    assert _pipeline(tmp_path, _config(tmp_path, "main")) == []
    assert not (tmp_path / "out").exists()
    lines = _pipeline(tmp_path, _config(tmp_path, "main", run=True))
    assert lines == ["mosdepth (step 3) is not part of grid_amd (steps 4-7 only); using existing outputs"]
    assert not (tmp_path / "out").exists()
    assert _pipeline(tmp_path, _config(tmp_path, "main", coverage={"run": False, "device": False})) == []
    assert not (tmp_path / "out").exists()


def test_gate_runs_the_step(tmp_path):
    lines = _pipeline(tmp_path, _config(tmp_path, "main", run=True, coverage={"run": True, "device": False}))
    assert lines[0].startswith("mosdepth (step 3) is not part of grid_amd")
    assert (tmp_path / "out" / "cov.tsv").read_text().count("\n") == 7
