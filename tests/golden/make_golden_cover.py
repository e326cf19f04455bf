#!/usr/bin/env python3
"""Generate tests/golden/g7_cover/: region coverage from mosdepth files, pinned
against the REFERENCE implementation's compute_region_coverage, called once
per (file, locus).

Run where a checkout of the reference is at hand (the tests never need it):

    python tests/golden/make_golden_cover.py REFERENCE_DIR

What it writes (data only, ~150 KB):
  main/{sample}.regions.bed.gz       the two cohorts of tests/cover_cases.py
  handover/{sample}.regions.bed.gz   (what every file and locus is for: there)
  edge/Z0.regions.bed.gz             a file of zero bytes (gzip.open reads no line)
  edge/Z1.regions.bed.gz             a truncated gzip file (the reference raises)
  loci.txt                           the 70 loci (CHR, BP_START, BP_END, GENE)
  expected.json                      {cohort: {sample: [cell per locus]}}, a cell
                                     the int the reference returns, or
                                     "Error:<exception class>" where it raises
                                     (run_mosdepth_single_cram turns any
                                     exception into "Error")

pysam is stubbed exactly as the reference's own test/conftest.py does.
"""
from __future__ import annotations

import json
import shutil
import sys
import tempfile
from pathlib import Path
from unittest.mock import MagicMock

HERE = Path(__file__).resolve().parent
DST = HERE / "g7_cover"
sys.path.insert(0, str(HERE.parent.parent))

from tests import cover_cases as cc  # noqa: E402


def write_inputs(root: Path):
    for cohort in cc.cases():
        cc.write_cohort(str(root / cohort), cohort)
    (root / "edge").mkdir()
    (root / "edge" / "Z0.regions.bed.gz").write_bytes(b"")
    whole = cc.bgzf(cc.cases()["main"]["texts"]["M5"])
    (root / "edge" / "Z1.regions.bed.gz").write_bytes(whole[: len(whole) // 2])
    (root / "loci.txt").write_text(cc.loci_file_text())


def run_reference(root: Path, ref: Path):
    sys.modules.setdefault("pysam", MagicMock())
    sys.path.insert(0, str(ref))
    from grid.utils.mosdepth import compute_region_coverage
    expected = {}
    for d in sorted(p for p in root.iterdir() if p.is_dir()):
        expected[d.name] = {}
        for f in sorted(d.glob("*.regions.bed.gz")):
            cells = []
            for chrom, start, end in cc.LOCI:
                try:
                    cells.append(compute_region_coverage(f, chrom, start, end))
                except Exception as e:
                    cells.append(f"Error:{type(e).__name__}")
            expected[d.name][f.name.split(".")[0]] = cells
    (root / "expected.json").write_text(json.dumps(expected, indent=0))
    return expected


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "grid" / "utils" / "mosdepth.py").exists():
        raise SystemExit("usage: make_golden_cover.py REFERENCE_DIR (the directory that holds grid/utils/mosdepth.py)")
    tmp = Path(tempfile.mkdtemp(prefix="golden_g7_cover_"))
    write_inputs(tmp)
    exp = run_reference(tmp, Path(sys.argv[1]))
    # what the cases hang on, as the reference sees it
    m = exp["main"]
    assert all(v == 0 for v in m["M4"]) and all(v == 0 for v in exp["edge"]["Z0"])
    assert all(str(v).startswith("Error") for v in exp["edge"]["Z1"])
    for s in ("M0", "M1", "M2", "M3", "M5"):
        assert [m[s][i] for i in cc.I_TIES] == cc.TIE_VALUES, s
        assert m[s][2] == 0 and m[s][3] == 0 and m[s][10] == 0 and m[s][11] == 0 and m[s][4] == m[s][7], s
    assert all(m["M0"][i] > 0 for i in cc.I_GEOM[:3]) and m["M1"][cc.I_GEOM[3]] == 6401
    h = exp["handover"]
    assert all(str(v).startswith("Error") for s in ("H2", "H3") for v in h[s])
    assert str(h["H6"][0]).startswith("Error") and str(h["H6"][cc.I_WHOLE]).startswith("Error") and h["H6"][1] > 0
    assert all(isinstance(v, int) for s in ("H0", "H1", "H4", "H5", "H7", "H8", "H9") for v in h[s])
    if DST.exists():
        shutil.rmtree(DST)
    shutil.copytree(tmp, DST)
    shutil.rmtree(tmp)
    print("g7_cover: ok", {k: len(v) for k, v in exp.items()})


if __name__ == "__main__":
    main()
