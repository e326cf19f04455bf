#!/usr/bin/env python3
"""Generate tests/golden/g6_loci/: step 6 over a loci table, pinned against the
REFERENCE implementation (read-only at /root/reference) run once per locus.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_loci6.py

What it writes (data only, a few tens of KB):
  loci.txt                     the first 7 regions of loci/734_...uniq.txt
  neighbors.zMax2.0.tsv.gz     40 rows, lists of 3-12 entries (n_nbr = 4 is
                               smaller than most), a neighbour id that is no
                               row (EXT0001), one list entry with scale 0.00
                               (ZERO in row ROW's list), one one-field line
  counts.{locus}.tsv           per locus; none for locus 4
  expected/dipcn.{locus}.tsv   what the reference's compute_diploid_genotypes
                               wrote with count_reads.output_file_prefix =
                               counts.{locus} and compute_diploid_genotypes.
                               output_file_prefix = dipcn.{locus}
  expected/status.json         {locus: "ok" | "ZeroDivisionError" | "FileNotFoundError"}
  config.json                  n_nbr and the ids the cases hang on

The loci ({locus} = chrom_start_end_gene):
  0  samples absent, an Error row, a duplicated sample (last one wins), a
     non-integer count; ZERO absent                                   -> ok
  1  other samples absent, the non-row id has a count; ZERO absent    -> ok
  2  ZERO has a count and is consulted by ROW                         -> ZeroDivisionError
  3  every count is 0 (mean == 0); ZERO absent                        -> ZeroDivisionError
  4  no counts file                                                   -> FileNotFoundError
  5  ZERO has a count but ROW has none (its list is never walked)     -> ok
  6  an all-numeric id column: pandas parses ints that match no id    -> ok, header only

pysam is stubbed exactly as the reference's own test/conftest.py does.
"""
from __future__ import annotations

import gzip
import json
import shutil
import sys
import tempfile
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
DST = HERE / "g6_loci"
TABLE = HERE / "loci" / "734_possible_coding_vntr_regions.IBD2R_gt_0.25.uniq.txt"
N, N_LOCI, N_NBR = 40, 7, 4


def locus_names(table_lines):
    head = table_lines[0].split("\t")
    c, s, e, g = (head.index(k) for k in ("CHR", "BP_START_HG38", "BP_END_HG38", "GENE"))
    return [f"{p[c]}_{p[s]}_{p[e]}_{p[g]}" for p in (ln.split("\t") for ln in table_lines[1:])]


def write_inputs(root: Path):
    rng = np.random.default_rng(606)
    rows = TABLE.read_text().splitlines()[: 1 + N_LOCI]
    (root / "loci.txt").write_text("\n".join(rows) + "\n")
    names = locus_names(rows)
    ids = [f"HG{i:05d}" for i in range(N)]
    ext = "EXT0001"
    row, zero = ids[2], ids[5]
    scale = {s: float(f"{rng.uniform(0.8, 1.25):.4f}") for s in ids + [ext]}
    lines = []
    for i, sid in enumerate(ids):
        k = int(rng.integers(3, 13))
        pool = [x for x in ids if x not in (sid, zero)]
        lst = [str(x) for x in rng.choice(pool, size=k, replace=False)]
        if i % 6 == 1:
            lst[int(rng.integers(0, k))] = ext              # a neighbour that is no row
        if sid == row:
            lst[1] = zero                                   # consulted: second of n_nbr = 4
        parts = [sid, f"{scale[sid]:.4f}"]
        for x in lst:
            sc = "0.00" if (sid == row and x == zero) else f"{scale[x]:.4f}"
            parts += [x, sc, f"{rng.uniform(5, 60):.3f}"]
        lines.append("\t".join(parts))
        if i == 17:
            lines.append("malformed-one-field-line")
    with open(root / "neighbors.zMax2.0.tsv.gz", "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
            f.write(("\n".join(lines) + "\n").encode())

    def counts(k):
        """Locus k's file lines (None: no file)."""
        if k == 4:
            return None
        if k == 6:
            return ["Sample\tReads"] + [f"{1000 + i}\t{int(rng.integers(50, 400))}" for i in range(N)]
        present = [s for s in ids if rng.random() < 0.85]
        if k in (0, 1, 3):
            present = [s for s in present if s != zero]
        if k == 2:
            present = sorted(set(present) | {row, zero}, key=ids.index)
        if k == 5:
            present = sorted((set(present) | {zero}) - {row}, key=ids.index)
        out = ["Sample\tReads"]
        for s in present:
            out.append(f"{s}\t{0 if k == 3 else int(rng.integers(50, 400))}")
        if k == 0:
            out.insert(4, f"{ids[30]}\tError")              # dropped by to_numeric + dropna
            out = [ln for ln in out if not ln.startswith(ids[31] + "\t")]
            out.insert(6, f"{ids[31]}\t77")                 # duplicated: the later row wins
            out.append(f"{ids[31]}\t215.5")
            out.append("HG99999\t123")                      # an id outside the universe
        if k == 1:
            out.append(f"{ext}\t181")
        return out

    for k, name in enumerate(names):
        c = counts(k)
        if c is not None:
            (root / f"counts.{name}.tsv").write_text("\n".join(c) + "\n")
    (root / "config.json").write_text(json.dumps({"n_nbr": N_NBR, "row": row, "zero": zero, "ext": ext}, indent=1))
    return names


def run_reference(root: Path, names):
    sys.modules.setdefault("pysam", MagicMock())
    sys.path.insert(0, str(REF))
    from rich.console import Console
    import grid.cli
    from grid.utils import compute_dipcn as ref_dip
    console = Console(theme=grid.cli.grid_theme, quiet=True)
    (root / "expected").mkdir()
    status = {}
    for name in names:
        cfg = {"output_dir": str(root), "output_file_type": "tsv",
               "count_reads": {"output_file_prefix": f"counts.{name}"},
               "mosdepth": {"neighbors": {"zmax": 2.0, "output_file_prefix": "neighbors"}},
               "compute_diploid_genotypes": {"output_file_prefix": f"dipcn.{name}", "n_nbr": N_NBR}}
        try:
            ref_dip.compute_diploid_genotypes(cfg, console)
            status[name] = "ok"
            shutil.move(root / f"dipcn.{name}.tsv", root / "expected" / f"dipcn.{name}.tsv")
        except (ZeroDivisionError, FileNotFoundError) as e:
            status[name] = type(e).__name__
    (root / "expected" / "status.json").write_text(json.dumps(status, indent=1))
    return status


def main():
    tmp = Path(tempfile.mkdtemp(prefix="golden_g6_loci_"))
    names = write_inputs(tmp)
    status = run_reference(tmp, names)
    want = ["ok", "ok", "ZeroDivisionError", "ZeroDivisionError", "FileNotFoundError", "ok", "ok"]
    if [status[n] for n in names] != want:
        raise RuntimeError(f"g6_loci: the reference's statuses are {status}, the cases need {want}")
    if DST.exists():
        shutil.rmtree(DST)
    shutil.copytree(tmp, DST)
    shutil.rmtree(tmp)
    print("g6_loci: ok", status)


if __name__ == "__main__":
    main()
