"""Step 6 over a loci table, host side (no GPU): the g6_loci fixture against the
oracle, the vectorised counts placement against the dict semantics of
_read_counts, and the path templates."""
import os

import numpy as np
import pandas as pd

from oracle import steps
from tests.dipcn_loci_cases import G6, g6_meta, g6_workdir
from tests.loci_cohort import LOCI_TABLE


def _names():
    from grid_amd.utils.compute_dipcn import _locus_name
    from grid_amd.utils.hi_inference import read_loci_file
    return [_locus_name(lc) for lc in read_loci_file(os.path.join(G6, "loci.txt"))]


def test_fixture_is_what_the_oracle_and_pandas_give():
    """Validates the fixture (passes without the loci mode): every expected
    file and status is the oracle's step 6 on that locus' counts, written as
    the reference writes it."""
    from grid_amd.utils.compute_dipcn import _read_counts, load_neighbors
    meta = g6_meta()
    names = _names()
    assert list(meta["status"]) == names and len(names) == 7
    neighbors, scales = load_neighbors(os.path.join(G6, "neighbors.zMax2.0.tsv.gz"))
    assert len(neighbors) == 40 and {len(l) for l in neighbors.values()} >= {3, 12}
    assert meta["ext"] not in neighbors and any(meta["ext"] in [x for x, _ in l] for l in neighbors.values())
    assert (meta["zero"], 0.0) in neighbors[meta["row"]]
    seen = set()
    for name in names:
        try:
            reads = _read_counts(os.path.join(G6, f"counts.{name}.tsv"))
            rows = steps.dipcn(neighbors, scales, reads, meta["n_nbr"])
            status = "ok"
        except (ZeroDivisionError, FileNotFoundError) as e:
            status = type(e).__name__
        assert status == meta["status"][name], name
        seen.add(status)
        exp = os.path.join(G6, "expected", f"dipcn.{name}.tsv")
        if status == "ok":
            text = pd.DataFrame(rows, columns=["Sample", "Norm_Reads"]).to_csv(sep="\t", index=False)
            assert open(exp).read() == text, name
        else:
            assert not os.path.exists(exp)
    assert seen == {"ok", "ZeroDivisionError", "FileNotFoundError"}


def test_place_counts_equals_the_dict_semantics(tmp_path):
    from grid_amd.utils.compute_dipcn import _read_counts, loci_ld, place_counts
    names = [f"S{i:02d}" for i in range(12)] + ["X1", "77"]
    index = pd.Index(np.array(names, dtype=object), dtype=object)
    files = {
        "plain": "Sample\tReads\nS03\t5\nS01\t7.5\nX1\t9\n",
        "dup_error": "Sample\tReads\nS04\t1\nS05\tError\nS04\t2\nS06\tinf\nS04\t3\nZZ\t8\n",     # last wins; ZZ unknown
        "numeric": "Sample\tReads\n77\t4\n1001\t6\n",                                    # ints: match no string id
        "header_only": "Sample\tReads\n",
    }
    ld = loci_ld(len(files))
    assert ld == 8 and loci_ld(8) == 8 and loci_ld(9) == 16 and loci_ld(0) == 0
    mat = np.zeros((len(names), ld))
    mat[:, len(files):] = np.nan
    for col, (key, text) in enumerate(files.items()):
        p = tmp_path / f"{key}.tsv"
        p.write_text(text)
        reads = _read_counts(p)
        place_counts(index, mat, col, reads)
        for r, sid in enumerate(names):                  # the reference's `sid in reads` / reads[sid]
            if sid in reads:
                assert mat[r, col] == float(reads[sid]), (key, sid)
            else:
                assert np.isnan(mat[r, col]), (key, sid)
    assert mat[4, 1] == 3.0 and np.isnan(mat[5, 1]) and np.isinf(mat[6, 1])
    assert np.isnan(mat[:, 2]).all() and np.isnan(mat[:, 3]).all()
    assert np.isnan(mat[:, len(files):]).all()           # the ldl padding


def test_default_output_template_is_step7s_default_input():
    from grid_amd.utils.compute_dipcn import _loci_config
    from grid_amd.utils.hi_inference import _locus_path, read_loci_file
    cfg = {"output_dir": "/o", "output_file_type": "tsv", "count_reads": {"output_file_prefix": "cnt"},
           "mosdepth": {"neighbors": {"output_file_prefix": "nb"}},
           "compute_diploid_genotypes": {"output_file_prefix": "dip", "loci_file": LOCI_TABLE}}
    loci, cnts, outs, nb_file, n_nbr = _loci_config(cfg)
    assert len(loci) == 734 and len(set(outs)) == 734 and n_nbr == 300
    assert str(nb_file) == "/o/nb.zMax2.0.tsv.gz"
    keys = dict(output_dir="/o", prefix="hap", dip_prefix="dip", type="tsv")
    for lc, c, o in zip(read_loci_file(LOCI_TABLE), cnts, outs):
        assert o == _locus_path("{output_dir}/{dip_prefix}.{locus}.{type}", lc, **keys)     # hi_inference_loci's default
        assert str(c) == f"/o/cnt.{lc['chrom']}_{lc['start']}_{lc['end']}_{lc['gene']}.tsv"
    cfg["compute_diploid_genotypes"].update(counts_file="/c/{count_prefix}/{chrom}/{gene}.{index}.{type}",
                                            loci_output="/d/{dip_prefix}.{start}-{end}.{type}")
    loci, cnts, outs, _, _ = _loci_config(cfg)
    assert str(cnts[1]) == "/c/cnt/1/TTLL10.1.tsv" and str(outs[1]) == "/d/dip.1184656-1184980.tsv"


def test_colliding_outputs_are_refused_before_the_device(tmp_path, monkeypatch):
    from grid_amd import engine
    from grid_amd.utils import compute_dipcn
    cfg = g6_workdir(tmp_path)
    cfg["compute_diploid_genotypes"]["loci_output"] = "{output_dir}/{dip_prefix}.chr{chrom}.{type}"

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(engine, "dipcn_loci", no_device)
    monkeypatch.setattr(compute_dipcn, "get_device", no_device)
    monkeypatch.setattr(compute_dipcn, "load_neighbors", no_device)
    assert compute_dipcn.compute_diploid_genotypes_loci(cfg, None) is None
    assert [f for f in os.listdir(cfg["output_dir"]) if f.startswith("dipcn")] == []
