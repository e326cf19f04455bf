"""Region coverage on the device (grid_md_cover: mosdepth_dev.hip k_md_cover /
k_cov_walk, driven by grid_amd/utils/coverage_device.py) on the g7_cover
fixture -- the cohorts of tests/cover_cases.py, pinned against the reference
by tests/golden/make_golden_cover.py and explained without a GPU in
test_cover_cpu.py.  The device's coverage equals the reference's on every
cell, its two sums equal the host restatement's bit for bit (the fp64 sum in
file-line order), whatever the batches and the hit buffer; a file with a line
outside the grammar is recomputed on the host alone; and the step chains into
step 6's loci mode through run_wgs_pipeline."""
import functools
import json
import os
import shutil

import numpy as np
import pytest

from tests import cover_cases as cc

pytestmark = pytest.mark.gpu

G7 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_cover")
EXPECTED = json.load(open(os.path.join(G7, "expected.json")))


def _dev():
    from grid_amd.device import get_device
    return get_device()


def _samples(cohort):
    return sorted(EXPECTED[cohort])


def _paths(cohort):
    return [os.path.join(G7, cohort, f"{s}.regions.bed.gz") for s in _samples(cohort)]


@functools.lru_cache(maxsize=None)
def _host(cohort):
    """The restatement's sums per file, computed once: [(region_cov, covered_bp, error)]."""
    from grid_amd.utils.mosdepth import region_sums
    return [region_sums(p, cc.LOCI) for p in _paths(cohort)]


def _cover(cohort, n_loci=70, **kw):
    from grid_amd.utils.coverage_device import cover_files
    return cover_files(_dev(), _paths(cohort), cc.LOCI[:n_loci], **kw)


def _check(cohort, res, n_loci=70):
    exp_path = dict(cc.cases()[cohort]["path"]) if cohort in cc.cases() else {}
    for k, s in enumerate(_samples(cohort)):
        exp = [v if isinstance(v, int) else None for v in EXPECTED[cohort][s][:n_loci]]
        assert res.coverage[k] == exp, (cohort, s)
        if s in exp_path:
            assert res.path[k] == exp_path[s], (cohort, s)
        if res.path[k] == "failed":
            continue
        cov, bp, err = _host(cohort)[k]
        ok = [i for i in range(n_loci) if err[i] is None]
        assert res.covered_bp[k, ok].tolist() == [bp[i] for i in ok], (cohort, s)
        # bit for bit (nan cells of a nan depth compare as bits too)
        assert res.region_cov[k, ok].view(np.int64).tolist() == \
            np.array([cov[i] for i in ok], np.float64).view(np.int64).tolist(), (cohort, s)


@pytest.mark.parametrize("n_loci", cc.N_LOCI_CASES)
def test_main_cohort_every_cell_and_both_sums(n_loci):
    res = _cover("main", n_loci)
    _check("main", res, n_loci)
    assert res.path == ["device"] * 6 and res.regrown == 0 and res.batches == 1
    if n_loci == 70:
        m = {s: k for k, s in enumerate(_samples("main"))}
        assert [res.coverage[m["M0"]][i] for i in cc.I_TIES] == cc.TIE_VALUES
        assert res.coverage[m["M4"]] == [0] * 70
        assert all(res.coverage[m["M0"]][i] > 0 for i in cc.I_GEOM[:3]) and res.coverage[m["M1"]][cc.I_GEOM[3]] == 6401
        # the same nine lines forwards (M0) and backwards (M3): other bits, each the file's own order
        a, b = res.region_cov[m["M0"], cc.I_ORDER], res.region_cov[m["M3"], cc.I_ORDER]
        assert a.hex() == cc._sum(cc.order_terms()).hex() and b.hex() == cc._sum(cc.order_terms()[::-1]).hex()
        assert a.hex() != b.hex()


def test_handover_files_are_recomputed_on_the_host_alone():
    res = _cover("handover")
    _check("handover", res)
    record = dict(zip(_samples("handover"), res.path))
    assert record == cc.cases()["handover"]["path"]
    assert sorted(s for s, p in record.items() if p == "host") == sorted(cc.HANDOVER_KINDS)
    assert record["H0"] == record["H1"] == "device"


def test_two_batches_give_the_same_result():
    one, two = _cover("main"), _cover("main", batch_files=3)
    assert (one.batches, two.batches) == (1, 2)
    _check("main", two)
    assert two.coverage == one.coverage and two.path == one.path
    assert np.array_equal(two.region_cov.view(np.int64), one.region_cov.view(np.int64))
    assert np.array_equal(two.covered_bp, one.covered_bp)
    mixed = _cover("handover", batch_files=4)
    assert mixed.batches == 3
    _check("handover", mixed)


def test_hit_buffer_regrows_and_nothing_partial_escapes():
    one, small = _cover("main"), _cover("main", hit_capacity=5)
    assert small.regrown >= 1
    _check("main", small)
    assert small.coverage == one.coverage
    assert np.array_equal(small.region_cov.view(np.int64), one.region_cov.view(np.int64))
    assert np.array_equal(small.covered_bp, one.covered_bp)


def test_raw_call_with_a_small_buffer_writes_nothing():
    """grid_md_cover itself: with room for fewer hits than the batch has it
    reports the number needed and leaves the outputs as they were."""
    import ctypes as C
    import gzip
    from grid_amd._abi import call
    from grid_amd.utils.coverage_device import LociTable
    from grid_amd.utils.ingest_device import _chunks
    dev = _dev()
    text = np.frombuffer(gzip.decompress(open(_paths("main")[0], "rb").read()), np.uint8)
    table = LociTable(dev, cc.LOCI)
    tlen, toff = np.array([text.size], np.int64), np.zeros(1, np.int64)
    cfile, cstart, cfirst, nch = _chunks([0], tlen)
    d_text = dev.upload(np.concatenate([text, np.zeros(256, np.uint8)]))
    d = [dev.upload(x) for x in (toff, tlen, cfile, cstart, cfirst)]
    cnl, cline0, flags = dev.alloc(nch, np.int32), dev.alloc(nch, np.int64), dev.zeros(1, np.int32)
    call("grid_md_count", dev.ctx, d_text.ptr, d[0].ptr, d[1].ptr, nch, d[2].ptr, d[3].ptr, d[4].ptr, 1, cnl.ptr,
         cline0.ptr, flags.ptr, None)
    ld = 72
    outs = [dev.alloc((1, ld), t).fill_bytes(0x5A) for t in (np.float64, np.int64, np.int64)]

    def run(cap):
        hits = (dev.alloc(max(cap, 1), np.uint64), dev.alloc(max(cap, 1), np.int64), dev.alloc(max(cap, 1), np.int32))
        need = C.c_int64()
        call("grid_md_cover", dev.ctx, d_text.ptr, d[0].ptr, d[1].ptr, nch, d[2].ptr, d[3].ptr, cline0.ptr, None, 1,
             C.byref(table.desc), hits[0].ptr, hits[1].ptr, hits[2].ptr, cap, C.byref(need), outs[0].ptr,
             outs[1].ptr, outs[2].ptr, ld, flags.ptr)
        return need.value
    cov, bp, err = _host("main")[0]
    need = run(7)
    assert need > 7
    for o in outs:
        assert (o.numpy().view(np.uint8) == 0x5A).all()
    assert run(need) == need
    assert outs[1].numpy()[0, :70].tolist() == bp and flags.numpy()[0] == 0
    assert outs[0].numpy()[0, :70].view(np.int64).tolist() == np.array(cov).view(np.int64).tolist()
    assert outs[2].numpy()[0, :70].tolist() == EXPECTED["main"][_samples("main")[0]]
    assert (outs[2].numpy()[0, 70:] == 0).all()


def test_edge_files_empty_and_truncated():
    res = _cover("edge")
    assert res.path == ["device", "failed"]
    assert res.coverage[0] == [0] * 70 and res.coverage[1] == [None] * 70
    _check("edge", res)


def test_a_file_the_device_refuses_is_inflated_on_the_host(monkeypatch):
    """The plain gzip file's device status forced to "bad data": the host
    inflates it, the device parses its text, the values do not change."""
    from grid_amd import _abi
    from grid_amd.utils import coverage_device as cd
    real = cd._gpu_inflate

    def refuse_whole_files(dev, d_in, d_text, units, mcap):
        out = real(dev, d_in, d_text, units, mcap)
        if mcap > 1:
            out[2].copy_from(np.full(len(units[0]), _abi.GZ_EDATA, np.int32))
        return out
    monkeypatch.setattr(cd, "_gpu_inflate", refuse_whole_files)
    res = _cover("main")
    record = dict(zip(_samples("main"), res.path))
    assert record["M5"] == "device:host-inflate" and record["M4"] == "device:host-inflate"
    assert all(record[s] == "device" for s in ("M0", "M1", "M2", "M3"))
    for k, s in enumerate(_samples("main")):
        assert res.coverage[k] == EXPECTED["main"][s], s


def test_pipeline_coverage_then_step6_loci(tmp_path):
    """coverage over a loci table -> step 6's loci mode reading the coverage
    files through its counts_file template: the dipCN files equal those of the
    single-region step run per region on the same coverage files."""
    import yaml
    from grid_amd.pipeline import run_wgs_pipeline
    from grid_amd.utils.compute_dipcn import _locus_name, compute_diploid_genotypes
    from grid_amd.utils.hi_inference import read_loci_file
    from tests.dipcn_loci_cases import G6, g6_meta
    meta = g6_meta()
    loci = read_loci_file(os.path.join(G6, "loci.txt"))
    ids = [f"HG{i:05d}" for i in range(40)]
    work, out = tmp_path / "md", tmp_path / "out"
    work.mkdir()
    out.mkdir()
    shutil.copy(os.path.join(G6, "neighbors.zMax2.0.tsv.gz"), out)
    rng = np.random.default_rng(77)
    for sid in ids:
        if sid == meta["zero"]:
            continue                                  # no file: logged, left out (and ROW's zero scale never met)
        lines = []
        for lc in loci:
            s0 = lc["start"] // 1000 * 1000 - 2000
            for s in range(s0, lc["end"] + 2000, 1000):
                lines.append(f"{lc['chrom']}\t{s}\t{s + 1000}\t{rng.uniform(15, 60):.2f}\n")
        (work / f"{sid}.regions.bed.gz").write_bytes(cc.bgzf("".join(lines).encode()))
    (tmp_path / "samples.txt").write_text("\n".join(ids) + "\n")
    cfg = {"samples_file": str(tmp_path / "samples.txt"), "output_dir": str(out), "output_file_type": "tsv",
           "index": {"run": None}, "count_reads": {"run": False, "output_file_prefix": "counts"},
           "mosdepth": {"run": False, "work_dir": str(work), "output_file_prefix": "cov",
                        "coverage": {"run": True, "loci_file": os.path.join(G6, "loci.txt")},
                        "normalize": {"run": False},
                        "neighbors": {"run": False, "zmax": 2.0, "output_file_prefix": "neighbors"}},
           "compute_diploid_genotypes": {"run": True, "output_file_prefix": "dipcn", "n_nbr": meta["n_nbr"],
                                         "loci_file": os.path.join(G6, "loci.txt"),
                                         "counts_file": "{output_dir}/cov.{locus}.{type}"},
           "compute_haploid_genotypes": {"run": False}, "gpu": {"device": 0}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    run_wgs_pipeline(console=None, config=str(tmp_path / "cfg.yaml"))
    from grid_amd.utils.mosdepth import compute_region_coverage
    for lc in loci:
        name = _locus_name(lc)
        cov = (out / f"cov.{name}.tsv").read_text().splitlines()
        assert cov[0] == f"Sample\t{lc['chrom']}:{lc['start']}-{lc['end']}"
        assert [r.split("\t")[0] for r in cov[1:]] == [s for s in ids if s != meta["zero"]]
        first = compute_region_coverage(work / f"{ids[0]}.regions.bed.gz", lc["chrom"], lc["start"], lc["end"])
        assert cov[1] == f"{ids[0]}\t{first}" and first > 0
        one = json.loads(json.dumps(cfg))
        one["count_reads"]["output_file_prefix"] = f"cov.{name}"
        one["compute_diploid_genotypes"] = {"run": True, "output_file_prefix": f"single.{name}",
                                            "n_nbr": meta["n_nbr"]}
        compute_diploid_genotypes(one, None)
        got = (out / f"dipcn.{name}.tsv").read_text()
        assert got == (out / f"single.{name}.tsv").read_text() and got.count("\n") > 20, name
