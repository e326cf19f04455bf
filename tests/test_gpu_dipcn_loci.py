"""Step 6 over a loci table on the GPU (grid_dipcn_loci): the batched kernel
against the oracle and the one-locus kernel bit for bit, per-locus zero
division, groups, the missed-id counts, and the step on the g6_loci fixture,
against the single-locus step, chained into step 7 and over two ranks."""
import os
import socket

import numpy as np
import pytest

from tests.dipcn_loci_cases import (G6, g6_meta, g6_workdir, missing_ids_count, oracle_locus, same_bits,
                                    single_locus_config, synth)

pytestmark = pytest.mark.gpu


def _dev():
    from grid_amd.device import get_device
    return get_device()


def _run(c, n_nbr, **kw):
    from grid_amd import engine
    return engine.dipcn_loci(_dev(), c["reads"], c["scale"], c["nbr"], c["nsc"], c["cnt"], n_nbr, c["n"], **kw)


def _one_locus(c, col, n_nbr):
    """The existing one-locus kernel on column ``col``."""
    from grid_amd import engine
    has = ~np.isnan(c["reads"][:, col])
    return engine.dipcn(_dev(), np.where(has, c["reads"][:, col], 0.0), has.astype(np.uint8), c["scale"], c["nbr"],
                        c["nsc"], c["cnt"], n_nbr, n_rows=c["n"])


_CASES = {}


def _parity_case(n_loci):
    """n = 70, universe n + 5, lists of 9 with ncnt 0..9; the edge loci."""
    if n_loci not in _CASES:
        c = synth(70, 5, 9, n_loci, seed=100 + n_loci)
        row = int(np.flatnonzero(c["cnt"] == 9)[0])
        c["reads"][:, 0] = np.arange(1, c["u"] + 1) * 3.0          # a locus with everything present
        c["reads"][c["nbr"][row, 0], 0] = np.inf                   # one inf count: it stays a value, and
        c["reads"][row, 0] = np.inf                                # this row's output is inf/inf, a valid NaN
        if n_loci > 1:
            c["reads"][:, n_loci - 1] = np.nan                     # a locus with nothing present
        if n_loci > 2:
            c["reads"][row, 1] = 77.0                              # a row whose neighbours are all absent
            c["reads"][c["nbr"][row, :9], 1] = np.nan
        c["row"] = row
        _CASES[n_loci] = c
    return _CASES[n_loci]


@pytest.mark.parametrize("n_loci", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n_nbr", [1, 4, 9, 20])
def test_kernel_parity(n_loci, n_nbr):
    c = _parity_case(n_loci)
    out, valid, zerodiv, _ = _run(c, n_nbr)
    assert out.shape == (70, n_loci) and valid.shape == (70, n_loci) and not zerodiv.any()
    for col in range(n_loci):
        e_out, e_valid = oracle_locus(c, col, n_nbr)
        assert np.array_equal(valid[:, col], e_valid), col
        assert same_bits(out[e_valid, col], e_out[e_valid]), col
        if col in (0, 1, n_loci // 2, n_loci - 1):                 # the one-locus kernel (a launch each)
            k_out, k_valid = _one_locus(c, col, n_nbr)
            assert np.array_equal(k_valid, e_valid) and same_bits(k_out[e_valid], out[e_valid, col]), col
    assert valid[:, 0].sum() == (c["cnt"] > 0).sum()
    assert valid[c["row"], 0] and np.isnan(out[c["row"], 0])
    if n_loci > 1:
        assert not valid[:, n_loci - 1].any()
    if n_loci > 2:
        assert not valid[c["row"], 1]                               # count == 0: no output


def test_zero_division_is_per_locus():
    c = synth(40, 3, 8, 6, seed=7, p_present=1.1)                  # everything present
    c["cnt"][:] = 8
    for i in range(40):
        c["nbr"][i] = (i + 1 + np.arange(8)) % c["u"]
    c["nsc"] = np.random.default_rng(8).uniform(0.7, 1.4, c["nbr"].shape)
    n_nbr = 4
    # row 3: a zero scale on its second neighbour j, present at locus 0, absent at locus 1
    j = int(c["nbr"][3, 1])
    c["nsc"][3, 1] = 0.0
    c["reads"][j, 1:] = np.nan
    # row 9: a zero scale after the n_nbr-th present neighbour: never used
    c["nsc"][9, 5] = 0.0
    # row 20: sample scale 0, counts at loci 0 and 2 only
    c["scale"][20] = 0.0
    c["reads"][20, [1, 3, 4, 5]] = np.nan
    # locus 3: all counts 0 (mean == 0); row 3's zero-scale neighbour stays absent
    c["reads"][~np.isnan(c["reads"][:, 3]), 3] = 0.0
    out, valid, zerodiv, _ = _run(c, n_nbr)
    assert zerodiv.tolist() == [True, False, True, True, False, False]
    for col in (1, 4, 5):
        e_out, e_valid = oracle_locus(c, col, n_nbr)
        assert e_valid[3] and e_valid[9] and not e_valid[20]
        assert np.array_equal(valid[:, col], e_valid) and same_bits(out[e_valid, col], e_out[e_valid])
    for col in (0, 2, 3):
        with pytest.raises(ZeroDivisionError):
            oracle_locus(c, col, n_nbr)
    # locus 2 is flagged by row 20's scale alone: without that row it is clean
    c["reads"][20, 2] = np.nan
    assert _run(c, n_nbr)[2].tolist() == [True, False, False, True, False, False]


def test_groups_equal_one_group():
    c = synth(50, 4, 7, 8, seed=21)
    c["nsc"][11, 0] = 0.0                                          # a flagged locus or two among them
    one = _run(c, 3)
    grouped = _run(c, 3, group=3)
    assert same_bits(one[0], grouped[0])
    for a, b in zip(one[1:], grouped[1:]):
        assert np.array_equal(a, b)
    assert one[1].any() and one[3].any()


@pytest.mark.parametrize("n_nbr", [1, 3, 20])
def test_missed_id_counts(n_nbr):
    c = synth(60, 6, 8, 70, seed=33, p_present=0.7)
    c["reads"][:, 2] = np.nan
    c["reads"][:, 3] = 5.0
    _, _, zerodiv, missed = _run(c, n_nbr)
    assert not zerodiv.any()
    exp = [missing_ids_count(c, col, n_nbr) for col in range(70)]
    assert missed.tolist() == exp
    assert exp[2] == 0 and exp[3] == 0 and max(exp) > 0


def _outputs(out_dir):
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))
            if f.startswith("dipcn.")}


def _expected_g6():
    meta = g6_meta()
    return {f"dipcn.{name}.tsv": open(os.path.join(G6, "expected", f"dipcn.{name}.tsv"), "rb").read()
            for name, st in meta["status"].items() if st == "ok"}


def test_step_on_the_fixture(tmp_path, capsys):
    from grid_amd.utils.compute_dipcn import compute_diploid_genotypes_loci
    cfg = g6_workdir(tmp_path)
    done = compute_diploid_genotypes_loci(cfg, None)
    exp = _expected_g6()
    assert len(exp) == 4 and _outputs(cfg["output_dir"]) == exp     # failed loci: no file; the others written
    assert sorted(d["index"] for d in done) == [0, 1, 5, 6]
    text = capsys.readouterr().out
    assert text.count("Failed to compute diploid CNV calls: float division by zero") == 2
    assert "1_1310773_1310936_PUSL1" in text and "1_1708835_1708932_CDK11A" in text
    assert text.count("Failed to compute diploid CNV calls:") == 3 and "1_1955019_1955089_CFAP74" in text
    assert "neighbor IDs not found in read counts" in text


def test_loci_mode_equals_the_single_locus_step(tmp_path):
    from grid_amd.utils.compute_dipcn import compute_diploid_genotypes, compute_diploid_genotypes_loci
    cfg = g6_workdir(tmp_path / "loci")
    compute_diploid_genotypes_loci(cfg, None, group=3)
    ref = g6_workdir(tmp_path / "single")
    for name, status in g6_meta()["status"].items():
        try:
            compute_diploid_genotypes(single_locus_config(ref, name), None)
            assert status == "ok", name
        except (ZeroDivisionError, FileNotFoundError) as e:
            assert status == type(e).__name__, name
            # the reference's step dies before it writes; ours may not leave a file either
            assert not os.path.exists(os.path.join(ref["output_dir"], f"dipcn.{name}.tsv"))
    assert _outputs(cfg["output_dir"]) == _outputs(ref["output_dir"]) and len(_outputs(ref["output_dir"])) == 4


def _cohort_with_counts(root):
    """tests/loci_cohort.py's cohort with step 6's inputs: a neighbours file
    and per-locus count files; its hand-written dipCN files are removed."""
    import gzip
    from grid_amd.utils.compute_dipcn import _locus_name
    from grid_amd.utils.hi_inference import read_loci_file
    from tests.loci_cohort import write_cohort
    cfg, table = write_cohort(str(root))
    out = cfg["output_dir"]
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    rng = np.random.default_rng(3)
    ids = [f"HG{i:05d}" for i in range(60)]
    scale = rng.uniform(0.8, 1.2, 60)
    with gzip.open(os.path.join(out, "neighbors.zMax2.0.tsv.gz"), "wt") as f:
        for i in range(60):
            lst = rng.choice([x for x in range(60) if x != i], size=int(rng.integers(4, 15)), replace=False)
            f.write("\t".join([ids[i], f"{scale[i]:.4f}"] + [f"{ids[j]}\t{scale[j]:.4f}\t{rng.uniform(1, 9):.3f}"
                                                             for j in lst]) + "\n")
    for lc in read_loci_file(table):
        with open(os.path.join(out, f"counts.{_locus_name(lc)}.tsv"), "w") as f:
            f.write("Sample\tReads\n")
            for i in range(60):
                if rng.random() < 0.95:
                    f.write(f"{ids[i]}\t{int(rng.integers(40, 500))}\n")
    cfg["count_reads"] = {"run": False, "output_file_prefix": "counts"}
    cfg["mosdepth"] = {"run": False, "normalize": {"run": False},
                       "neighbors": {"run": False, "zmax": 2.0, "output_file_prefix": "neighbors"}}
    cfg["index"] = {"run": False}
    cfg["compute_diploid_genotypes"].update(run=True, loci_file=table, n_nbr=5)
    return cfg


def test_pipeline_chains_step6_into_step7(tmp_path):
    import yaml
    from grid_amd.pipeline import run_wgs_pipeline
    from tests.loci_cohort import expected_outputs
    cfg = _cohort_with_counts(tmp_path)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    run_wgs_pipeline(console=None, config=str(p))
    assert len(_outputs(cfg["output_dir"])) == 7                    # step 6's files, read by the oracle's step 7
    exp = expected_outputs(cfg)
    assert len(exp) == 7
    for path, text in exp.items():
        assert open(path).read() == text and text.count("\n") > 40, path


def _worker(rank, world, port, cfg):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("LOCAL_RANK", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from grid_amd.utils.compute_dipcn import compute_diploid_genotypes_loci
    done = compute_diploid_genotypes_loci(cfg, None)
    assert sorted(d["index"] for d in done) == [i for i in (0, 1, 5, 6) if i % world == rank]
    dist.destroy_process_group()


def test_loci_sharded_world2(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cfg = g6_workdir(tmp_path)
    mp.start_processes(_worker, args=(2, port, cfg), nprocs=2, join=True, start_method="spawn")
    assert _outputs(cfg["output_dir"]) == _expected_g6()
