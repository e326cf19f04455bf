"""The distributed drop-in above 16 neighbours: `grid wgs` with
num_neighbors: 20 on one GPU against 2 ranks sharing that GPU (gloo through
host memory, as tests/test_gpu_dist_wgs.py).  dist_step4 hands the config's k
to Steps47(split="bin"), which now takes the row exchange; every output
file's text must equal the one-GPU run's."""
import os
import shutil

import pytest
import yaml

from tests.test_gpu_dist_wgs import FILES, _content, _run

pytestmark = pytest.mark.gpu
K = 20


def test_dist_wgs_20_neighbours_equals_one_gpu(tmp_path):
    import bench
    data, out1, outw = tmp_path / "data", tmp_path / "out1", tmp_path / "out"
    cfg_path, _, _ = bench.prepare_files_cohort(str(data), str(out1), 203, 25_000, gen_threads=8, threads=4)
    c = yaml.safe_load(open(cfg_path))
    c["mosdepth"]["neighbors"]["num_neighbors"] = K
    with open(cfg_path, "w") as f:
        yaml.safe_dump(c, f)
    from grid_amd.pipeline import run_wgs_pipeline
    run_wgs_pipeline(console=None, config=cfg_path)
    os.makedirs(outw)
    shutil.copy(out1 / "counts.tsv", outw / "counts.tsv")
    c["output_dir"] = str(outw)
    p = tmp_path / "config.yaml"
    p.write_text(yaml.safe_dump(c))
    logs = _run(2, str(p), tmp_path)
    assert "Failed" not in logs and "rank 0 reads the cohort" not in logs, logs
    for f in FILES:
        assert _content(outw / f) == _content(out1 / f), f
    rows = _content(outw / FILES[1]).splitlines()       # id, scale, then (id, scale, distance) per neighbour
    assert len(rows) == 203 and all(len(r.split("\t")) == 2 + 3 * K for r in rows)
