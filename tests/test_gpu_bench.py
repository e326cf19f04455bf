"""bench.py's command line at a small shape (the chain headline): a plain run
times --steps steps and prints one result line without the --full records,
and --dump-outputs writes what the last timed pass computed -- the same bits
as the chain run here on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, STEPS, WARMUP = 96, 20000, 3, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    dump = tmp_path_factory.mktemp("bench_dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--samples", str(N), "--bins", str(M), "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}


def test_plain_run_prints_the_headline_only(plain_run):
    stdout, _ = plain_run
    lines = [x for x in stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["ms_per_step"] > 0
    # value = samples per second of the timed steps
    assert abs(d["value"] - N / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["config"]["samples"] == N and d["config"]["bins"] == M
    # what takes runs of its own is measured with --full only
    for key in ("cpu_baseline", "config3_1gpu", "ingest_roofline", "device_chain", "speedup_vs_cpu_baseline"):
        assert key not in d
    assert d["stages_ms"] is None


def test_dump_outputs_are_the_chain_outputs(plain_run):
    import bench
    from grid_amd import _abi
    from grid_amd.fused import Depth16, HipOps, Steps47, TorchAlloc
    _, got = plain_run
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    dev = _abi.Device(0)
    dev.set_stream(torch.cuda.current_stream())
    q = Depth16.synth(TorchAlloc(0), dev.ctx, bench.SEED, N, M, 0, bench.NCL)
    reads, off, nbr, w = bench.synth_reads_and_ibs(N)
    st = Steps47(HipOps(dev), TorchAlloc(0), N, M, 0, M, k=10, n_nbr=300, top_frac=0.1, zmax=2.0, sigma2_max=1000.0,
                 frac_r=1.0, min_nbr=1, n_iters=100)
    st.set_reads(reads)
    st.set_phasing_graph(off, nbr, w)
    st.run(q, q.ld)
    st.finish()
    torch.cuda.synchronize()
    cols = got["columns"].astype(np.int64)
    assert len(cols) == min(M, bench.DUMP_COLS) and (np.diff(cols) > 0).all()
    exp = {"row_means": st.rm[:N], "column_means": st.mu[:M].cpu()[cols], "column_variances": st.var[:M].cpu()[cols],
           "neighbors_index": st.idx_out[:N], "neighbors_d2": st.d2[:N], "neighbors_count": st.cnt_out[:N],
           "dipcn": st.dip[:N], "haploid": st.hap[: 2 * N], "haploid_imputed": st.imp[: 2 * N],
           "haploid_mean": st.mean}
    exp = {name: t.cpu().numpy().astype(np.float64) for name, t in exp.items()}
    # slots past a row's neighbour count and invalid dipCN rows hold nothing: NaN in the dump
    unused = np.arange(10)[None, :] >= exp["neighbors_count"][:, None]
    exp["neighbors_index"][unused] = np.nan
    exp["neighbors_d2"][unused] = np.nan
    exp["dipcn"][st.valid[:N].cpu().numpy() == 0] = np.nan
    assert np.isfinite(exp["dipcn"]).any() and np.isfinite(exp["haploid"]).any()
    for name, a in exp.items():
        assert np.array_equal(got[name], a, equal_nan=True), name
