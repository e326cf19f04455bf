"""The sharded steps 4-7 chain above 16 neighbours with the real HIP kernels:
k = 20 and 40 at world sizes 2, 3, 4 and 8, bin split and cohort split (ranks
sharing the one visible GPU, gloo standing in for RCCL), must take the row
exchange on every rank and give one rank's neighbours, dipCN and phasing bit
for bit.  The cohort and the checks are those of tests/test_gpu_sharded.py."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import test_gpu_sharded as base

pytestmark = pytest.mark.gpu


def run_chain(rank, world, comm, lanes, split, k):
    """base.run_chain (two passes, step 7 on its own lanes) that also reports
    the step-5 route the chain took."""
    import torch

    from grid_amd import _abi
    from grid_amd.fused import HipOps, Steps47, TorchAlloc, shard_range
    N, M = base.N, base.M
    q, reads, off, nbr, w = base.cohort()
    c0, c1 = shard_range(M, rank, world)
    dev = _abi.Device(0)
    dev.set_stream(torch.cuda.current_stream())
    qs = torch.from_numpy(np.ascontiguousarray(q[:, c0:c1])).cuda()
    pl = []
    for _ in range(lanes):
        pdev = _abi.Device(0)
        ps = torch.cuda.Stream()
        pdev.set_stream(ps)
        pl.append((HipOps(pdev), ps))
    pl = None if not pl else pl[0] if lanes == 1 else pl
    st = Steps47(HipOps(dev), TorchAlloc(0), N, M, c0, c1 - c0, k=k, n_nbr=4, n_iters=base.ITERS, comm=comm,
                 phase_lane=pl, split=split)
    st.set_reads(reads)
    st.set_phasing_graph(off, nbr, w)
    st.run(qs, c1 - c0)
    st.run(qs, c1 - c0)
    st.finish()
    torch.cuda.synchronize()
    ml = c1 - c0
    return {
        "rm": st.rm[:N].cpu().numpy(), "mu": st.mu[:ml].cpu().numpy(), "var": st.var[:ml].cpu().numpy(),
        "zq": st.zq_int32()[:N, : st.r_loc].cpu().numpy(), "idx": st.idx_out[:N].cpu().numpy(),
        "d2": st.d2[:N].cpu().numpy(), "dip": st.dip[:N].cpu().numpy(), "hap": st.hap[: 2 * N].cpu().numpy(),
        "imp": st.imp[: 2 * N].cpu().numpy(), "scale": st.scale, "ruse": st.ruse_loc,
        "row_exchange": bool(st.row_exchange), "full_rows": bool(st.full_rows),
    }


def _worker(rank, world, port, out_path, split, k):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from grid_amd.fused import TorchComm
    res = run_chain(rank, world, TorchComm(dist), 2 if world % 2 == 0 else 1, split, k)
    np.savez(f"{out_path}.{rank}.npz", **{key: np.asarray(v) for key, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def _run(world, tmp_path, split, k):
    port = base._free_port()
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, port, out, split, k), nprocs=world, join=True, start_method="spawn")
    return [dict(np.load(f"{out}.{r}.npz")) for r in range(world)]


_single = {}


def single(k):
    """The one-rank run at k (shared by the cases of that k)."""
    if k not in _single:
        _single[k] = run_chain(0, 1, None, 0, "bin", k)
        assert not _single[k]["row_exchange"] and not _single[k]["full_rows"]
    return _single[k]


@pytest.mark.parametrize("world,k,split", [(2, 20, "bin"), (3, 40, "bin"), (8, 20, "bin"), (2, 20, "cohort"),
                                           (4, 40, "cohort")])
def test_gpu_row_exchange_equals_single(world, k, split, tmp_path):
    one = single(k)
    assert one["idx"].shape == (base.N, k)
    parts = _run(world, tmp_path, split, k)
    for p in parts:
        assert bool(p["row_exchange"]) and not bool(p["full_rows"])
    base._check(parts, one)
