"""Sharded step 5 above the 16-key candidate lists (k + 1 > SEG_K1) on CPU:
the row exchange's slot rule, the pack / all-to-all / fill round trip on the
NumPy restatements (tests/wide_ops.py), and the chain under gloo -- bin split
and cohort split -- against one rank, whose order is the total (d2, j) order."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import wide_ops
from tests.test_sharded_gloo import FULL, ITERS, K_FULL, WIDE, _check_parts, _free_port, cohort


@pytest.mark.parametrize("W", range(1, 10))
def test_slot_rule_covers_every_tile_once(W):
    """Every tile T(b', b), b' < b, has its own (source rank, destination
    rank, slot); a pair p != q carries exactly two tiles and p == q one."""
    place = {}
    for b in range(2 * W):
        for bs in range(b):
            key = (wide_ops.own(bs, W), wide_ops.own(b, W), wide_ops.tile_slot(bs, b, W))
            assert key[2] in (0, 1)
            assert key not in place, (bs, b, place[key])
            place[key] = (bs, b)
    for p in range(W):
        for q in range(W):
            slots = sorted(s for (pp, qq, s) in place if (pp, qq) == (p, q))
            assert slots == ([0, 1] if p != q else [0]), (p, q)
    assert len(place) == W * (2 * W - 1)


@pytest.mark.parametrize("W,B", wide_ops.SHAPES)
def test_pack_exchange_fill_equals_definition(W, B):
    mat = wide_ops.exchange_matrix(W, B, seed=W * 100 + B)
    got = wide_ops.round_trip(mat, W, B, wide_ops.tiles_pack, wide_ops.rows_fill)
    for b in range(2 * W):
        assert np.array_equal(got[b], wide_ops.expected_rows(mat, B, b)), b


def run_chain(rank, world, comm, shape, split="bin", k=K_FULL, wide=True):
    from grid_amd.fused import Steps47, TorchAlloc, shard_range
    from tests.cpu_ops import NumpyOps
    N, M = shape
    q, reads, off, nbr, w = cohort(N, M)
    c0, c1 = shard_range(M, rank, world)
    qs = torch.from_numpy(np.ascontiguousarray(q[:, c0:c1]))
    ops = wide_ops.WideOps() if wide else NumpyOps()
    st = Steps47(ops, TorchAlloc("cpu"), N, M, c0, c1 - c0, k=k, n_nbr=3, n_iters=ITERS, comm=comm, split=split)
    st.set_reads(reads)
    st.set_phasing_graph(off, nbr, w)
    st.run(qs, c1 - c0)
    ml = c1 - c0
    return {
        "rm": st.rm.numpy()[:N].copy(), "mu": st.mu.numpy()[:ml].copy(), "var": st.var.numpy()[:ml].copy(),
        "sel": (st.sel.numpy()[: st.r_loc] + c0).copy(), "zq": st.zq_int32().numpy()[:N, : st.r_loc].copy(),
        "idx": st.idx_out.numpy()[:N].copy(), "d2": st.d2.numpy()[:N].copy(), "cnt": st.cnt_out.numpy()[:N].copy(),
        "dip": st.dip.numpy()[:N].copy(), "hap": st.hap.numpy()[: 2 * N].copy(),
        "imp": st.imp.numpy()[: 2 * N].copy(), "scale": st.scale, "ruse": st.ruse_loc,
        "row_exchange": bool(st.row_exchange), "full_rows": bool(st.full_rows),
    }


def _worker(rank, world, port, out_path, shape, split, k):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from grid_amd.fused import TorchComm
    res = run_chain(rank, world, TorchComm(dist), shape, split=split, k=k)
    np.savez(f"{out_path}.{rank}.npz", **{key: np.asarray(v) for key, v in res.items()})
    dist.barrier()
    dist.destroy_process_group()


def _run_world(world, shape, tmp_path, split="bin", k=K_FULL):
    port = _free_port()
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(world, port, out, shape, split, k), nprocs=world, join=True,
                       start_method="spawn")
    return [dict(np.load(f"{out}.{r}.npz")) for r in range(world)]


@pytest.fixture(scope="module")
def single_full():
    return run_chain(0, 1, None, FULL)


@pytest.fixture(scope="module")
def single_wide():
    return run_chain(0, 1, None, WIDE)


def _check_route(parts, single):
    assert not single["row_exchange"] and not single["full_rows"]
    for p in parts:
        assert bool(p["row_exchange"]) and not bool(p["full_rows"])
        assert np.array_equal(p["cnt"], single["cnt"])
    _check_parts(parts, single)


@pytest.mark.parametrize("world", [2, 3])
def test_bin_split_row_exchange_equals_single(single_full, world, tmp_path):
    _check_route(_run_world(world, FULL, tmp_path), single_full)


def test_bin_split_row_exchange_world_5_padded_blocks(single_wide, tmp_path):
    """n = 300, np = 512, W = 5: 2WB = 520 > np, and blocks 6-9 hold only
    padding rows -- their ranks still issue every collective."""
    _check_route(_run_world(5, WIDE, tmp_path), single_wide)


def test_cohort_split_row_exchange_equals_single(single_full, tmp_path):
    """The cohort split has no whole Gram: before the row exchange it refused
    k + 1 > SEG_K1."""
    _check_route(_run_world(2, FULL, tmp_path, split="cohort"), single_full)


def test_k_beyond_the_cohort_world_2(tmp_path):
    """k >= n - 1: every row lists all 47 others, unused slots hold (-1, 0)."""
    n, k = FULL[0], 60
    one = run_chain(0, 1, None, FULL, k=k)
    parts = _run_world(2, FULL, tmp_path, k=k)
    _check_route(parts, one)
    for p in parts:
        assert p["cnt"].tolist() == [n - 1] * n
        assert (p["idx"][:, n - 1:] == -1).all() and (p["d2"][:, n - 1:] == 0).all()
        assert all(sorted(p["idx"][i, : n - 1].tolist()) == [j for j in range(n) if j != i] for i in range(n))


def test_ops_without_the_tile_operations_keep_the_earlier_routes():
    """NumpyOps lacks seg_tiles_pack / seg_rows_fill: the bin split all-reduces
    the whole Gram as before, the cohort split raises as before; so does
    step5_wide="allreduce" on ops that have them."""
    from grid_amd._abi import GridNativeError
    from grid_amd.fused import SimComm, Steps47, TorchAlloc
    from tests.cpu_ops import NumpyOps
    mk = lambda ops, **kw: Steps47(ops, TorchAlloc("cpu"), 48, 8192, 0, 8192, k=20, comm=SimComm(2, 0), **kw)  # noqa: E731
    st = mk(NumpyOps())
    assert st.full_rows and not st.row_exchange
    with pytest.raises(GridNativeError, match="cohort split needs k"):
        mk(NumpyOps(), split="cohort")
    st = mk(wide_ops.WideOps(), step5_wide="allreduce")
    assert st.full_rows and not st.row_exchange
    assert mk(wide_ops.WideOps()).row_exchange and mk(wide_ops.WideOps(), split="cohort").row_exchange
    st = Steps47(wide_ops.WideOps(), TorchAlloc("cpu"), 48, 8192, 0, 8192, k=15, comm=SimComm(2, 0))
    assert not st.row_exchange and not st.full_rows          # k + 1 <= 16: the candidate path
    with pytest.raises(ValueError):
        mk(wide_ops.WideOps(), step5_wide="rows")
    with pytest.raises(ValueError):
        mk(wide_ops.WideOps(), split="cohort", step5_wide="allreduce")


def test_simulated_rank_counts_the_all_to_all():
    """SimComm.all_to_all copies the local block and counts the other W - 1
    blocks: (W-1) * 2 B^2 int64 into this rank per step."""
    from grid_amd.fused import SimComm
    comm = SimComm(4, 1)
    out, inp = torch.zeros(4 * 6, dtype=torch.int64), torch.arange(4 * 6, dtype=torch.int64)
    comm.all_to_all(out, inp, [6] * 4, [6] * 4)
    assert out.tolist() == [0] * 6 + list(range(6, 12)) + [0] * 12
    assert comm.bytes_in == {"all_to_all": 3 * 6 * 8}
    comm = SimComm(4, 1)
    res = run_chain(1, 4, comm, WIDE)
    B = 512 // 8
    assert res["row_exchange"] and comm.bytes_in["all_to_all"] == 3 * 2 * B * B * 8
    assert "reduce_scatter" in comm.bytes_in and res["idx"].shape == (WIDE[0], K_FULL)
