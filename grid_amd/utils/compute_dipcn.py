"""Step 6 -- neighbour-normalised diploid copy number, MI355X path.

Drop-in for grid/utils/compute_dipcn.py.  Counts and neighbour files are
read exactly as the reference reads them (pandas for the counts, :46-49);
the per-sample gather-ratio (:62-88) runs as a HIP kernel
(grid_amd/csrc/dipcn_phase.hip) in fp64 with the reference's operation
order, including its ZeroDivisionError cases.
"""
from __future__ import annotations

import gzip
from pathlib import Path

import numpy as np
import pandas as pd

from .. import engine
from ..device import get_device
from .utils import log, progress_bar


def load_neighbors(neighbors_file):
    """:105-152 -> ({id: [(nbr_id, nbr_scale), ...]}, {id: scale})."""
    neighbors, scales = {}, {}
    with gzip.open(neighbors_file, "rt") as f:
        for line in f:
            parts = line.strip().split("\t")
            if len(parts) < 2:
                continue
            try:
                s = float(parts[1])
            except ValueError:
                continue
            scales[parts[0]] = s
            lst = []
            i = 2
            while i + 2 <= len(parts):
                try:
                    lst.append((parts[i], float(parts[i + 1])))
                except ValueError:
                    pass
                i += 3
            neighbors[parts[0]] = lst
    return neighbors, scales


def _read_counts(path) -> dict:
    """:46-49, verbatim semantics (pandas parses all-numeric IDs as ints)."""
    raw = pd.read_csv(path, sep="\t", header=0, names=["Sample", "Reads"])
    raw["Reads"] = pd.to_numeric(raw["Reads"], errors="coerce")
    raw.dropna(subset=["Reads"], inplace=True)
    return raw.set_index("Sample")["Reads"].to_dict()


def dipcn_arrays(neighbors: dict, sample_scales: dict, reads: dict, n_nbr: int, dev=None):
    """Run the device kernel on dict inputs; returns ([(id, value)], missing_ids)."""
    ids = list(neighbors)
    n = len(ids)
    universe = {sid: i for i, sid in enumerate(ids)}
    for lst in neighbors.values():
        for nid, _ in lst:
            if nid not in universe:
                universe[nid] = len(universe)
    u = len(universe)
    names = list(universe)
    has = np.array([x in reads for x in names], dtype=np.uint8)
    rd = np.array([float(reads[x]) if h else 0.0 for x, h in zip(names, has)], dtype=np.float64)
    k = max((len(l) for l in neighbors.values()), default=0)
    nbr = np.full((max(n, 1), max(k, 1)), -1, dtype=np.int32)
    nsc = np.zeros((max(n, 1), max(k, 1)), dtype=np.float64)
    cnt = np.zeros(max(n, 1), dtype=np.int32)
    scale = np.zeros(max(u, 1), dtype=np.float64)
    missing = set()
    for i, sid in enumerate(ids):
        lst = neighbors[sid]
        cnt[i] = len(lst)
        scale[i] = sample_scales[sid]
        c = 0
        for t, (nid, ns) in enumerate(lst):
            nbr[i, t] = universe[nid]
            nsc[i, t] = ns
            if c < n_nbr and sid in reads:
                if nid in reads:
                    c += 1
                else:
                    missing.add(nid)
    if n == 0:
        return [], missing
    out, valid = engine.dipcn(dev or get_device(), rd, has, scale, nbr, nsc, cnt, int(n_nbr), n_rows=n)
    return [(ids[i], float(out[i])) for i in range(n) if valid[i]], missing


def compute_diploid_genotypes(config, console) -> None:
    """Step entry point (:10-101)."""
    try:
        prefix = config.get("compute_diploid_genotypes", {}).get("output_file_prefix", None)
        ftype = config.get("output_file_type", "tsv")
        output_dir = config.get("output_dir", ".")
        output_file = Path(f"{output_dir}/{prefix}.{ftype}")
        n_nbr = config.get("compute_diploid_genotypes", {}).get("n_nbr", 300)
        counts_prefix = config["count_reads"].get("output_file_prefix", None)
        counts_file = Path(f"{output_dir}/{counts_prefix}.{ftype}")
        zmax = config["mosdepth"]["neighbors"].get("zmax", 2.0)
        nb_prefix = config["mosdepth"]["neighbors"].get("output_file_prefix", None)
        neighbors_file = Path(f"{output_dir}/{nb_prefix}.zMax{zmax:.1f}.{ftype}.gz")
    except Exception as e:
        log(console, f"Config error: {e}", style="danger")
        return

    from .dist_step4 import dist_comm, rank0_step
    comm = dist_comm()
    if comm is not None:                    # torch.distributed: rank 0 computes, the others wait
        rank0_step(comm, lambda: _compute_one(console, counts_file, neighbors_file, n_nbr, output_file, config))
        return
    _compute_one(console, counts_file, neighbors_file, n_nbr, output_file, config)


# ---------------------------------------------------------------------------
# Multi-locus step (BASELINE config 5): the reference runs step 6 once per
# region, each run with that region's counts file and the SAME neighbours file
# (steps 4-5 run once per cohort).  Here the neighbours file is loaded and
# indexed once, the loci's counts go locus-minor into one [U][ldl] matrix and
# ONE launch (grid_dipcn_loci) computes every region; each locus' file is what
# the single-locus step writes for it, and a locus fails alone, as its own
# reference run would.

def neighbor_arrays(neighbors: dict, sample_scales: dict):
    """The locus-independent half of dipcn_arrays: (ids, names, scale, nbr,
    nscale, ncnt).  ``ids`` are the n neighbour-file rows, ``names`` the id
    universe (the rows first, then neighbour ids that are not rows); nbr holds
    universe indices (-1 padding)."""
    ids = list(neighbors)
    n = len(ids)
    universe = {sid: i for i, sid in enumerate(ids)}
    for lst in neighbors.values():
        for nid, _ in lst:
            if nid not in universe:
                universe[nid] = len(universe)
    k = max((len(l) for l in neighbors.values()), default=0)
    nbr = np.full((max(n, 1), max(k, 1)), -1, dtype=np.int32)
    nsc = np.zeros((max(n, 1), max(k, 1)), dtype=np.float64)
    cnt = np.zeros(max(n, 1), dtype=np.int32)
    scale = np.zeros(max(len(universe), 1), dtype=np.float64)
    for i, sid in enumerate(ids):
        lst = neighbors[sid]
        cnt[i] = len(lst)
        scale[i] = sample_scales[sid]
        if lst:
            nbr[i, :len(lst)] = [universe[nid] for nid, _ in lst]
            nsc[i, :len(lst)] = [ns for _, ns in lst]
    return ids, list(universe), scale, nbr, nsc, cnt


def loci_ld(n_loci: int) -> int:
    """Row length of the locus-minor matrix: every row starts on 64 bytes."""
    return -(-int(n_loci) // 8) * 8


def place_counts(index: pd.Index, mat: np.ndarray, col: int, reads: dict) -> None:
    """Column ``col`` of the locus-minor matrix from one locus' _read_counts
    dict: mat[index of id, col] = count for the ids of the universe, NaN (no
    count) everywhere else.  One vectorised lookup; keys that are no id of the
    universe -- other samples, or the ints pandas makes of an all-numeric id
    column -- match nothing, as ``id in reads`` finds nothing for them."""
    mat[:, col] = np.nan
    if not reads:
        return
    keys = np.empty(len(reads), dtype=object)
    keys[:] = list(reads)
    vals = np.fromiter(reads.values(), dtype=np.float64, count=len(reads))
    pos = index.get_indexer(keys)
    hit = pos >= 0
    mat[pos[hit], col] = vals[hit]


def _loci_config(config):
    """(loci, counts paths, output paths, neighbours file, n_nbr) of the loci mode."""
    from .hi_inference import _locus_path, read_loci_file
    dc = config.get("compute_diploid_genotypes", {})
    ftype = config.get("output_file_type", "tsv")
    output_dir = config.get("output_dir", ".")
    keys = dict(output_dir=output_dir, dip_prefix=dc.get("output_file_prefix", None),
                count_prefix=config["count_reads"].get("output_file_prefix", None), type=ftype)
    cnt_t = dc.get("counts_file", "{output_dir}/{count_prefix}.{locus}.{type}")
    out_t = dc.get("loci_output", "{output_dir}/{dip_prefix}.{locus}.{type}")
    zmax = config["mosdepth"]["neighbors"].get("zmax", 2.0)
    nb_prefix = config["mosdepth"]["neighbors"].get("output_file_prefix", None)
    neighbors_file = Path(f"{output_dir}/{nb_prefix}.zMax{zmax:.1f}.{ftype}.gz")
    loci = read_loci_file(dc["loci_file"])
    return (loci, [_locus_path(cnt_t, lc, **keys) for lc in loci], [_locus_path(out_t, lc, **keys) for lc in loci],
            neighbors_file, dc.get("n_nbr", 300))


def _barrier():
    """Every rank leaves the step together (step 7's table may deal the loci
    differently), when a default process group is initialised."""
    import sys
    dist = sys.modules.get("torch.distributed")
    if dist is not None and dist.is_available() and dist.is_initialized():
        dist.barrier()


def compute_diploid_genotypes_loci(config, console, comm=None, group=None):
    """Step 6 over every region of ``compute_diploid_genotypes.loci_file``.

    Per-locus inputs and outputs are path templates ({chrom} {start} {end}
    {gene} {index} {locus}; {output_dir} {dip_prefix} {count_prefix} {type}
    too):
      * ``counts_file`` (default ``{output_dir}/{count_prefix}.{locus}.{type}``,
        count_prefix = ``count_reads.output_file_prefix``),
      * ``loci_output`` (default ``{output_dir}/{dip_prefix}.{locus}.{type}``:
        step 7's default ``dip_cn_file``, so ``loci_file`` in both sections
        chains 6 -> 7).
    The neighbours file is one, shared by every locus.  Each output file is
    what the reference's step writes for that locus' counts; a locus the
    reference fails on (ZeroDivisionError, unreadable counts) is logged and
    writes no file, the others are written.  Loci are dealt ``index % world
    == rank`` over the ranks of a torch.distributed job (``comm``: as in
    hi_inference_loci) and every rank writes its own loci's files; the step
    ends with a barrier.  Returns the loci this rank wrote (dicts with their
    output paths), None on a config error."""
    try:
        loci, cnt_paths, outs, neighbors_file, n_nbr = _loci_config(config)
    except Exception as e:
        log(console, f"Config error: {e}", style="danger")
        return None
    if len(set(outs)) != len(outs):
        log(console, "Config error: loci_output names collide (add {index} or {start} to the template)",
            style="danger")
        return None
    try:
        return _compute_loci(config, console, comm, group, loci, cnt_paths, outs, neighbors_file, n_nbr)
    finally:
        _barrier()


def _locus_name(lc):
    return f"{lc['chrom']}_{lc['start']}_{lc['end']}_{lc['gene']}"


def _compute_loci(config, console, comm, group, loci, cnt_paths, outs, neighbors_file, n_nbr):
    from .hi_inference import _rank_world
    rank, world = _rank_world(comm)
    mine = [lc for lc in loci if lc["index"] % world == rank]
    log(console, f"Computing dipCN of {len(mine)} of {len(loci)} loci on rank {rank}/{world}")
    neighbors, scales = load_neighbors(neighbors_file)
    ids, names, scale, nbr, nsc, cnt = neighbor_arrays(neighbors, scales)
    n = len(ids)
    index = pd.Index(np.array(names, dtype=object), dtype=object)
    mat = np.empty((len(names), loci_ld(len(mine))), dtype=np.float64)
    mat[:, len(mine):] = np.nan
    ok = []
    for col, lc in enumerate(mine):
        try:
            place_counts(index, mat, col, _read_counts(cnt_paths[lc["index"]]))
            ok.append(True)
        except Exception as e:                  # the reference's run for this locus ends here
            mat[:, col] = np.nan
            ok.append(False)
            log(console, f"Failed to compute diploid CNV calls: {e} (locus {_locus_name(lc)})", style="danger")
    if n and mine:
        with progress_bar(console, total=len(mine), description="Computing dipCN...") as (progress, task):
            out, valid, zerodiv, missed = engine.dipcn_loci(get_device(config), mat, scale, nbr, nsc, cnt,
                                                            int(n_nbr), n, group=group)
            progress.advance(task, len(mine))
    else:
        out, valid = np.zeros((n, len(mine))), np.zeros((n, len(mine)), dtype=bool)
        zerodiv, missed = np.zeros(len(mine), dtype=bool), np.zeros(len(mine), dtype=np.int64)
    id_arr = np.empty(n, dtype=object)
    id_arr[:] = ids
    done = []
    for col, lc in enumerate(mine):
        if not ok[col]:
            continue
        if zerodiv[col]:
            log(console, f"Failed to compute diploid CNV calls: float division by zero (locus {_locus_name(lc)})",
                style="danger")
            continue
        if missed[col]:
            log(console, f"Warning: {int(missed[col])} neighbor IDs not found in read counts "
                         f"(locus {_locus_name(lc)})", style="warning")
        sel = np.flatnonzero(valid[:, col])
        df = pd.DataFrame({"Sample": id_arr[sel], "Norm_Reads": out[sel, col]}, columns=["Sample", "Norm_Reads"])
        output_file = outs[lc["index"]]
        output_file.parent.mkdir(parents=True, exist_ok=True)
        df.to_csv(output_file, sep="\t", index=False)
        done.append(dict(lc, output=str(output_file), samples=len(df)))
    log(console, f"Saved dipCN of {len(done)} loci (rank {rank})", style="success")
    return done


def _compute_one(console, counts_file, neighbors_file, n_nbr, output_file, config):
    reads = _read_counts(counts_file)
    neighbors, scales = load_neighbors(neighbors_file)
    with progress_bar(console, total=len(neighbors), description="Computing dipCN...") as (progress, task):
        rows, missing = dipcn_arrays(neighbors, scales, reads, n_nbr, get_device(config))
        progress.advance(task, len(neighbors))
    if missing:
        log(console, f"Warning: {len(missing)} neighbor IDs not found in read counts "
                     f"(showing up to 5: {list(missing)[:5]})", style="warning")
    df = pd.DataFrame(rows, columns=["Sample", "Norm_Reads"])
    df.to_csv(output_file, sep="\t", index=False)
    log(console, f"Saved {len(df)} samples → {output_file}", style="success")
