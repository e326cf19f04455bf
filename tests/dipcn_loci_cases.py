"""Shared pieces of the step-6 loci-mode tests: the g6_loci fixture (step 6 over
a loci table, pinned against the reference run once per locus), its configs,
and synthetic locus-minor kernel inputs with their per-locus oracle."""
import json
import os
import shutil

import numpy as np

G6 = os.path.join(os.path.dirname(__file__), "golden", "g6_loci")


def g6_meta():
    with open(os.path.join(G6, "config.json")) as f:
        meta = json.load(f)
    with open(os.path.join(G6, "expected", "status.json")) as f:
        meta["status"] = json.load(f)
    return meta


def g6_workdir(root):
    """A writable copy of the fixture's inputs; returns the loci-mode config."""
    out = os.path.join(str(root), "out")
    os.makedirs(out)
    for f in os.listdir(G6):
        if f.startswith(("counts.", "neighbors.")):
            shutil.copy(os.path.join(G6, f), out)
    return {"output_dir": out, "output_file_type": "tsv",
            "count_reads": {"run": False, "output_file_prefix": "counts"},
            "mosdepth": {"run": False, "normalize": {"run": False},
                         "neighbors": {"run": False, "zmax": 2.0, "output_file_prefix": "neighbors"}},
            "compute_diploid_genotypes": {"run": True, "output_file_prefix": "dipcn", "n_nbr": g6_meta()["n_nbr"],
                                          "loci_file": os.path.join(G6, "loci.txt")},
            "gpu": {"device": 0}}


def single_locus_config(cfg, name):
    """The config of one single-locus run, prefixes set as the fixture's generator sets them."""
    c = json.loads(json.dumps(cfg))
    c["count_reads"]["output_file_prefix"] = f"counts.{name}"
    c["compute_diploid_genotypes"]["output_file_prefix"] = f"dipcn.{name}"
    c["compute_diploid_genotypes"].pop("loci_file", None)
    return c


def synth(n, extra, k, n_loci, seed, p_present=0.85):
    """Kernel inputs: n rows, universe n + extra, lists of k entries with ncnt
    0..k, presence drawn per (id, locus).  Returns dict of arrays; reads is
    [U][n_loci] with NaN = absent."""
    rng = np.random.default_rng(seed)
    u = n + extra
    nbr = np.full((n, max(k, 1)), -1, np.int32)
    nsc = np.zeros((n, max(k, 1)))
    cnt = (np.arange(n) % (k + 1)).astype(np.int32)
    rng.shuffle(cnt)
    for i in range(n):
        nbr[i, :cnt[i]] = rng.choice(u, size=cnt[i], replace=False)
        nsc[i, :cnt[i]] = rng.uniform(0.7, 1.4, cnt[i])
    scale = rng.uniform(0.7, 1.4, u)
    reads = rng.integers(20, 900, (u, n_loci)).astype(np.float64)
    reads[rng.random((u, n_loci)) >= p_present] = np.nan
    return dict(n=n, u=u, reads=reads, scale=scale, nbr=nbr, nsc=nsc, cnt=cnt)


def oracle_locus(c, col, n_nbr):
    """oracle.steps.dipcn on column ``col``: (out [n], valid [n]), or
    ZeroDivisionError."""
    from oracle import steps
    n, u = c["n"], c["u"]
    rd = {j: float(c["reads"][j, col]) for j in range(u) if not np.isnan(c["reads"][j, col])}
    nbrs = {i: [(int(c["nbr"][i, t]), float(c["nsc"][i, t])) for t in range(c["cnt"][i])] for i in range(n)}
    sc = {i: float(c["scale"][i]) for i in range(n)}
    out, valid = np.zeros(n), np.zeros(n, bool)
    for i, v in steps.dipcn(nbrs, sc, rd, n_nbr):
        out[i], valid[i] = v, True
    return out, valid


def missing_ids_count(c, col, n_nbr):
    """Size of the reference's missing_ids set (compute_dipcn.py:72-77) for
    column ``col``: neighbours consulted (row has a count, fewer than n_nbr
    found so far) that have no count."""
    has = ~np.isnan(c["reads"][:, col])
    miss = np.zeros(c["u"], bool)
    for i in range(c["n"]):
        if not has[i]:
            continue
        lst = c["nbr"][i, :c["cnt"][i]]
        present = has[lst]
        before = np.cumsum(present) - present          # present neighbours before entry t
        miss[lst[(before < n_nbr) & ~present]] = True
    return int(miss.sum())


def same_bits(a, b):
    """Equal as float.hex() is: bit for bit, any NaN equal to any NaN (the sign
    of the NaN an invalid operation makes is the processor's choice)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
