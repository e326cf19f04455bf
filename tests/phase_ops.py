"""Shared helpers of the phasing tests (tests/test_abi_cpu.py,
tests/test_phase_cases_cpu.py, tests/test_gpu_phase.py): the Python executor
of the level schedule, the oracle's result per case (computed once) and the
digests tests/golden/g8_phase.json holds."""
from __future__ import annotations

import hashlib
import json
import math
import os

import numpy as np

from oracle import steps

G8 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_phase.json")
QNAN = np.uint64(0x7FF8000000000000)


def run_levels(irr, hn, min_nbr, iters, watch=None):
    """Execute the level schedule in Python (read-all-then-write per level).
    ``watch``: called with every intermediate value of the sweep."""
    from grid_amd import _abi, engine
    off, nbr, w = engine.csr_from_lists(hn)
    order, loff, nl = _abi.hi_levels(off, nbr)
    n = len(irr)
    assert sorted(order.tolist()) == list(range(n))
    see = watch or (lambda *v: None)
    hap = [float("nan")] * (2 * n)
    for i in range(n):
        if len(hn[2 * i]) >= min_nbr and len(hn[2 * i + 1]) >= min_nbr:
            hap[2 * i] = hap[2 * i + 1] = irr[i] / 2
    for _ in range(iters):
        for l in range(nl):
            upd = []
            for e in range(loff[l], loff[l + 1]):
                i = int(order[e])
                if math.isnan(hap[2 * i]):
                    continue
                ws, wv = [1e-9, 1e-9], [0.0, 0.0]
                for h in range(2):
                    for nb, wt in hn[2 * i + h]:
                        v = hap[nb]
                        if not math.isnan(v):
                            ws[h] += wt
                            wv[h] += wt * v
                            see(wt * v, ws[h], wv[h])
                m0, m1 = wv[0] / ws[0], wv[1] / ws[1]
                see(m0, m1, m0 + m1)
                if m0 + m1 > 0:
                    see(irr[i] * m0, irr[i] * m1)
                    upd.append((i, irr[i] * m0 / (m0 + m1), irr[i] * m1 / (m0 + m1)))
            for i, a, b in upd:
                hap[2 * i], hap[2 * i + 1] = a, b
    return hap


def digest(values) -> str:
    """SHA-256 of the little-endian float64 bytes, every NaN as 0x7ff8000000000000."""
    a = np.array(values, dtype="<f8").reshape(-1)
    bits = a.view("<u8").copy()
    bits[np.isnan(a)] = QNAN
    return hashlib.sha256(bits.tobytes()).hexdigest()


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


_oracle = {}


def oracle(case):
    """(hap [2n], imp [2n], mean) of oracle.steps on a case of tests/phase_cases.py,
    computed once per case and shared by the tests (read-only arrays)."""
    if case.name not in _oracle:
        hap, mean = steps.run_phasing(case.irr, case.hn, case.min_nbr, case.iters)
        imp = [x for i in range(case.n) for x in steps.compute_imp(i, hap, case.hn, mean)]
        hap, imp = np.array(hap, dtype=np.float64), np.array(imp, dtype=np.float64).reshape(-1)
        hap.setflags(write=False)
        imp.setflags(write=False)
        _oracle[case.name] = (hap, imp, float(mean))
    return _oracle[case.name]


_golden = None


def golden():
    """{case name: record} of tests/golden/g8_phase.json."""
    global _golden
    if _golden is None:
        _golden = {r["name"]: r for r in json.load(open(G8))["cases"]}
    return _golden


def mean_hex(m: float) -> str:
    return "nan" if math.isnan(m) else float(m).hex()
