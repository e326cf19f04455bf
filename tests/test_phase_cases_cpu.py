"""The phasing case table (tests/phase_cases.py) on the CPU: the oracle
reproduces the reference's digests (tests/golden/g8_phase.json), the Python
executor of the level schedule reproduces the oracle on the adversarial graph
shapes (pins grid_hi_levels), and every case reaches the edge it is named for
-- checked with the host schedule (grid_hi_levels / grid_hi_pack) and the
route query, not the kernels.  tests/test_gpu_phase.py runs the same table
through every kernel."""
import math

import numpy as np
import pytest

from grid_amd import _abi, engine
from tests import phase_cases as pc
from tests import phase_ops as po

IDS = [c.name for c in pc.CASES]
ROUTE = {"PHASE4": _abi.HI_ROUTE_PHASE4, "PH2_SPLIT_LDS": _abi.HI_ROUTE_PH2_SPLIT_LDS,
         "PH2_PAIRED_LDS": _abi.HI_ROUTE_PH2_PAIRED_LDS, "PH_LEGACY_LDS": _abi.HI_ROUTE_PH_LEGACY_LDS,
         "PH2_SPLIT_GLOBAL": _abi.HI_ROUTE_PH2_SPLIT_GLOBAL, "PH_LEGACY_GLOBAL": _abi.HI_ROUTE_PH_LEGACY_GLOBAL}
FLAG = {"default": 0, "ph2": _abi.HI_PH2, "paired": _abi.HI_PAIRED, "legacy": _abi.HI_LEGACY}

_sched = {}


def schedule(case):
    if case.name not in _sched:
        off, nbr, w = engine.csr_from_lists(case.hn)
        _sched[case.name] = (off,) + tuple(_abi.hi_schedule(off, nbr, w))
    return _sched[case.name]


def test_table_is_deterministic_and_well_formed():
    assert len(set(IDS)) == len(IDS)
    again = {c.name: c for c in pc._build()}
    for c in pc.CASES:
        assert c.facts, c.name                       # every case names the edge it exists for
        assert len(c.hn) == 2 * c.n and c.iters <= 6 and c.min_nbr >= 0
        for lst in c.hn:
            for a, wt in lst:
                assert 0 <= a < 2 * c.n and math.isfinite(wt) and wt >= 0
        if c.name in again:
            assert again[c.name].hn == c.hn
            assert np.array_equal(np.array(again[c.name].irr), np.array(c.irr), equal_nan=True)
    small = [c for c in pc.SMALL if c.n > 600]
    assert sorted(c.name for c in small) == ["chain", "div_hard", "div_sweep", "div_sweep_k8"]


@pytest.mark.parametrize("name", IDS)
def test_oracle_reproduces_the_reference_digests(name):
    case, rec = pc.BY_NAME[name], po.golden()[name]
    hap, imp, mean = po.oracle(case)
    assert rec["n"] == case.n
    assert po.mean_hex(mean) == rec["mean"]
    assert po.digest(hap) == rec["hap_sha256"]
    assert po.digest(imp) == rec["imp_sha256"]


def test_fixture_lists_exactly_the_table():
    assert sorted(po.golden()) == sorted(IDS)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.n <= 600])
def test_level_executor_equals_the_sequential_sweep(name):
    """grid_hi_levels' schedule, executed level by level in Python, is the
    oracle's sequential sweep bit for bit."""
    case = pc.BY_NAME[name]
    got = po.run_levels(case.irr, case.hn, case.min_nbr, case.iters)
    assert po.same_bits(got, po.oracle(case)[0]).all()


def _levels_of(case):
    _, order, loff, nl = schedule(case)[:4]
    lvl = np.zeros(case.n, dtype=np.int64)
    for l in range(nl):
        lvl[order[loff[l]:loff[l + 1]]] = l
    return lvl


@pytest.mark.parametrize("name", IDS)
def test_case_reaches_its_edge(name):
    case = pc.BY_NAME[name]
    f = case.facts
    off, order, loff, nl, pk_nbr, pk_w, pk_cnt, flags, max_list = schedule(case)
    widths = np.diff(loff).tolist()
    lens = np.diff(off)
    if "n" in f:
        assert case.n == f["n"]
    if "nlev" in f:
        assert nl == f["nlev"]
    for l, wd in f.get("widths", {}).items():
        assert widths[l] == wd, (l, widths[l])
    for chunk in (128, 256):
        if f"nch{chunk}" in f:
            assert pc.nch(widths, chunk) == f[f"nch{chunk}"]
        if f"odd{chunk}" in f:
            assert bool(case.iters * pc.nch(widths, chunk) % 2) == f[f"odd{chunk}"]
    if "max_list" in f:
        assert max_list == f["max_list"] == int(lens.max())
    if "has_long" in f:
        assert bool((pk_cnt[:case.n] == -1).any()) == f["has_long"]
        assert f["has_long"] == bool(lens.max() > _abi.PACK_CAP)
    if "unit" in f:
        assert bool(flags & _abi.HI_UNIT_WEIGHTS) == f["unit"]
    if "capt" in f:
        assert _abi.hi_phase_route(case.n, nl, flags, max_list)[1] == f["capt"]
        assert _abi.hi_phase_route(case.n, nl, flags, max_list, batch=True)[1] == f["capt"]
    for fl, kern in f.get("route", {}).items():
        assert _abi.hi_phase_route(case.n, nl, flags | FLAG[fl], max_list)[0] == ROUTE[kern], fl
    if "lone" in f:
        l, pos = f["lone"]
        with_list = [e - loff[l] for e in range(loff[l], loff[l + 1])
                     if lens[2 * order[e]] or lens[2 * order[e] + 1]]
        assert with_list == [pos]
        assert pos % 128 == 0 and pos == widths[l] - 1          # alone in the level's last chunk of 128
    if f.get("mixed_pair"):
        a, b = lens[0::2], lens[1::2]
        assert ((a > 16) & (b <= 16) & (b > 0)).any() and ((b > 16) & (a <= 16) & (a > 0)).any()
    if "minl_binding" in f:
        lvl = _levels_of(case)
        binding = fwd_same = back_one = 0
        for j in range(case.n):
            nb = [a >> 1 for h in range(2) for a, _ in case.hn[2 * j + h]]
            back = max([lvl[b] + 1 for b in nb if b < j], default=0)
            binding += lvl[j] > back
            fwd_same += sum(1 for b in nb if b > j and lvl[b] == lvl[j])
            back_one += sum(1 for b in nb if b < j and lvl[b] == lvl[j] - 1)
        assert binding >= f["minl_binding"] and fwd_same >= 100 and back_one >= 100, (binding, fwd_same, back_one)
    if f.get("self"):
        assert any(a == hh for hh, lst in enumerate(case.hn) for a, _ in lst)
    if f.get("sibling"):
        assert any(a == hh ^ 1 for hh, lst in enumerate(case.hn) for a, _ in lst)
    if f.get("triple"):
        assert any(max(np.bincount([a for a, _ in lst])) >= 3 for lst in case.hn if lst)
    hap, imp, mean = po.oracle(case)
    init = np.array([x / 2 for x in case.irr for _ in range(2)])
    if "phased" in f:
        assert int((~np.isnan(hap[0::2])).sum()) == f["phased"]
        if f["phased"] == 0:
            assert mean == 0.0 and (imp == 0.0).all()
    if f.get("hap_unchanged"):
        ph = ~np.isnan(hap)
        assert ph.any() and po.same_bits(hap[ph], init[ph]).all()
        assert (imp[ph] == mean / 2).all()                      # no phased neighbour: the mean/2 fallback
    if "zero_block" in f:
        a, b = f["zero_block"]
        assert po.same_bits(hap[2 * a:2 * b], init[2 * a:2 * b]).all()
        assert (hap[2 * a:2 * b] == 0).all() and np.signbit(hap[2 * a:2 * b]).any()
        assert any(x == 0 and math.copysign(1, x) < 0 for x in case.irr[:a])
        assert any(x == 0 and math.copysign(1, x) > 0 for x in case.irr[:a])
    if "list_lens" in f:
        assert set(f["list_lens"]) <= set(lens.tolist())
    if f.get("vanishing"):
        wts = {wt for lst in case.hn for _, wt in lst}
        assert {0.0, 1e-30} <= wts and 1e-9 + 1e-30 == 1e-9
        fell_back = [hh for hh, lst in enumerate(case.hn)
                     if lst and all(wt <= 1e-30 for _, wt in lst) and imp[hh] == mean / 2]
        assert len(fell_back) >= 20
        assert (~po.same_bits(hap, init)).sum() >= 20          # while the sweep divided by 1e-9 and updated
    if f.get("no_overflow"):
        seen = []
        po.run_levels(case.irr, case.hn, case.min_nbr, case.iters, watch=lambda *v: seen.extend(v))
        assert seen and all(math.isfinite(v) for v in seen)
        assert max(abs(v) for v in seen) > 1e299 and min(abs(v) for v in seen if v) < 1e-299
        assert np.isfinite(hap[~np.isnan(hap)]).all() and np.isfinite(imp).all()
        assert {1e300, 1e-300} <= set(case.irr) and min(case.irr) < 0


def test_iters0_is_the_initial_halves():
    case = pc.BY_NAME["iters0"]
    hap, imp, _ = po.oracle(case)
    init = np.array([x / 2 for x in case.irr for _ in range(2)])
    ph = ~np.isnan(hap)
    assert po.same_bits(hap[ph], init[ph]).all() and case.iters == 0


def test_nan_irr_is_listed_and_spreads_to_the_mean():
    case = pc.BY_NAME["nan_irr"]
    bad = [i for i, x in enumerate(case.irr) if math.isnan(x)]
    assert len(bad) == 1 and len(case.hn[2 * bad[0]]) >= 1 and len(case.hn[2 * bad[0] + 1]) >= 1
    assert sum(1 for lst in case.hn for a, _ in lst if a >> 1 == bad[0]) >= 6
    assert math.isnan(po.oracle(case)[2])


def test_min_nbr_cases_share_one_graph():
    a, b, c = (pc.BY_NAME[f"min_nbr_{m}"] for m in (0, 1, 2))
    assert a.hn == b.hn == c.hn and a.irr == b.irr == c.irr and (a.min_nbr, b.min_nbr, c.min_nbr) == (0, 1, 2)
    ph = [int((~np.isnan(po.oracle(x)[0])).sum()) for x in (a, b, c)]
    assert ph[0] > ph[1] > ph[2] > 0


def test_len_cases_sit_on_both_sides_of_each_threshold():
    for u in "uw":
        for L, capt, long in ((8, 8, False), (9, 16, False), (16, 16, False), (17, 16, True)):
            f = pc.BY_NAME[f"len_{L}_{u}"].facts
            assert (f["max_list"], f["capt"], f["has_long"], f["unit"]) == (L, capt, long, u == "u")


LO, HI = float.fromhex("0x1p-500"), float.fromhex("0x1p500")


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.facts.get("division")])
def test_division_cases_cover_the_reciprocal_window(name):
    """From the inputs alone (one sweep, every neighbour a later sample with
    empty lists, so a probe reads exactly irr[j] / 2): the sums sv that
    k_phase4 divides lie below, inside and above its window [2^-500, 2^500]
    and on each edge, at every number of summed neighbours.  A list of k = 0
    neighbours has sv == 0 exactly, which the kernel sends through the
    reciprocal branch, so k = 0 counts as inside; it occurs beside a list
    below and a list above the window too."""
    case = pc.BY_NAME[name]
    f = case.facts
    assert case.iters == 1 and case.min_nbr == 0 and f["unit"]
    probes = [i for i in range(case.n) if case.hn[2 * i] or case.hn[2 * i + 1]]
    for i in probes:
        assert 0.5 <= case.irr[i] < 2
        for h in range(2):
            for a, wt in case.hn[2 * i + h]:
                assert a >> 1 > i and not case.hn[a] and not case.hn[a ^ 1] and wt == 1.0
    region = {"below": {}, "inside": {}, "above": {}, "negative": {}}
    exact = {}
    beside = set()
    for i in probes:
        rs = []
        for h in range(2):
            sv = 0.0
            for a, _ in case.hn[2 * i + h]:
                sv = sv + case.irr[a >> 1] / 2
            k = len(case.hn[2 * i + h])
            r = ("negative" if sv < 0 else "inside" if sv == 0 or LO <= sv <= HI else "below" if sv < LO
                 else "above")
            region[r][(h, k)] = region[r].get((h, k), 0) + 1
            exact.setdefault(k, set()).add(float(sv).hex())
            rs.append((r, k))
        for (r, k), (r2, _) in (rs, rs[::-1]):
            if k == 0:
                beside.add(r2)
    for k, vals in f.get("sv_exact", {}).items():
        assert set(vals) <= exact.get(k, set()), (k, sorted(set(vals) - exact.get(k, set())))
    if name.startswith("div_sweep"):
        ks = range(f["kmax"] + 1)
        for h in range(2):
            assert all((h, k) in region["inside"] for k in ks)
            assert all((h, k) in region["below"] and (h, k) in region["above"] for k in ks if k)
        assert {"below", "above"} <= beside
        total = {r: sum(v.values()) for r, v in region.items()}
        assert min(total["below"], total["inside"], total["above"]) >= 100, total
        if name == "div_sweep":
            assert len(probes) >= 1000 and case.n - len(probes) >= 2000
    elif "hard" in f:
        from fractions import Fraction
        dens, u = [1e-9], 1e-9
        for _ in range(16):
            u = u + 1.0
            dens.append(u)
        for h in range(2):
            assert sorted(k for hh, k in region["inside"] if hh == h) == list(range(1, 17))
        for i in probes:
            for h in range(2):
                sv, k = 0.0, len(case.hn[2 * i + h])
                for a, _ in case.hn[2 * i + h]:
                    sv = sv + case.irr[a >> 1] / 2
                q = Fraction(sv) / Fraction(dens[k])
                ulp = Fraction(2) ** (math.floor(math.log2(q)) - 52)
                assert abs(q / ulp % 1 - Fraction(1, 2)) < f["hard"], (i, h, k)
    else:
        assert region["negative"] and region["below"] and region["above"] and region["inside"]
    # nothing overflows in the reference: every result is finite
    hap, imp, _ = po.oracle(case)
    assert np.isfinite(hap).all() and np.isfinite(imp).all()
    # and the probes did move: the sweep's one division per haplotype is what the result holds
    init = np.array([x / 2 for x in case.irr for _ in range(2)])
    moved = sum(1 for i in probes if not po.same_bits(hap[2 * i:2 * i + 2], init[2 * i:2 * i + 2]).all())
    assert moved >= len(probes) // 2


def test_capacity_constants():
    """The capacity sizes of the table are the thresholds of the route query."""
    R = lambda n, nlev, fl=0: _abi.hi_phase_route(n, nlev, fl, 4)[0]
    P4, S2 = _abi.HI_ROUTE_PHASE4, _abi.HI_ROUTE_PH2_SPLIT_LDS
    assert R(pc.PHASE4_MAX_3LEV, 3) == P4 and R(pc.PHASE4_MAX_3LEV + 1, 3) == S2
    assert all(R(n, 3) == P4 for n in range(1, pc.PHASE4_MAX_3LEV, 97))
    # band_ph2: the first n of a 600-level graph that k_phase4 cannot hold, and k_phase2 can
    assert R(pc.BAND_N - 1, pc.BAND_CHAIN) == P4 and R(pc.BAND_N, pc.BAND_CHAIN) == S2
    # the band widens with the level count
    band = lambda nlev: sum(1 for n in range(3000, 5000) if R(n, nlev) == S2)
    assert band(3) < band(600) < band(1200)
    assert R(pc.CHAIN_N, pc.CHAIN_N) == P4
    assert R(pc.GLOBAL_N, 30) == _abi.HI_ROUTE_PH2_SPLIT_GLOBAL
    assert R(pc.GLOBAL_N, 30, _abi.HI_LEGACY) == R(pc.GLOBAL_N, 30, _abi.HI_PAIRED) == _abi.HI_ROUTE_PH_LEGACY_GLOBAL
    # the batch launch has no k_phase4 and takes the same thresholds otherwise
    B = lambda n, nlev, fl=0: _abi.hi_phase_route(n, nlev, fl, 4, batch=True)[0]
    assert B(100, 3) == B(100, 3, _abi.HI_PH2) == S2 and B(100, 3, _abi.HI_PAIRED) == _abi.HI_ROUTE_PH2_PAIRED_LDS
    assert B(100, 3, _abi.HI_LEGACY) == _abi.HI_ROUTE_PH_LEGACY_LDS
    assert B(pc.GLOBAL_N, 30) == _abi.HI_ROUTE_PH2_SPLIT_GLOBAL
    assert B(pc.GLOBAL_N, 30, _abi.HI_PAIRED) == _abi.HI_ROUTE_PH_LEGACY_GLOBAL
    # CAPT follows the longest list; the legacy kernels have none
    assert [_abi.hi_phase_route(100, 3, 0, m)[1] for m in (0, 8, 9, 16, 17, 40)] == [8, 8, 16, 16, 16, 16]
    assert _abi.hi_phase_route(100, 3, _abi.HI_LEGACY, 9)[1] == 0
    with pytest.raises(_abi.GridNativeError):
        _abi.hi_phase_route(-1, 3, 0, 4)


def test_table_covers_every_kernel():
    """The single-locus launches of tests/test_gpu_phase.py (every case under
    every flag, each asserted there before it runs) hold: a default-flag
    k_phase2 launch, every register kernel at CAPT 8 and 16 in unit and
    weighted form, hap in LDS and in global memory, and both legacy kernels."""
    seen = set()
    for case in pc.CASES:
        _, _, _, nl, _, _, _, flags, max_list = schedule(case)
        for fl, bit in FLAG.items():
            kern, capt = _abi.hi_phase_route(case.n, nl, flags | bit, max_list)
            seen.add((fl == "default", kern, capt, bool(flags & _abi.HI_UNIT_WEIGHTS)))
    for unit in (True, False):
        for capt in (8, 16):
            for kern in (_abi.HI_ROUTE_PHASE4, _abi.HI_ROUTE_PH2_SPLIT_GLOBAL):
                assert (True, kern, capt, unit) in seen, (kern, capt, unit)
            for kern in (_abi.HI_ROUTE_PH2_SPLIT_LDS, _abi.HI_ROUTE_PH2_PAIRED_LDS):
                assert (False, kern, capt, unit) in seen, (kern, capt, unit)
        for kern in (_abi.HI_ROUTE_PH_LEGACY_LDS, _abi.HI_ROUTE_PH_LEGACY_GLOBAL):
            assert (False, kern, 0, unit) in seen, (kern, unit)
    assert any(d and k == _abi.HI_ROUTE_PH2_SPLIT_LDS for d, k, _, _ in seen)      # band_ph2, no flag


def test_abi_names_the_ph2_flag_and_routes_as_the_header_does():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "grid_abi.h")).read()
    assert int(re.search(r"#define GRID_HI_PH2 (\d+)", txt).group(1)) == _abi.HI_PH2 == 8
    for nm, val in ROUTE.items():
        assert int(re.search(rf"GRID_HI_ROUTE_{nm} = (\d+)", txt).group(1)) == val
