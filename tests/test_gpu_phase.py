"""Every case of tests/phase_cases.py through every phasing kernel
(grid_amd/csrc/dipcn_phase.hip), bit for bit against the oracle's sequential
sweep and against the reference's digests (tests/golden/g8_phase.json).

Before each launch the route query (grid_hi_phase_route /
grid_hi_phase_batch_route, the function the launch itself calls) must name
the kernel the parametrisation is about, so a threshold change cannot turn a
k_phase2 test into a second k_phase4 test unnoticed.
tests/test_phase_cases_cpu.py checks that each case reaches its edge and that
the table's launches cover every kernel at both capacities and weight forms."""
import numpy as np
import pytest

from grid_amd import _abi, engine
from tests import phase_cases as pc
from tests import phase_ops as po

pytestmark = pytest.mark.gpu

KERNEL = {_abi.HI_ROUTE_PHASE4: "PHASE4", _abi.HI_ROUTE_PH2_SPLIT_LDS: "PH2_SPLIT_LDS",
          _abi.HI_ROUTE_PH2_PAIRED_LDS: "PH2_PAIRED_LDS", _abi.HI_ROUTE_PH_LEGACY_LDS: "PH_LEGACY_LDS",
          _abi.HI_ROUTE_PH2_SPLIT_GLOBAL: "PH2_SPLIT_GLOBAL", _abi.HI_ROUTE_PH_LEGACY_GLOBAL: "PH_LEGACY_GLOBAL"}
FLAG = {"default": 0, "ph2": _abi.HI_PH2, "paired": _abi.HI_PAIRED, "legacy": _abi.HI_LEGACY}
# what each flag runs on a locus that fits LDS with room to spare (every small case)
SMALL_ROUTE = {"default": "PHASE4", "ph2": "PH2_SPLIT_LDS", "paired": "PH2_PAIRED_LDS", "legacy": "PH_LEGACY_LDS"}



@pytest.fixture(scope="module")
def dev():
    d = _abi.Device(0)
    yield d
    d.close()


def check(case, got, where):
    """hap, imp and mean equal the oracle's bit for bit (NaN equal to NaN) and
    the reference's digests; a mismatch names its first index."""
    hap, imp, mean = got
    ehap, eimp, emean = po.oracle(case)
    for what, g, e in (("hap", hap, ehap), ("imp", imp, eimp)):
        assert len(g) == len(e) == 2 * case.n
        ok = po.same_bits(g, e)
        if not ok.all():
            k = int(np.argmin(ok))
            i = k >> 1
            off, nbr, w = engine.csr_from_lists(case.hn)
            order, loff, nl = _abi.hi_levels(off, nbr)
            e_at = int(np.nonzero(order == i)[0][0])
            lvl = int(np.searchsorted(loff, e_at, side="right") - 1)
            pytest.fail(f"{case.name} {where}: {what}[{k}] = {float(g[k]).hex()}, expected {float(e[k]).hex()} "
                        f"({int((~ok).sum())} differ); sample {i} haplotype {k & 1}, schedule entry {e_at} "
                        f"(level {lvl} of {nl}, position {e_at - int(loff[lvl])} of "
                        f"{int(loff[lvl + 1] - loff[lvl])}), lists {len(case.hn[2 * i])} / {len(case.hn[2 * i + 1])}")
    assert po.same_bits([mean], [emean]).all(), (case.name, where, float(mean).hex(), float(emean).hex())
    rec = po.golden()[case.name]
    assert po.digest(hap) == rec["hap_sha256"] and po.digest(imp) == rec["imp_sha256"]
    assert po.mean_hex(mean) == rec["mean"]


def expected_kernel(case, flag):
    return case.facts.get("route", {}).get(flag, SMALL_ROUTE[flag] if case.n < 3500 else None)


@pytest.mark.parametrize("flag", list(FLAG))
@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_single_locus(dev, name, flag):
    """grid_hi_phase (engine.phase): default, ph2, paired and legacy."""
    case = pc.BY_NAME[name]
    want = expected_kernel(case, flag)
    assert want is not None, "a capacity case names its route under every flag"
    off, nbr, w = engine.csr_from_lists(case.hn)
    _, _, nl, _, _, _, flags, max_list = _abi.hi_schedule(off, nbr, w)
    kern, capt = _abi.hi_phase_route(case.n, nl, flags | FLAG[flag], max_list)
    assert KERNEL[kern] == want, f"{name} {flag}: the launch would run {KERNEL[kern]}"
    if "capt" in case.facts and capt:
        assert capt == case.facts["capt"]
    got = engine.phase(dev, np.array(case.irr, dtype=np.float64), off, nbr, w, case.min_nbr, case.iters,
                       **({flag: True} if flag != "default" else {}))
    check(case, got, f"{flag} ({want}, CAPT {capt})")


def test_band_ph2_runs_k_phase2_by_default():
    case = pc.BY_NAME["band_ph2"]
    off, nbr, w = engine.csr_from_lists(case.hn)
    _, _, nl, _, _, _, flags, max_list = _abi.hi_schedule(off, nbr, w)
    assert KERNEL[_abi.hi_phase_route(case.n, nl, flags, max_list)[0]] == "PH2_SPLIT_LDS"
    assert KERNEL[_abi.hi_phase_route(pc.GLOBAL_N, 1, 0, 4)[0]] == "PH2_SPLIT_GLOBAL"


# ------------------------------------------------------------- batches --
def _unit(c):
    return all(wt == 1.0 for lst in c.hn for _, wt in lst)


def _maxlen(c):
    return max(len(lst) for lst in c.hn)


GROUPS = {}
for _c in pc.SMALL:
    GROUPS.setdefault((_c.min_nbr, _c.iters), []).append(_c.name)
BATCHES = {f"min{m}_it{it}": names for (m, it), names in sorted(GROUPS.items())}
# the whole batch on the global-memory kernels: one locus too large for LDS among the others
BATCHES["min1_it3_global"] = GROUPS[(1, 3)] + ["global_5200"]
# CAPT 16 for loci whose lists are all <= 8 long: one 17-long list in the batch
BATCHES["short_lists_and_one_17"] = ["len_8_u", "len_8_w", "min_nbr_1", "nan_irr", "vanishing_weights", "len_17_u"]
BATCHES["unit_only_short"] = ["len_8_u", "min_nbr_1", "nan_irr"]


def test_batches_hold_the_named_mixes():
    assert all(_unit(pc.BY_NAME[n]) for n in BATCHES["min0_it1"]) and len(BATCHES["min0_it1"]) >= 4
    mixed = [_unit(pc.BY_NAME[n]) for n in BATCHES["min1_it3"]]
    assert any(mixed) and not all(mixed)
    short = BATCHES["short_lists_and_one_17"]
    assert [_maxlen(pc.BY_NAME[n]) <= 8 for n in short] == [True] * (len(short) - 1) + [False]
    assert _maxlen(pc.BY_NAME[short[-1]]) == 17
    assert all(_maxlen(pc.BY_NAME[n]) <= 8 and _unit(pc.BY_NAME[n]) for n in BATCHES["unit_only_short"])
    assert sorted(n for names in GROUPS.values() for n in names) == sorted(c.name for c in pc.SMALL)


@pytest.mark.parametrize("paired", [False, True], ids=["default", "paired"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_batch(dev, batch, paired):
    """grid_hi_pack_batch + grid_hi_phase_batch (hi_inference.run_phasing_batch):
    one workgroup per locus, the lists packed on the device."""
    from grid_amd.utils.hi_inference import run_phasing_batch
    cases = [pc.BY_NAME[n] for n in BATCHES[batch]]
    assert len({(c.min_nbr, c.iters) for c in cases}) == 1 and len(cases) <= 200      # one launch
    sched = [_abi.hi_schedule(*engine.csr_from_lists(c.hn)) for c in cases]
    flags = _abi.HI_UNIT_WEIGHTS if all(s[6] for s in sched) else 0
    max_n, max_nlev, max_list = max(c.n for c in cases), max(s[2] for s in sched), max(s[7] for s in sched)
    kern, capt = _abi.hi_phase_route(max_n, max_nlev, flags | (_abi.HI_PAIRED if paired else 0), max_list,
                                     batch=True)
    big = max_n >= pc.GLOBAL_N
    want = (("PH_LEGACY_GLOBAL" if paired else "PH2_SPLIT_GLOBAL") if big
            else ("PH2_PAIRED_LDS" if paired else "PH2_SPLIT_LDS"))
    assert KERNEL[kern] == want
    if batch == "short_lists_and_one_17":
        assert capt == 16
    if batch == "unit_only_short":
        assert capt == 8 and flags
    got = run_phasing_batch([c.irr for c in cases], [c.hn for c in cases], cases[0].min_nbr, cases[0].iters,
                            dev=dev, paired=paired)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        check(c, g, f"batch {batch} ({want}, CAPT {capt})")
