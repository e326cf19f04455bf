"""Hand-built phasing graphs at the edges of the level-schedule kernels
(grid_amd/csrc/dipcn_phase.hip: k_phase4, k_phase2 split / paired / global,
k_phase) -- the case table of step 7.

Pure NumPy / Python, deterministic, no import of the library.  A case is a
``Case``: ``irr`` (list of float), ``hn`` (2n lists of (hap index, weight)),
``min_nbr``, ``iters`` and ``facts``: the edge the case exists for, as data.
tests/test_phase_cases_cpu.py checks every fact with the host schedule
(grid_hi_levels / grid_hi_pack) and the route query, so a case that misses
its edge fails there; tests/test_gpu_phase.py runs every case through every
kernel; tests/golden/g8_phase.json holds the reference's results.

Every input is one the reference accepts: neighbour indices in [0, 2n),
finite weights >= 0.

Facts (all optional, each checked when present):
  nlev          number of levels of the schedule
  widths        {level: entries}
  nch128/nch256 chunks of one sweep at 128 (k_phase4) / 256 (k_phase2, k_phase)
                entries per chunk; ``odd128`` / ``odd256``: parity of iters * nch
  max_list      longest list; ``has_long``: a list longer than the packed 16
  unit          every weight is 1.0 (GRID_HI_UNIT_WEIGHTS)
  lone          (level, position): the only entry of that level with a list
  mixed_pair    a sample with one list > 16 and one <= 16, both orders
  route         {flag name: kernel name} of grid_hi_phase_route
  division      the case is checked by the sv-window census (unit weights,
                one sweep, sources with empty lists); ``sv_exact``: {list
                length: sums that must occur exactly}
  hard          every probe's quotient sv / (1e-9 + k) lies within this many
                ulps of the midpoint of two doubles
  capt          the register capacity (8 / 16) of the default launch
  minl_binding  at least this many samples whose level is set by an earlier
                sample that lists them (the minl rule of grid_hi_levels)
  self/sibling/triple   lists holding the own haplotype, the sample's other
                haplotype, one neighbour three times
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

NAN = float("nan")


@dataclass
class Case:
    name: str
    irr: list
    hn: list
    min_nbr: int
    iters: int
    facts: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.irr)


# Capacity sizes, found with grid_hi_phase_route and asserted in
# tests/test_phase_cases_cpu.py::test_capacity_constants (120 KiB of LDS):
CHAIN_N = 2001           # chain: nlev == n, still k_phase4
BAND_CHAIN = 600         # band_ph2: a 600-level chain ...
BAND_N = 4413            # ... padded to the first n whose k_phase4 table no longer fits (k_phase2's does)
PHASE4_MAX_3LEV = 4887   # the largest n of a 3-level graph that k_phase4 holds
GLOBAL_N = 5200          # 3n doubles do not fit LDS: hap in global memory


def _irr(rng, n, lo=0.1, hi=4.0):
    return [float(x) for x in rng.uniform(lo, hi, n)]


def _wt(rng, weighted):
    return float(rng.uniform(0.05, 1.0)) if weighted else 1.0


def layered(rng, widths, klo, khi, weighted=False, exact=None):
    """A graph whose level l has exactly widths[l] samples (samples in level
    order).  A sample of level l lists samples of lower levels, later samples
    (which the schedule may not move before it) and itself; from level 1 on,
    its first list starts with a sample of level l - 1.  ``exact``: every
    ``exact``-th list has exactly khi entries."""
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    n = int(starts[-1])
    hn = []
    for l in range(len(widths)):
        for i in range(starts[l], starts[l + 1]):
            for h in range(2):
                k = int(rng.integers(klo, khi + 1))
                if exact and (2 * i + h) % exact == 0:
                    k = khi
                lst = []
                for _ in range(k):
                    r = int(rng.integers(0, 4))
                    if r == 0 and l > 0:
                        j = int(rng.integers(0, starts[l]))
                    elif r == 3 or i + 1 >= n:
                        j = i
                    else:
                        j = int(rng.integers(i + 1, n))
                    lst.append((2 * j + int(rng.integers(0, 2)), _wt(rng, weighted)))
                if l > 0 and h == 0:
                    first = (2 * int(rng.integers(starts[l - 1], starts[l])) + int(rng.integers(0, 2)),
                             _wt(rng, weighted))
                    if lst:
                        lst[0] = first
                    else:
                        lst.append(first)
                hn.append(lst)
    return hn


def random_graph(rng, n, klo, khi, weighted=False, exact=None, window=None):
    """Lists of klo..khi neighbours anywhere in [0, 2n) (``window``: within
    +-window samples).  ``exact``: every ``exact``-th list has khi entries."""
    hn = []
    for hh in range(2 * n):
        k = int(rng.integers(klo, khi + 1))
        if exact and hh % exact == 0:
            k = khi
        lst = []
        for _ in range(k):
            if window:
                i = hh // 2
                j = int(rng.integers(max(0, i - window), min(n, i + window + 1)))
                lst.append((2 * j + int(rng.integers(0, 2)), _wt(rng, weighted)))
            else:
                lst.append((int(rng.integers(0, 2 * n)), _wt(rng, weighted)))
        hn.append(lst)
    return hn


def nch(widths, chunk):
    return int(sum(-(-w // chunk) for w in widths))


def pad(case: Case, n: int, name: str | None = None, **facts) -> Case:
    """``case`` followed by isolated samples (empty lists) up to n samples."""
    assert n >= case.n
    rng = np.random.default_rng(n)
    extra = n - case.n
    facts = {**{k: v for k, v in case.facts.items() if k in ("unit", "max_list", "has_long", "capt")}, **facts}
    return Case(name or f"{case.name}_pad{n}", list(case.irr) + _irr(rng, extra, 0.5, 3.0),
                [list(l) for l in case.hn] + [[] for _ in range(2 * extra)], case.min_nbr, case.iters, facts)


# ------------------------------------------------------------- division --
# the bands of 2^e * [1, 2) the sources of div_sweep come from: below, on the
# edges of, inside and above k_phase4's reciprocal window [2^-500, 2^500]
DIV_BANDS = ([-520, -515, -510, -506, -503, -502, -501] + [-500, -499]
             + [-480, -400, -300, -200, -100, -50, -10, -1, 0, 1, 10, 50, 100, 200, 300, 400, 480]
             + [498, 499, 500] + [501, 502, 503, 506, 510, 515, 520])
DIV_SRC_PER_BAND = 56


def div_sweep(name, kmax, seed):
    """Probes (low indices) with two unit-weight lists of k0, k1 sources (high
    indices, empty lists, min_nbr 0): after the one sweep a probe has read
    exactly irr[j] / 2 of its sources.  Both lists draw from one band."""
    rng = np.random.default_rng(seed)
    nb = len(DIV_BANDS)
    combos = (kmax + 1) * nb
    nprobe = 2 * combos
    nsrc = nb * DIV_SRC_PER_BAND
    irr = _irr(rng, nprobe, 0.5, 2.0)
    for b in DIV_BANDS:
        for _ in range(DIV_SRC_PER_BAND):
            m = float(rng.uniform(1.0, 2.0))
            irr.append(float(np.ldexp(m, b + 1)))           # hap = irr / 2 = 2^b * m
    hn = []
    for p in range(nprobe):
        q = p % combos
        ka, band = q % (kmax + 1), q // (kmax + 1)          # every (k, band) pair, once per haplotype
        kb = int(rng.integers(0, kmax + 1))
        k0, k1 = (ka, kb) if p < combos else (kb, ka)
        base = nprobe + band * DIV_SRC_PER_BAND
        for k in (k0, k1):
            src = rng.choice(DIV_SRC_PER_BAND, size=k, replace=False)
            hn.append([(2 * (base + int(s)) + int(rng.integers(0, 2)), 1.0) for s in src])
    hn += [[] for _ in range(2 * nsrc)]
    return Case(name, irr, hn, 0, 1, dict(division=True, unit=True, nlev=1, max_list=kmax, has_long=False,
                                          route={"default": "PHASE4"}, capt=8 if kmax <= 8 else 16, kmax=kmax))


def div_window_edges(name, with16):
    """Lists whose one-sweep sum sv is exactly 2^-500, the double before it,
    2^500, the double after it, +0.0, a negative value and a subnormal: from a
    single neighbour, and (``with16``) from 16 neighbours."""
    lo, hi = float.fromhex("0x1p-500"), float.fromhex("0x1p500")
    lo_pred, hi_succ = float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, np.inf))
    sub = float.fromhex("0x0.0000000000123p-1022")
    singles = [lo, lo_pred, hi, hi_succ, 0.0, -1.5, sub, float.fromhex("0x1.8p-500"), float.fromhex("0x1.8p499")]
    groups = [[v] for v in singles]
    partners = [v * 1.25 if abs(v) > 1e-300 or v == 0 else 1e-320 for v in singles]
    partners[4], partners[5] = 3.0, 2.0
    if with16:
        l4, h4 = float.fromhex("0x1p-504"), float.fromhex("0x1p496")
        groups += [[l4] * 16, [l4] * 15 + [l4 - float.fromhex("0x1p-553")], [h4] * 16,
                   [h4] * 15 + [h4 + float.fromhex("0x1p448")], [0.0] * 16, [-0.25] * 15 + [3.75]]
        partners += [lo * 1.25, lo * 1.25, hi * 0.75, hi * 0.75, 1.0, 1.0]
    rng = np.random.default_rng(77)
    nprobe = 2 * len(groups)
    irr = _irr(rng, nprobe, 0.5, 1.9)
    hn = [[] for _ in range(2 * nprobe)]

    def source(v):
        irr.append(2.0 * v)                                  # exact, also for the subnormal
        hn.extend([[], []])
        return 2 * (len(irr) - 1) + (len(irr) & 1)

    sums = []
    for g, (vals, pv) in enumerate(zip(groups, partners)):
        for flip in range(2):
            p = 2 * g + flip
            hn[2 * p + flip] = [(source(v), 1.0) for v in vals]
            hn[2 * p + 1 - flip] = [(source(pv), 1.0)]
            sums.append((2 * p + flip, vals))
    want1 = [lo, lo_pred, hi, hi_succ, 0.0, -1.5, sub]
    want16 = [lo, lo_pred, hi, hi_succ, 0.0] if with16 else []
    return Case(name, irr, hn, 0, 1, dict(division=True, unit=True, nlev=1, max_list=16 if with16 else 1,
                                          has_long=False, route={"default": "PHASE4"}, capt=16 if with16 else 8,
                                          sv_exact={1: [v.hex() for v in want1], 16: [v.hex() for v in want16]},
                                          kmax=16 if with16 else 1))


def hard_numerators(b, deltas=(1, -1, 3, -3, 5, -5)):
    """Doubles a in [1, 2) whose quotient a / b lies next to the midpoint of
    two doubles, as near as a 53-bit a allows: with a = A 2^-52 and b = B 2^e,
    A 2^S = B M + delta for an odd 54-bit M and a small delta (S = 53: a >= b's
    mantissa, 54: below it).  The division that rounds these correctly has
    about 2^-100 of relative slack; a reciprocal one ulp off does not."""
    import math
    mb, _ = math.frexp(b)
    B = int(mb * 2 ** 53)
    t = (B & -B).bit_length() - 1                            # B = Bo 2^t, Bo odd: delta is a multiple of 2^t
    Bo = B >> t
    out = []
    for S in (53, 54):
        mod = 1 << (S - t)
        inv = pow(Bo, -1, mod)
        for d in deltas:
            M = (-d * inv) % mod
            while M < 1 << 54:
                if M >= 1 << 53 and M % 2:
                    A = (Bo * M + d) // mod
                    if 1 << 52 <= A < 1 << 53:
                        out.append(float(A) * 2.0 ** -52)
                        break
                M += mod
    return out


def div_hard():
    """div_sweep's layout with numerators chosen against each of k_phase4's
    sixteen unit denominators 1e-9 + k: haplotype 0 sums k sources to a
    hard_numerators value of that denominator, haplotype 1 sums 17 - k."""
    rng = np.random.default_rng(53)
    dens, u = {}, 1e-9
    for k in range(1, 17):
        u = u + 1.0
        dens[k] = hard_numerators(u)
    probes = [(k, t) for k in range(1, 17) for t in range(len(dens[k]))]
    irr = _irr(rng, len(probes), 0.5, 2.0)
    hn = [[] for _ in range(2 * len(probes))]
    c = 2.0 ** -8

    def sources(a, k):                                       # k values whose sequential sum is a, exactly
        vals = [a - (k - 1) * c] + [c] * (k - 1)
        lst = []
        for v in vals:
            irr.append(2.0 * v)
            hn.extend([[], []])
            lst.append((2 * (len(irr) - 1) + (len(irr) & 1), 1.0))
        return lst

    for p, (k, t) in enumerate(probes):
        k1 = 17 - k
        hn[2 * p] = sources(dens[k][t], k)
        hn[2 * p + 1] = sources(dens[k1][t % len(dens[k1])], k1)
    return Case("div_hard", irr, hn, 0, 1, dict(division=True, unit=True, nlev=1, max_list=16, has_long=False,
                                               route={"default": "PHASE4"}, capt=16, kmax=16, hard=2.0 ** -40))


# ----------------------------------------------------- loop and geometry --
def _geom(name, widths, iters, seed, klo=1, khi=6, min_nbr=1, **facts):
    rng = np.random.default_rng(seed)
    n = int(sum(widths))
    c128, c256 = nch(widths, 128), nch(widths, 256)
    f = dict(nlev=len(widths), widths=dict(enumerate(widths)), nch128=c128, nch256=c256,
             odd128=bool(iters * c128 % 2), odd256=bool(iters * c256 % 2), unit=True)
    f.update(facts)
    return Case(name, _irr(rng, n), layered(rng, widths, klo, khi), min_nbr, iters, f)


def last_lane_only(name, long):
    """A level of 129 entries (then a second level that reads it); of the 129
    only the last has lists, so one lane sets its chunk's segment count."""
    rng = np.random.default_rng(129 + long)
    n = 129 + 20
    hn = [[] for _ in range(2 * n)]
    fwd = lambda k: [(2 * int(rng.integers(129, n)) + int(rng.integers(0, 2)), 1.0) for _ in range(k)]
    hn[2 * 128] = fwd(17 if long else 5) + [(2 * 128, 1.0)]
    hn[2 * 128 + 1] = fwd(3)
    for i in range(129, n):
        for h in range(2):
            hn[2 * i + h] = [(2 * int(rng.integers(0, 129)) + int(rng.integers(0, 2)), 1.0)
                             for _ in range(int(rng.integers(1, 5)))]
        hn[2 * i][0] = (2 * 128 + (i & 1), 1.0)
    return Case(name, _irr(rng, n), hn, 0, 2,
                dict(nlev=2, widths={0: 129, 1: 20}, nch128=3, nch256=2, lone=(0, 128), unit=True,
                     max_list=18 if long else 6, has_long=bool(long)))


# ---------------------------------------------------------- graph shape --
def chain(n, name="chain", iters=2):
    """Sample i lists sample i - 1: one level per sample."""
    rng = np.random.default_rng(n)
    hn = [[], []]
    for i in range(1, n):
        hn.append([(2 * (i - 1), 1.0)])
        hn.append([(2 * (i - 1) + 1, 1.0), (2 * (i - 1), 1.0)])
    return Case(name, _irr(rng, n), hn, 0, iters,
                dict(nlev=n, nch128=n, nch256=n, unit=True, max_list=2 if n > 1 else 0, has_long=False))


def self_and_sibling():
    rng = np.random.default_rng(61)
    n = 61
    hn = random_graph(rng, n, 1, 5)
    for i in range(n):
        for h in range(2):
            hh = 2 * i + h
            if i % 3 == 0:
                hn[hh].append((hh, 1.0))
            if i % 3 == 1:
                hn[hh].insert(0, (hh ^ 1, 1.0))
            if i % 4 == 2:
                t = int(rng.integers(0, 2 * n))
                hn[hh] += [(t, 1.0)] * 3
    return Case("self_and_sibling", _irr(rng, n), hn, 1, 4, dict(self=True, sibling=True, triple=True, unit=True))


def forward_same_level(weighted=False):
    rng = np.random.default_rng(240 + weighted)
    n = 241
    hn = random_graph(rng, n, 2, 7, weighted, window=12)
    return Case("forward_same_level" + ("_w" if weighted else ""), _irr(rng, n), hn, 1, 4,
                dict(minl_binding=20, unit=not weighted))


def odd_n(n):
    rng = np.random.default_rng(1000 + n)
    hn = random_graph(rng, n, 0, 10, weighted=bool(n % 4 == 1))
    return Case(f"odd_n_{n}", _irr(rng, n), hn, 1, 3, dict(n=n))


# --------------------------------------------------------- list lengths --
def len_case(L, weighted):
    rng = np.random.default_rng(10 * L + weighted)
    n = 151
    hn = random_graph(rng, n, 1, L, weighted, exact=7)
    return Case(f"len_{L}_{'w' if weighted else 'u'}", _irr(rng, n), hn, 1, 3,
                dict(max_list=L, has_long=L > 16, unit=not weighted, capt=8 if L <= 8 else 16))


def long_short_pair(weighted):
    rng = np.random.default_rng(170 + weighted)
    n = 121
    hn = random_graph(rng, n, 1, 16, weighted)
    unph = [5, 40, 77, 100]
    for i in unph:
        hn[2 * i] = []                                       # unphased at min_nbr 1: NaN haplotypes
    some = lambda k: [(int(rng.integers(0, 2 * n)), _wt(rng, weighted)) for _ in range(k)]
    for t, i in enumerate(range(3, n, 9)):
        if i in unph:
            continue
        a, b = some(int(rng.integers(17, 26))), some(3)
        hn[2 * i], hn[2 * i + 1] = (a, b) if t % 2 == 0 else (b, a)
    hn[2 * 60] = some(30) + [(2 * i + (i & 1), _wt(rng, weighted)) for i in unph] + some(6)
    assert len(hn[2 * 60]) == 40
    return Case("long_short_pair_" + ("w" if weighted else "u"), _irr(rng, n), hn, 1, 3,
                dict(max_list=40, has_long=True, mixed_pair=True, unit=not weighted, capt=16))


# --------------------------------------------------------------- values --
def zeros():
    rng = np.random.default_rng(80)
    n = 83
    irr = _irr(rng, n)
    hn = random_graph(rng, n, 1, 6)
    for i in range(0, 60, 7):
        irr[i] = 0.0 if i % 2 else -0.0
    for i in range(60, n):                                   # a closed neighbourhood of zero-valued samples
        irr[i] = -0.0 if i % 3 == 0 else 0.0
        for h in range(2):
            hn[2 * i + h] = [(int(rng.integers(120, 2 * n)), 1.0) for _ in range(int(rng.integers(1, 6)))]
    return Case("zeros", irr, hn, 1, 3, dict(unit=True, zero_block=(60, n)))


def negative_and_huge(weighted):
    """Negative irr, 1e-300 and 1e300.  The samples that list the 1e300 sample
    have irr of order 1 and the 1e300 sample lists ordinary samples, so no
    product or sum overflows (asserted on the CPU)."""
    rng = np.random.default_rng(90 + weighted)
    n = 91
    irr = _irr(rng, n, 0.5, 3.0)
    # neighbours only among samples 10.., so 0..9 are read by nobody but the lists set below
    hn = [[(int(rng.integers(20, 2 * n)), _wt(rng, weighted)) for _ in range(int(rng.integers(1, 7)))]
          for _ in range(2 * n)]
    for i in (12, 30, 31, 55):
        irr[i] = -float(rng.uniform(0.2, 1.5))
    irr[0], irr[1], irr[2] = 1e300, 1e-300, 1e300
    for i in (20, 41, 63):                                   # read the huge and the tiny samples
        hn[2 * i] = hn[2 * i] + [(0, _wt(rng, weighted)), (2, _wt(rng, weighted))]
        hn[2 * i + 1] = hn[2 * i + 1] + [(3, _wt(rng, weighted)), (5, _wt(rng, weighted))]
    return Case("negative_and_huge_" + ("w" if weighted else "u"), irr, hn, 1, 3,
                dict(unit=not weighted, no_overflow=True))


def all_unphased_neighbours():
    rng = np.random.default_rng(40)
    n = 41
    hn = []
    for i in range(n):
        for h in range(2):
            if i < 20:
                hn.append([(int(rng.integers(40, 2 * n)), 1.0) for _ in range(3)])
            else:
                hn.append([(int(rng.integers(0, 2 * n)), 1.0)])
    return Case("all_unphased_neighbours", _irr(rng, n), hn, 2, 3, dict(unit=True, phased=20, hap_unchanged=True))


def nobody_phased():
    rng = np.random.default_rng(41)
    n = 45
    return Case("nobody_phased", _irr(rng, n), random_graph(rng, n, 0, 5), 6, 2, dict(phased=0, unit=True))


def min_nbr_case(m):
    rng = np.random.default_rng(70)
    n = 71
    hn = random_graph(rng, n, 0, 4)
    return Case(f"min_nbr_{m}", _irr(rng, n), hn, m, 3, dict(list_lens=(0, 1, 2), unit=True))


def vanishing_weights():
    rng = np.random.default_rng(66)
    n = 63
    hn = random_graph(rng, n, 1, 6)
    for hh in range(2 * n):
        if hh % 5 != 4:
            hn[hh] = [(a, 1e-30 if (a + t) % 2 else 0.0) for t, (a, _) in enumerate(hn[hh])]
        else:
            hn[hh] = [(a, 0.5 + 0.25 * (t % 3)) for t, (a, _) in enumerate(hn[hh])]
    return Case("vanishing_weights", _irr(rng, n), hn, 1, 3, dict(unit=False, vanishing=True))


def nan_irr():
    rng = np.random.default_rng(33)
    n = 35
    irr = _irr(rng, n)
    irr[7] = NAN
    hn = random_graph(rng, n, 1, 6)
    for i in (3, 9, 20):
        hn[2 * i].append((14, 1.0))
        hn[2 * i + 1].append((15, 1.0))
    return Case("nan_irr", irr, hn, 1, 3, dict(unit=True))


# ------------------------------------------------------------- the table --
def _build():
    cs = [div_sweep("div_sweep", 16, 500), div_sweep("div_sweep_k8", 8, 501),
          div_window_edges("div_window_edges", True), div_window_edges("div_window_edges_single", False), div_hard()]
    for it in (1, 2, 3):
        cs.append(_geom(f"one_chunk_odd_it{it}", [97], it, 97))
        cs.append(_geom(f"one_chunk_even_it{it}", [64], it, 64))
        cs.append(_geom(f"three_chunks_it{it}", [130, 90], it, 3))
    for it in (1, 3):
        cs.append(_geom(f"two_chunks_it{it}", [100, 60], it, 2))
        cs.append(_geom(f"two_chunks_wide_it{it}", [200], it, 200))       # 2 chunks of 128, 1 of 256
    cs.append(_geom("iters0", [50, 31], 0, 50))
    for w in (127, 128, 129, 255, 256, 257):
        cs.append(_geom(f"width_{w}", [w, 41], 2, w))
    cs += [last_lane_only("last_lane_only", False), last_lane_only("last_lane_only_long", True)]
    ch = chain(CHAIN_N)
    ch.facts["route"] = {"default": "PHASE4"}
    cs.append(ch)
    cs.append(Case("no_edges", _irr(np.random.default_rng(37), 37), [[] for _ in range(74)], 0, 2,
                   dict(nlev=1, widths={0: 37}, nch128=1, nch256=1, max_list=0, unit=True)))
    cs += [self_and_sibling(), forward_same_level(False), forward_same_level(True)]
    cs += [odd_n(n) for n in (1, 2, 3, 5, 127, 129, 257)]
    for L in (8, 9, 16, 17):
        cs += [len_case(L, False), len_case(L, True)]
    cs += [long_short_pair(False), long_short_pair(True)]
    cs += [zeros(), negative_and_huge(False), negative_and_huge(True), all_unphased_neighbours(), nobody_phased()]
    cs += [min_nbr_case(m) for m in (0, 1, 2)]
    cs += [vanishing_weights(), nan_irr()]
    return cs


SMALL = _build()
_by = {c.name: c for c in SMALL}

_GLOBAL = {"default": "PH2_SPLIT_GLOBAL", "ph2": "PH2_SPLIT_GLOBAL", "paired": "PH_LEGACY_GLOBAL",
           "legacy": "PH_LEGACY_GLOBAL"}
_three = _geom("three_levels", [30, 30, 30], 2, 30)

# capacity: listed explicitly, padded from small cases
CAPACITY = [
    pad(chain(BAND_CHAIN, "chain600"), BAND_N, "band_ph2", nlev=BAND_CHAIN,
        route={"default": "PH2_SPLIT_LDS", "ph2": "PH2_SPLIT_LDS", "paired": "PH2_PAIRED_LDS",
               "legacy": "PH_LEGACY_LDS"}),
    pad(_three, PHASE4_MAX_3LEV, "fits_phase4_max", nlev=3,
        route={"default": "PHASE4", "ph2": "PH2_SPLIT_LDS", "paired": "PH2_PAIRED_LDS", "legacy": "PH_LEGACY_LDS"}),
    pad(_three, PHASE4_MAX_3LEV + 1, "fits_phase4_max_plus1", nlev=3,
        route={"default": "PH2_SPLIT_LDS", "ph2": "PH2_SPLIT_LDS", "paired": "PH2_PAIRED_LDS",
               "legacy": "PH_LEGACY_LDS"}),
    pad(_by["odd_n_257"], GLOBAL_N, "global_5200", route=_GLOBAL),
]
# the same edges through the global-memory kernels
PADDED = [pad(_by[nm], GLOBAL_N, route=_GLOBAL) for nm in
          ("len_16_u", "len_16_w", "len_17_u", "len_17_w", "long_short_pair_u", "long_short_pair_w",
           "forward_same_level", "zeros", "vanishing_weights")]

CASES = SMALL + CAPACITY + PADDED
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
