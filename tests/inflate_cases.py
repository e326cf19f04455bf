"""Hand-built DEFLATE streams for the inflate tests (tests/test_inflate_cases_cpu.py,
tests/test_gpu_inflate.py): a small DEFLATE writer in plain Python and, built
with it, streams aimed at the device inflater's own constants
(grid_amd/csrc/inflate.hip, inflate_core.hpp) -- the 2 KiB ring and its
near/far boundary, the 1 KiB flushes, the unmasked copy's spare slots, the
fast tables' widths, the 48-bit refill budget, the last 296 bytes of output
room, the last 16 bytes of input, and the header grammar zlib enforces.

Every case is (name, blob, expect): expect is "ok" or "reject" BY
CONSTRUCTION; no expected text is stored (the tests take it from zlib, and
the CPU test first checks that zlib's verdict is the case's expect, which
guards this writer).  The name's first component is the family.  Per name:
  SIZE[name]       length of the text the stream was written for (the output
                   capacity a caller would give it; for a rejected stream the
                   text it pretends to hold)
  CAP_EXTRA[name]  capacities to decode at, as offsets to SIZE (default (0,));
                   -1 must give E_SPACE
  MEMBERS[name]    gzip members in the blob (default 1)
  CRC_FLIPPED      names whose only defect is one flipped trailer-CRC bit
  F1_TOKENS[name]  family 1's token lists (to count the (dist, len) pairs)
"""
import bisect
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import numpy as np

# the kernel's constants (tests/test_inflate_cases_cpu.py checks them against the source)
RING, FLUSH = 2048, 1024
NEAR = RING - 258
ROOM = 296                  # fast_codes leaves the last ROOM bytes of output room to the core
TAIL = 16                   # ... and the last TAIL bytes of input
LFAST, DFAST = 8, 7

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [x for k in range(1, 14) for x in (k, k)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def host_core(lfast, workdir):
    """The decoding core built for the host (tests/native/inflate_core_host.cpp)
    at a literal/length fast table of 2^lfast entries, as a ctypes library."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(workdir), "libicore.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-DGRID_INFLATE_LFAST={lfast}",
                    "-I" + os.path.join(root, "grid_amd", "csrc"),
                    os.path.join(root, "tests", "native", "inflate_core_host.cpp"), "-o", so, "-lz"], check=True)
    lib = C.CDLL(so)
    lib.host_gunzip.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                C.POINTER(C.c_int32)]
    assert lib.host_lfast() == lfast
    return lib


def host_gunzip(lib, blob, cap):
    """(status, text, members) of the host core on ``blob`` with room for cap bytes."""
    src = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    out = np.zeros(max(cap, 1), np.uint8)
    n, m = C.c_int64(), C.c_int32()
    rc = lib.host_gunzip(src.ctypes.data, len(blob), out.ctypes.data, cap, C.byref(n), C.byref(m))
    return rc, out[: n.value].tobytes(), m.value


class BitWriter:
    """An integer bit accumulator, least significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.acc, self.cnt, self.done_bytes = 0, 0, bytearray()

    def bits(self, v, n):
        """n bits of v, LSB first (extra bits, header fields; Huffman codes
        arrive here already reversed: canonical() stores them so)."""
        self.acc |= (v & ((1 << n) - 1)) << self.cnt
        self.cnt += n
        if self.cnt >= 2048:
            k = self.cnt >> 3
            self.done_bytes += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.cnt -= 8 * k

    def align(self):
        self.cnt = -(-self.cnt // 8) * 8

    def raw(self, b):
        assert self.cnt % 8 == 0
        self.done_bytes += self.acc.to_bytes(self.cnt // 8, "little") + bytes(b)
        self.acc = self.cnt = 0

    def phase(self):
        return self.cnt & 7

    def getvalue(self):
        return bytes(self.done_bytes) + self.acc.to_bytes((self.cnt + 7) // 8, "little")


def canonical(lens):
    """{symbol: (code reversed for LSB-first writing, length)} of the canonical
    Huffman code with these lengths (RFC 1951 3.2.2; 0 = unused).  Incomplete
    and over-subscribed sets are written as the algorithm gives them (an
    over-subscribed set's codes wrap): their streams are reject cases."""
    maxl = max(lens, default=0)
    count = [0] * (maxl + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            c = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)      # MSB-first code -> LSB-first bits
    return out


def kraft(lens):
    """sum of 2^-l as a fraction of 2^15."""
    return sum(1 << (15 - l) for l in lens if l)


def as_list(d, n_min):
    d = dict(d)
    n = max(n_min, max(d, default=-1) + 1)
    return [d.get(s, 0) for s in range(n)]


def staircase(steps, tail):
    """A complete length set with codes up to 15 bits: the symbols of ``steps``
    get 1, 2, ..., len(steps) bits and the 2^k symbols of ``tail`` 15 bits
    (len(steps) = 15 - k: 14 steps and 2 tail symbols, 13 and 4, ...)."""
    k = len(tail).bit_length() - 1
    assert len(tail) == 1 << k and len(steps) == 15 - k
    d = {s: i + 1 for i, s in enumerate(steps)}
    d.update({s: 15 for s in tail})
    assert len(d) == len(steps) + len(tail) and kraft(d.values()) == 1 << 15
    return d


LL_FIXED = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
D_FIXED = canonical([5] * 32)
_LEN_SYM = {}
for _s in range(28):
    for _x in range(1 << LEN_EXTRA[_s]):
        _LEN_SYM.setdefault(LEN_BASE[_s] + _x, (257 + _s, _x))
_LEN_SYM[258] = (285, 0)


def D(dist):
    """the raw distance token of a distance."""
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return ("D", s, dist - DIST_BASE[s])


def emit(w, tokens, ll, dd, eob=True):
    """Tokens: an int is a literal byte; (len, dist) a match in its usual
    coding; ("L", sym, extra) / ("D", sym, extra) a raw literal/length or
    distance symbol with its extra-bits value (illegal symbols have none);
    ("B", value, nbits) raw bits."""
    for t in tokens:
        if isinstance(t, int):
            w.bits(*ll[t])
        elif t[0] == "L":
            w.bits(*ll[t[1]])
            w.bits(t[2], LEN_EXTRA[t[1] - 257] if 257 <= t[1] <= 285 else 0)
        elif t[0] == "D":
            w.bits(*dd[t[1]])
            w.bits(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        elif t[0] == "B":
            w.bits(t[1], t[2])
        else:
            s, x = _LEN_SYM[t[0]]
            w.bits(*ll[s])
            w.bits(x, LEN_EXTRA[s - 257])
            _, ds, dx = D(t[1])
            w.bits(*dd[ds])
            w.bits(dx, DIST_EXTRA[ds])
    if eob:
        w.bits(*ll[256])


def expand(out, tokens):
    """Append the text of ``tokens`` to the bytearray ``out`` (whose contents
    are the history).  Lenient, for the reject cases' pretended text: a source
    byte before the history reads 0, illegal symbols give nothing."""
    pend = None
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if t[0] == "B":
            continue
        if t[0] == "L":
            pend = LEN_BASE[t[1] - 257] + t[2] if 257 <= t[1] <= 285 else None
            continue
        if t[0] == "D":
            if pend is None or t[1] >= 30:
                pend = None
                continue
            ln, dist, pend = pend, DIST_BASE[t[1]] + t[2], None
        else:
            ln, dist = t
        n = len(out)
        if dist > n:
            for k in range(ln):
                i = len(out) - dist
                out.append(out[i] if i >= 0 else 0)
        elif dist >= ln:
            out += out[n - dist:n - dist + ln]
        else:
            out += (bytes(out[n - dist:]) * (ln // dist + 1))[:ln]


def rle_zero_runs(lens):
    """The plainest code-length sequence: lengths as themselves, runs of >= 3
    zeros as 17 / 18."""
    seq, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0:
                j += 1
            run = j - i
            while run >= 3:
                r = min(run, 138)
                seq.append((18, r - 11) if r >= 11 else (17, r - 3))
                run -= r
            seq += [(0, 0)] * run
            i = j
        else:
            seq.append((lens[i], 0))
            i += 1
    return seq


CL_DEFAULT = {s: 4 if s < 13 else 5 for s in range(19)}     # complete: 13/16 + 6/32


class Member:
    """One DEFLATE stream under construction, with the text it stands for."""

    def __init__(self, history=b""):
        self.w = BitWriter()
        self.out = bytearray(history)
        self.base = len(history)

    @property
    def pos(self):
        return len(self.out) - self.base

    @property
    def text(self):
        return bytes(self.out[self.base:])

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + bytes(data))
        self.out += data
        return self

    def stored_long(self, data, final=False):
        """any length, as stored blocks of up to 65535 bytes."""
        parts = [data[a:a + 65535] for a in range(0, len(data), 65535)] or [b""]
        for k, p in enumerate(parts):
            self.stored(p, final and k == len(parts) - 1)
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        emit(self.w, tokens, LL_FIXED, D_FIXED, eob)
        expand(self.out, tokens)
        return self

    def dynamic(self, tokens, ll, dd, final=False, eob=True, hlit=None, hdist=None, cl=None, seq=None):
        """ll / dd: {symbol: length} of the literal/length and distance sets.
        hlit / hdist: the header's raw 5-bit fields when they are to lie;
        cl: {symbol: length} of the code-length code; seq: the explicit
        code-length-code sequence [(symbol, extra value)]."""
        ll_l, dd_l = as_list(ll, 257), as_list(dd, 1)
        cl = CL_DEFAULT if cl is None else cl
        seq = rle_zero_runs(ll_l + dd_l) if seq is None else seq
        cl_l = as_list(cl, 19)
        hclen = max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl_l[s]), default=4))
        w = self.w
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(len(ll_l) - 257 if hlit is None else hlit, 5)
        w.bits(len(dd_l) - 1 if hdist is None else hdist, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_l[s], 3)
        clc = canonical(cl_l)
        for s, x in seq:
            w.bits(*clc[s])
            w.bits(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        emit(w, tokens, canonical(ll_l), canonical(dd_l), eob)
        expand(self.out, tokens)
        return self

    def raw_bits(self, v, n):
        self.w.bits(v, n)
        return self

    def gz(self, crc=None, isize=None, bgzf=False):
        """The gzip member: the trailer is the caller's (default: the text's)."""
        body = self.w.getvalue()
        t = self.text
        crc = zlib.crc32(t) if crc is None else crc
        isize = len(t) & 0xFFFFFFFF if isize is None else isize
        if bgzf:
            head = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 6) + b"BC"
            head += struct.pack("<HH", 2, (12 + 6 + len(body) + 8 - 1) & 0xFFFF)
        else:
            head = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
        return head + body + struct.pack("<II", crc, isize)


CASES = []
SIZE, CAP_EXTRA, MEMBERS, F1_TOKENS = {}, {}, {}, {}
CRC_FLIPPED = set()


def _add(name, blob, expect, size, extra=(0,), members=1):
    assert name not in SIZE and expect in ("ok", "reject")
    CASES.append((name, bytes(blob), expect))
    SIZE[name], CAP_EXTRA[name], MEMBERS[name] = size, tuple(extra), members


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n)) if n < 64 else rng.getrandbits(8 * n).to_bytes(n, "little")


def family(name):
    return name.split("/")[0]


# 1. overlapping copies, exhaustive: every (dist, len), 1 <= dist < len <= 258
# (copy_bytes' quotient k - dist * floor((k + 0.5) * rcp(dist))), and dist in
# {len, len + 1} (its no-division branch); each after 8 fresh literals, so the
# window a copy repeats is not itself periodic in dist.  32 streams = 32 waves.
F1_STREAMS = 32


def _f01():
    for i in range(F1_STREAMS):
        rng = random.Random(100 + i)
        toks = list(_rb(rng, 260))
        for ln in range(3, 259):
            if ln % F1_STREAMS != i:
                continue
            for dist in range(1, ln + 2):
                toks += list(_rb(rng, 8))
                toks.append((ln, dist))
        toks += list(_rb(rng, 8))
        m = Member().fixed(toks, final=True)
        name = "f01_overlap/%02d" % i
        F1_TOKENS[name] = toks
        _add(name, m.gz(), "ok", m.pos)


# 2. the near/far boundary: dist x len, the copy starting 0..2 bytes before and
# after a flush boundary that is the ring's wrap (a multiple of RING), one that
# is not, and half a copy before the wrap.  Random stored bytes carry the text
# to each start; each copy is followed by a near copy of what it wrote (the
# ring must hold it, a far copy's bytes included).
F2_DISTS = (NEAR - 1, NEAR, NEAR + 1, NEAR + 2, RING - 1, RING, RING + 1, 32767, 32768)
F2_LENS = (3, 63, 64, 65, 258)


def _f02():
    for dist in F2_DISTS:
        rng = random.Random(200 + dist)
        m = Member()
        for ln in F2_LENS:
            offs = [-(ln // 2)] + [b + d for b in (0, FLUSH) for d in (-2, -1, 0, 1, 2)]
            for off in sorted(set(offs)):
                base = -(-(max(m.pos, dist) + 2 + ln) // RING) * RING
                m.stored_long(_rb(rng, base + off - m.pos))
                assert m.pos == base + off and m.pos >= dist
                m.fixed([(ln, dist), (ln, ln)])
        m.stored(_rb(rng, 300), final=True)
        _add("f02_nearfar/d%d" % dist, m.gz(), "ok", m.pos)


# 3. spare slots: a length-3 copy's unmasked 64-lane store leaves bytes in the
# ring slots 1988..2048 back from the next symbol; a copy that reads there at
# once must take its source from the flushed output.
F3_DISTS = (NEAR, NEAR + 1, 1984, 1985, 2000, 2045, RING)


def _f03():
    for k, fill in enumerate((611, 1021)):
        rng = random.Random(300 + k)
        m = Member().stored(_rb(rng, 2300 + k))
        for dist in F3_DISTS:
            for ln in (3, 64, 258):
                m.fixed([(3, 7), (ln, dist)])
                m.stored(_rb(rng, fill))
        m.stored(_rb(rng, 300), final=True)
        _add("f03_spare/%d" % k, m.gz(), "ok", m.pos)


# 4. distance against the member's start: dist == pos - mstart is the longest
# legal one.  fast: >= ROOM bytes of text and > TAIL bytes of input follow the
# copy (the device's fast loop tests it); core: the copy ends the text (the
# core's copy() does).  In a later member the trailer is written for a decoder
# that reached into the previous member's text: only the distance test rejects.
def _f04():
    rng = random.Random(400)
    prev = _rb(rng, 3000)
    for p in (100, NEAR, NEAR + 1, 5000):
        pre = _rb(rng, p)
        for path in ("fast", "core"):
            for over in (0, 1):
                for later in (0, 1):
                    m = Member(prev if later else b"").stored(pre).fixed([(20, p + over)], final=path == "core")
                    if path == "fast":
                        m.stored(_rb(rng, 400), final=True)
                    blob, size = m.gz(bgzf=True), m.pos
                    if later:
                        blob, size = Member().stored(prev, final=True).gz(bgzf=True) + blob, size + len(prev)
                    _add("f04_mstart/%s_p%d_%s_%s" % ("later" if later else "first", p, path,
                                                      "over" if over else "exact"),
                         blob, "reject" if over else "ok", size, members=1 + later)


# 5. the longest symbols.
def _f05():
    rng = random.Random(500)
    # a: length symbols 281-284 and distance symbols 28-29 at 15 bits: 15 + 5 +
    # 15 + 13 = 48 bits a pair, back to back and after 0..7 one-bit literals
    ll = staircase(list(b"abcdefghijkl") + [256], [281, 282, 283, 284])
    dd = staircase(list(range(14)), [28, 29])
    toks = []
    for rep in range(3):
        for r in range(8):
            toks += [ord("a")] * r
            for k in range(3):       # extra bits all ones, all zeros, random
                toks += [("L", 281 + (rep + r + k) % 4, (31, 0, rng.randrange(32))[k]),
                         ("D", 28 + (r + k) % 2, (8191, 0, rng.randrange(8192))[(k + rep) % 3])]
    m = Member().stored(_rb(rng, 32768)).dynamic(toks, ll, dd).stored(_rb(rng, 300), final=True)
    _add("f05_long/pairs48", m.gz(), "ok", m.pos)
    # b: a code of every length 1..15 -- exactly LFAST and LFAST + 1, DFAST and
    # DFAST + 1 bits among them at any table width -- for literals, for length
    # symbols and for distance symbols
    lits = list(b"ABCDEFGHIJKLMN")
    ll = staircase(lits, [256, 257])
    dd = staircase(list(range(14)), [14, 15])
    toks = []
    for k in range(4):
        toks += lits + lits[::-1] + [("L", 257, 0), D(1 + k)]
    m = Member().dynamic(toks, ll, dd).stored(_rb(rng, 300), final=True)
    _add("f05_long/literal_steps", m.gz(), "ok", m.pos)
    ll = staircase(list(range(257, 271)), [256, ord("z")])
    toks = [ord("z")] * 4
    for s in range(257, 271):
        for ds in list(range(16)):
            toks += [("L", s, LEN_EXTRA[s - 257] and 1), ("D", ds, (1 << DIST_EXTRA[ds]) - 1), ord("z")]
    m = Member().stored(_rb(rng, 400)).dynamic(toks, ll, dd).stored(_rb(rng, 300), final=True)
    _add("f05_long/length_and_distance_steps", m.gz(), "ok", m.pos)
    # c: length 258 as symbol 285 and as symbol 284 with extra 31
    toks = list(b"0123456789") + [("L", 285, 0), D(10), 33, ("L", 284, 31), D(3), 34, ("L", 284, 30), D(1)]
    m = Member().fixed(toks).stored(_rb(rng, 300), final=True)
    _add("f05_long/len258_both_ways", m.gz(), "ok", m.pos)


# 6. illegal symbols, once in mid-block (the fast loop) and once at the very
# end of the input (the core's loop).
def _f06():
    rng = random.Random(600)
    ll = {ord("a"): 1, ord("b"): 2, 256: 3, 257: 3}
    bad = {
        "litlen286": ("fixed", [("L", 286, 0)]),
        "litlen287": ("fixed", [("L", 287, 0)]),
        "dist30": ("fixed", [("L", 257, 0), ("D", 30, 0)]),
        "dist31": ("fixed", [("L", 257, 0), ("D", 31, 0)]),
        "onebit_dist_unused_code": ({1: 1}, [("L", 257, 0), ("B", 1, 1)]),
        "length_without_dist_code": ({}, [("L", 257, 0), ("B", 0, 5)]),
    }
    for what, (dd, toks) in bad.items():
        for where in ("mid", "tail"):
            lits = [rng.choice(b"ab") for _ in range(420)]
            toks_all = lits[:20] + toks + lits[20:] if where == "mid" else lits + toks
            m = Member()
            if dd == "fixed":
                m.fixed(toks_all, final=True)
            else:
                m.dynamic(toks_all, ll, dd, final=True)
            _add("f06_illegal/%s_%s" % (what, where), m.gz(), "reject", m.pos)
    # the same blocks without the illegal symbol are fine
    lits = [rng.choice(b"ab") for _ in range(420)]
    _add("f06_illegal/none_fixed", Member().fixed(lits, final=True).gz(), "ok", 420)
    _add("f06_illegal/none_onebit_dist", Member().dynamic(lits + [(3, 2)], ll, {1: 1}, final=True).gz(), "ok", 423)
    _add("f06_illegal/none_no_dist", Member().dynamic(lits, ll, {}, final=True).gz(), "ok", 420)


# 7. header grammar.  zlib (inflate_table): an over-subscribed set is an error;
# an incomplete one too, unless it is a literal/length or distance set with a
# single code of length 1 (or a distance set with no code).
INCOMPLETE = ("f07_header/incomplete_litlen_2_2_2", "f07_header/incomplete_dist_two_of_length_2",
              "f07_header/incomplete_dist_one_of_length_2", "f07_header/incomplete_code_length_code")


def _f07():
    a, b = ord("a"), ord("b")
    full = {a: 2, b: 2, 256: 2, 257: 2}
    abab = [a, b, (3, 2)]
    lit3 = {a: 1, b: 2, 256: 2}

    def dyn(name, expect, toks, ll, dd, **kw):
        m = Member().dynamic(toks, ll, dd, final=True, **kw)
        _add("f07_header/" + name, m.gz(), expect, m.pos)

    dyn("ok_complete_litlen_one_1bit_dist", "ok", abab, full, {1: 1})
    dyn("incomplete_litlen_2_2_2", "reject", [a, b], {a: 2, b: 2, 256: 2}, {0: 1})
    dyn("incomplete_dist_two_of_length_2", "reject", abab, full, {0: 2, 1: 2})
    dyn("incomplete_dist_one_of_length_2", "reject", abab, full, {1: 2})
    dyn("ok_no_dist_code", "ok", [a, b, a, b], lit3, {})
    # the code-length code: lit3 + one zero distance length need symbols 0, 1, 2 (no repeats)
    plain = [(l, 0) for l in as_list(lit3, 257) + [0]]
    dyn("ok_complete_code_length_code", "ok", [a, b, a, b], lit3, {}, cl={0: 1, 1: 2, 2: 2}, seq=plain)
    dyn("incomplete_code_length_code", "reject", [a, b, a, b], lit3, {}, cl={0: 2, 1: 2, 2: 2}, seq=plain)
    dyn("ok_only_end_of_block", "ok", [], {256: 1}, {})
    m = Member().dynamic([], {256: 1}, {}).fixed([a, b, a, b], final=True)
    _add("f07_header/ok_only_end_of_block_then_text", m.gz(), "ok", m.pos)
    dyn("oversubscribed_litlen", "reject", [a, b], {a: 1, b: 1, 256: 1}, {0: 1})
    dyn("oversubscribed_dist", "reject", abab, full, {0: 1, 1: 1, 2: 1})
    dyn("oversubscribed_code_length_code", "reject", [a, b, a, b], lit3, {}, cl={0: 1, 1: 1, 2: 1}, seq=plain)
    dyn("no_end_of_block_code", "reject", [a, b, a, b], {a: 1, b: 1}, {}, eob=False)
    dyn("repeat_16_first", "reject", [a, b, a, b], lit3, {}, seq=[(16, 0)] + rle_zero_runs(as_list(lit3, 257) + [0]))
    # lengths 256, 257 = 2, 2 and then a repeat of the previous length that
    # runs on into the four distance lengths
    head = [(18, a - 11), (2, 0), (2, 0), (18, 127), (18, 157 - 138 - 11), (2, 0), (2, 0)]
    assert a + 2 + 138 + 19 + 2 == 258
    dyn("ok_repeat_runs_into_distances", "ok", abab + [(3, 4), (3, 1), (3, 3)], full, {0: 2, 1: 2, 2: 2, 3: 2},
        seq=head + [(16, 1)])
    dyn("repeat_overruns_total", "reject", abab, full, {0: 2, 1: 2, 2: 2, 3: 2}, seq=head + [(16, 3)])
    for v in (30, 31):
        dyn("hlit_%d" % v, "reject", abab, full, {1: 1}, hlit=v)
        dyn("hdist_%d" % v, "reject", abab, full, {1: 1}, hdist=v)
    m = Member().raw_bits(1, 1).raw_bits(3, 2).raw_bits(0, 200)
    _add("f07_header/block_type_3", m.gz(crc=0, isize=0), "reject", 4)


# 8. stored blocks: LEN 0 between Huffman blocks at all 8 bit phases (a fixed
# block of m nine-bit and n eight-bit literals ends at bit 2 + m mod 8), LEN
# 65535, LEN / NLEN mismatch.
def _f08():
    rng = random.Random(800)
    chain = Member()
    for ph in range(8):
        m = Member()
        for mm in (m, chain):
            mm.fixed([200 + ph] * ((ph - 2) % 8) + [65, 66, 67])
            assert mm is chain or mm.w.phase() == ph
            mm.stored(b"").fixed([68, (3, 2), 69], final=mm is m)
        _add("f08_stored/len0_phase%d" % ph, m.gz(), "ok", m.pos)
    chain.stored(b"", final=True)
    _add("f08_stored/len0_chain_final", chain.gz(), "ok", chain.pos)
    m = Member().stored(_rb(rng, 65535), final=True)
    _add("f08_stored/len65535", m.gz(), "ok", m.pos)
    m = Member().fixed([65] * 5).stored(_rb(rng, 65535)).fixed([66, (258, 32768)], final=True)
    _add("f08_stored/len65535_between_fixed", m.gz(), "ok", m.pos)
    for nlen in (0x0005, 0xFFFB, 0xFFFA ^ 0x8000):
        m = Member().stored(b"hello", final=True, nlen=nlen)
        _add("f08_stored/nlen_%04x" % nlen, m.gz(), "reject", 5)


# 9. the input's tail: one fixed block ending in 0..40 one-byte literals, so
# the fast loop's hand-over to the core (fewer than TAIL bytes ahead) falls on
# every byte; streams of 244, 256, 512 +- 2 bytes (the 256-byte input window,
# its last refill at offset 244).  Decoded with ROOM spare bytes of capacity
# too (CAP_EXTRA), or the output room would end the fast loop first.
def _f09():
    rng = random.Random(900)
    lit = lambda n: [rng.randrange(32, 127) for _ in range(n)]    # noqa: E731  (8-bit codes)
    for t in range(41):
        m = Member().fixed(lit(30) + [(258, 30), (40, 1), (3, 288)] + lit(t), final=True)
        _add("f09_tail/trailing%02d" % t, m.gz(), "ok", m.pos, extra=(0, ROOM))
    for n in (244, 256, 512):
        for d in (-2, -1, 0, 1, 2):
            m = Member().fixed(lit(n + d - 20), final=True)
            blob = m.gz()
            assert len(blob) == n + d
            _add("f09_tail/stream%d" % (n + d), blob, "ok", m.pos, extra=(0, ROOM))


# 10. output room: texts that end in copies, decoded at the capacities of
# CAP_EXTRA; one byte too few must give E_SPACE.
F10_EXTRA = (0, 1, ROOM - 1, ROOM, ROOM + 1, -1)


def _f10():
    rng = random.Random(1000)
    lits = list(_rb(rng, 500))
    for name, end in (("copies", [(258, 5), (100, 300), (3, 1), (258, 258)]), ("copy_far", [(258, 1900)]),
                      ("copy_literal", [(258, 7), 65]), ("short_copy", [(3, 3)])):
        m = Member().stored(_rb(rng, 1500)).fixed(lits + end, final=True)
        _add("f10_room/" + name, m.gz(), "ok", m.pos, extra=F10_EXTRA)
    m = Member().stored(_rb(rng, 700), final=True)
    _add("f10_room/stored", m.gz(), "ok", m.pos, extra=F10_EXTRA)


# 11. member sizes for the two CRC kernels (k_gz_crc: 256 ranges of a multiple
# of 8 bytes; k_member_check: 1 KiB chunks, 64 lanes, a byte-wise tail), each
# also with one bit of the trailer's CRC flipped.
F11_SIZES = (0, 1, 1023, 1024, 1025, 65535, 65536, 65537, 66559, 131073)


def _f11():
    rng = random.Random(1100)
    for n in F11_SIZES:
        m = Member().stored_long(_rb(rng, n), final=True)
        _add("f11_crc/len%d" % n, m.gz(bgzf=n < 60000), "ok", n)
        name = "f11_crc/len%d_crcflip" % n
        _add(name, m.gz(crc=zlib.crc32(m.text) ^ (1 << rng.randrange(32)), bgzf=n < 60000), "reject", n)
        CRC_FLIPPED.add(name)


for _f in (_f01, _f02, _f03, _f04, _f05, _f06, _f07, _f08, _f09, _f10, _f11):
    _f()
FAMILIES = sorted({family(n) for n, _, _ in CASES})


def overlap_pairs():
    """the (dist, len) of every copy in family 1's streams."""
    return {(t[1], t[0]) for toks in F1_TOKENS.values() for t in toks if isinstance(t, tuple)}
