"""Mosdepth files and a loci table placed at the edges of the device region
coverage (grid_amd/csrc/mosdepth_dev.hip k_md_cover / k_cov_walk, driven by
grid_amd/utils/coverage_device.py) -- the inputs of tests/golden/
make_golden_cover.py (which pins them against the reference), of
test_cover_cpu.py and of test_gpu_cover.py.

The kernel's geometry is the step-4 parse's: 16 KiB chunks, one workgroup per
chunk, a 64-byte segment per thread, a line belongs to the thread whose
segment holds its first byte.  Two cohorts over ONE table of 70 loci:

``main`` (6 samples, ~40 KiB of text each = three chunks; all on the device)
  M0  BGZF.  Geometry: hit lines that start in the last segment of chunk 0,
      straddle the chunk edge, straddle a 64-byte segment edge; a locus whose
      lines lie in chunks 0 and 1 (two workgroups feed one sum).
  M1  BGZF, no final newline, the last line hits a locus.
  M2  BGZF, chr1 block in an order of its own (unsorted) with one line twice:
      both count, in file order.
  M3  BGZF, the order-sensitive depths (below) in reverse line order.
  M4  an empty file (gzip of no bytes): every cell 0.
  M5  one plain gzip member (not BGZF).
  Every file but M4 also holds: chr10 / chr11 decoy lines that repeat chr1's
  coordinates with other depths (a ``startswith`` would take them), the two
  rounding ties, and the order-sensitive locus.

``handover`` (10 samples): H0 and H1 are clean; each of H2..H9 holds ONE line
  outside the device grammar -- an empty line, three fields, five fields, depth
  1e3, depth nan (inside a locus: the reference gives Error there), a CR before
  the newline, a byte >= 0x80, a 300-byte line -- and is recomputed on the host
  while the others stay on the device.

The table (``LOCI``; tests use its prefixes of 1, 63, 64, 65 and all 70):
partial overlap at each end, a bin-aligned locus (the neighbours' r_end ==
start and r_start == end must not count), a locus with no line, a locus on an
absent chromosome, nested / overlapping / identical loci, the ties, the
order-sensitive locus, the geometry lines' loci, then chr2 windows.

Pure Python: no library is needed to build a case."""
import functools
import gzip
import struct
import zlib

CH, SEG = 16384, 64
BIN0, NBIN1 = 100000, 260          # chr1: 260 bins of 1 kb from 100000


def _depth(fi, k, salt=0):
    """File fi's depth text of record k: "%.2f" in 20-90."""
    h = 2000 + (k * 7919 + fi * 1237 + salt * 331 + 13) % 7001
    return f"{h // 100}.{h % 100:02d}"


def _bin(chrom, k, fi, salt=0):
    s = BIN0 + 1000 * k
    return f"{chrom}\t{s}\t{s + 1000}\t{_depth(fi, k, salt)}\n"


def _pad_to(text, target):
    """Filler lines (a chromosome no locus names) until the next line starts at
    byte ``target``."""
    out = []
    pos = len(text)
    assert target >= pos + 8 or target == pos
    while target - pos > 214:
        ln = "pad\t0\t1\t0.00\n"
        out.append(ln)
        pos += len(ln)
    gap = target - pos
    if gap:
        if gap < 8:                                # room for one more short line first
            raise AssertionError("pad gap too small")
        out.append("p" * (gap - 7) + "\t0\t1\t0\n")
    return "".join(out)


# --- the order-sensitive locus: depths and overlaps whose fp64 sum depends on the order ---
def _sum(terms):
    acc = 0.0
    for q, ov in terms:
        acc += (q / 100) * ov
    return acc


@functools.lru_cache(maxsize=None)
def order_terms():
    """[(hundredths, width)] of 9 adjacent chrO bins whose region_cov bits
    differ when the lines are summed in reverse (searched over seeds with a
    small LCG; the assertion keeps the order check from passing vacuously)."""
    for seed in range(1, 200):
        x, terms = seed * 2654435761 % (1 << 32), []
        for _ in range(9):
            x = (x * 1103515245 + 12345) % (1 << 31)
            q = 1 + x % 9000
            x = (x * 1103515245 + 12345) % (1 << 31)
            terms.append((q, 1 + x % 997))
        if _sum(terms).hex() != _sum(terms[::-1]).hex():
            return tuple(terms)
    raise AssertionError("no order-sensitive depths found")


def order_lines(reverse=False):
    s, lines = 5000, []
    for q, w in order_terms():
        lines.append(f"chrO\t{s}\t{s + w}\t{q // 100}.{q % 100:02d}\n")
        s += w
    return lines[::-1] if reverse else lines


def order_locus():
    return ("chrO", 5000, 5000 + sum(w for _, w in order_terms()))


TIES = ["chrT\t500\t501\t0.25\n", "chrT\t501\t502\t0.00\n",      # 0.25 / 2 -> 12.5 -> 12
        "chrU\t500\t501\t0.75\n", "chrU\t501\t502\t0\n"]          # 0.75 / 2 -> 37.5 -> 38
TIE_LOCI = [("chrT", 500, 502), ("chrU", 500, 502)]
TIE_VALUES = [12, 38]

# geometry lines: unique coordinates on chrG, a locus each
G_LAST_SEG = "chrG\t7000000\t7001000\t31.25\n"       # starts in the last segment of chunk 0
G_CHUNK_EDGE = "chrG\t7100000\t7101000\t42.50\n"     # straddles byte 16384
G_SEG_EDGE = "chrG\t7200000\t7201000\t53.75\n"       # straddles a 64-byte segment edge
G_LAST_LINE = "chrG\t7300000\t7301000\t64.01"        # a file's last line, no newline
GEOM_LOCI = [("chrG", 7000500, 7001000), ("chrG", 7100000, 7100001), ("chrG", 7199000, 7200999),
             ("chrG", 7300100, 7300900)]


def _loci():
    e = BIN0 + 1000 * NBIN1
    loci = [
        ("chr1", BIN0 + 500, BIN0 + 2500),           # 0 partial overlap at each end
        ("chr1", BIN0 + 3000, BIN0 + 4000),          # 1 one bin exactly: its neighbours touch, never count
        ("chr1", 50000000, 50001000),                # 2 no line
        ("chrZ", BIN0, e),                           # 3 an absent chromosome
        ("chr1", BIN0 + 5000, BIN0 + 10000),         # 4
        ("chr1", BIN0 + 6000, BIN0 + 8000),          # 5 nested in 4
        ("chr1", BIN0 + 7500, BIN0 + 12500),         # 6 overlaps 4
        ("chr1", BIN0 + 5000, BIN0 + 10000),         # 7 identical to 4
        ("chr1", BIN0 + 5000, BIN0 + 5001),          # 8 shares 4's start, 1 bp
        ("chr1", BIN0, e),                           # 9 the whole block: lines in chunks 0 and 1
        ("chr1", BIN0 + 4000, BIN0 + 4000),          # 10 empty
        ("chr1", BIN0 + 9000, BIN0 + 8000),          # 11 end < start
        ("chr10", BIN0 + 500, BIN0 + 2500),          # 12 the decoys' own locus
    ] + TIE_LOCI + [order_locus()] + GEOM_LOCI
    k = 0
    while len(loci) < 70:                            # chr2 windows of growing width
        loci.append(("chr2", BIN0 + 1700 * k, BIN0 + 1700 * k + 900 + 450 * k))
        k += 1
    return loci


LOCI = _loci()
N_LOCI_CASES = (1, 63, 64, 65, 70)
I_WHOLE, I_ORDER = 9, 15
I_TIES = (13, 14)
I_GEOM = (16, 17, 18, 19)


def _common(fi, reverse_order=False):
    return ([_bin("chr10", k, fi, 1) for k in range(40)] + [_bin("chr11", k, fi, 2) for k in range(40)] + TIES
            + order_lines(reverse_order))


def _main_text(fi):
    """~40 KiB: chr2, then the chr1 block across the chunk-0 edge, the special lines, the rest."""
    t = "".join(_bin("chr2", k, fi) for k in range(420))            # ~11 KiB
    chr1 = [_bin("chr1", k, fi) for k in range(NBIN1)]               # ~7 KiB: crosses byte 16384
    if fi == 2:                                                      # an order of its own, one line twice
        chr1 = chr1[130:] + chr1[:130]
        chr1.insert(50, chr1[7])
    if fi == 0:
        # chr1 lines up to the last segment of chunk 0, then the geometry lines
        n = 0
        while len(t) + len(chr1[n]) < CH - SEG - 8:
            t += chr1[n]
            n += 1
        t += _pad_to(t, CH - SEG + 5) + G_LAST_SEG                   # starts in [CH - 64, CH)
        t += _pad_to(t, CH - 11) + G_CHUNK_EDGE                      # starts before CH, ends after it
        t += "".join(chr1[n:])                                       # the rest of chr1, in chunk 1
        t += _pad_to(t, (len(t) // SEG + 2) * SEG - 9) + G_SEG_EDGE  # starts 9 bytes before a segment edge
    else:
        t += "".join(chr1)
    t += "".join(_common(fi, reverse_order=(fi == 3)))
    k = 420
    while len(t) < 40000:
        t += _bin("chr2", k, fi)
        k += 1
    if fi == 1:
        t += G_LAST_LINE
    return t.encode("ascii")


HANDOVER_KINDS = {
    "H2": ("an empty line", b"\n"),
    "H3": ("three fields", b"chr1\t100500\t100600\n"),
    "H4": ("five fields", b"chr1\t100500\t100600\t10.00\textra\n"),
    "H5": ("depth 1e3", b"chr1\t100500\t100600\t1e3\n"),
    "H6": ("depth nan, inside loci 0 and 9", b"chr1\t100500\t100600\tnan\n"),
    "H7": ("a CR before the newline", b"chr1\t100500\t100600\t10.00\r\n"),
    "H8": ("a byte >= 0x80 (valid UTF-8)", "chr\u00e9\t100500\t100600\t10.00\n".encode("utf-8")),
    "H9": ("a 300-byte line", b"chr1" + b"_" * 277 + b"\t100500\t100600\t10.00\n"),
}


def _handover_text(name, fi):
    lines = [_bin("chr2", k, fi).encode() for k in range(700)] + [_bin("chr1", k, fi).encode() for k in range(NBIN1)]
    lines += [ln.encode() for ln in _common(fi)]
    lines += [_bin("chr2", k, fi).encode() for k in range(700, 1250)]
    if name in HANDOVER_KINDS:
        lines.insert(900, HANDOVER_KINDS[name][1])                   # in the second chunk
    return b"".join(lines)


def bgzf(data, block=65280):
    """BGZF as htslib writes it: gzip members of <= 64 KiB with the "BC" extra
    field, then the empty EOF member."""
    out = bytearray()
    for a in range(0, len(data), block):
        chunk = data[a:a + block]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out += bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 6)
        out += b"BC" + struct.pack("<HH", 2, 12 + 6 + len(body) + 8 - 1) + body
        out += struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out)


def plain_gzip(data):
    return gzip.compress(data, 6, mtime=0)


@functools.lru_cache(maxsize=None)
def cases():
    """{cohort: dict(texts={sample: bytes}, pack={sample: callable}, path={sample: expected path record})}"""
    main = {f"M{i}": (b"" if i == 4 else _main_text(i)) for i in range(6)}
    hand = {f"H{i}": _handover_text(f"H{i}", i) for i in range(10)}
    return {
        "main": dict(texts=main, pack={s: (plain_gzip if s in ("M4", "M5") else bgzf) for s in main},
                     path={s: "device" for s in main}),
        "handover": dict(texts=hand, pack={s: bgzf for s in hand},
                         path={s: ("host" if s in HANDOVER_KINDS else "device") for s in hand}),
    }


def split_lines(text):
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def line_starts(text):
    out, pos = [], 0
    for ln in split_lines(text):
        out.append(pos)
        pos += len(ln) + 1
    return out


def write_cohort(root, cohort):
    """The cohort's files as ``root/{sample}.regions.bed.gz``; returns their paths in sample order."""
    import os
    c = cases()[cohort]
    os.makedirs(root, exist_ok=True)
    paths = []
    for s, text in c["texts"].items():
        p = os.path.join(root, f"{s}.regions.bed.gz")
        with open(p, "wb") as f:
            f.write(c["pack"][s](text))
        paths.append(p)
    return paths


def loci_file_text(loci=None):
    """The table as read_loci_file reads it (CHR, BP_START, BP_END, GENE)."""
    rows = ["CHR\tBP_START\tBP_END\tGENE"]
    rows += [f"{c}\t{s}\t{e}\tL{i:02d}" for i, (c, s, e) in enumerate(loci or LOCI)]
    return "\n".join(rows) + "\n"
