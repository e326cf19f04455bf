"""Mosdepth text placed at the device parser's own edges (grid_amd/csrc/
mosdepth_dev.hip: k_md_count, k_md_scan, k_md_parse) -- the inputs of
test_gpu_mdparse.py, and of test_mdparse_cases_cpu.py, which pins what they
mean without a GPU (the host parser against the line-by-line restatement of
the reference, and the geometry computed from the text).

The parser's geometry: the text is cut in chunks of CH = 16384 bytes, a
workgroup holds one chunk in LDS with a 16-byte halo before it and MAXLINE =
256 bytes of look-ahead after it; a thread owns a 64-byte segment and finds
newlines per 16-byte word; a line belongs to the thread whose segment holds
its first byte; the file's last partial 16-byte word is loaded byte by byte.

Its grammar (md_line): CHROM\\tSTART\\tEND\\tDEPTH with CHROM one or more bytes
0x21-0x7e, START / END 1-18 digits, DEPTH D{1,15}(.D{0,2})? of at most
21474836.47; a line of more than 256 bytes, any byte >= 0x80 and every other
form hand the cohort to the host parser.  ``device_accepts`` restates that.

A case is dict(files={sample: [lines]}, chrom, start, end, excluded, lo, hi,
expect="device" | "hands_over") plus what its own assertions need.  Lines are
str (ASCII); a file's text is their concatenation, so a last line without
"\\n" is a file without a final newline.  Every file of a cohort has the same
layout and depths of its own ("%.2f" in 20-90), so all files hold the same
keys.  Pure Python: no library is needed to build a case."""
import functools
import re

CH, SEG, WORD, MAXLINE = 16384, 64, 16, 256

_LINE = re.compile(rb"([\x21-\x7e]+)\t([0-9]{1,18})\t([0-9]{1,18})\t([0-9]{1,15})(?:\.([0-9]{0,2}))?")


def parse_line(line):
    """md_line on one line (bytes, no newline): (chrom, start, end,
    hundredths), or None where the device declines."""
    m = _LINE.fullmatch(line)
    if m is None:
        return None
    fp = m.group(5) or b""
    q = int(m.group(4)) * 100 + (int(fp) * (10 if len(fp) == 1 else 1) if fp else 0)
    if q > 2147483647:
        return None
    return m.group(1), int(m.group(2)), int(m.group(3)), q


def split_lines(text):
    """The lines of a file (bytes, newlines removed); an unterminated last
    line counts, an empty tail after the last newline does not."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def device_accepts(text, prefix):
    """Whether the device parser reads this file (bytes) itself: no byte
    >= 0x80, no line of more than MAXLINE bytes (even one the prefix test would
    skip), and every line that starts with ``prefix`` (every line when it is
    empty or None) inside md_line's grammar."""
    if any(b >= 0x80 for b in text):
        return False
    pre = (prefix or "").encode()
    for ln in split_lines(text):
        if len(ln) > MAXLINE:
            return False
        if pre and not ln.startswith(pre):
            continue
        if parse_line(ln) is None:
            return False
    return True


def ref_lines(text, prefix):
    """What the reference-file pass (MODE 0) sees in a file with no window and
    no mask: (number of lines, [(0-based line number, start, end)] of the
    lines that pass the prefix test, in line order)."""
    pre = (prefix or "").encode()
    lines = split_lines(text)
    kept = []
    for i, ln in enumerate(lines):
        if pre and not ln.startswith(pre):
            continue
        _, s, e, _ = parse_line(ln)
        kept.append((i, s, e))
    return len(lines), kept


def text_of(lines):
    return "".join(lines).encode("ascii")


def line_starts(text):
    """Byte offsets at which a line starts."""
    out, pos = [], 0
    for ln in split_lines(text):
        out.append(pos)
        pos += len(ln) + 1
    return out


def _case(files, chrom=None, start=None, end=None, excluded=None, lo=20, hi=100, expect="device", **extra):
    return dict(files=files, chrom=chrom, start=start, end=end, excluded=excluded or {}, lo=lo, hi=hi,
                expect=expect, **extra)


def _depth(fi, k):
    """File fi's depth text of record k: "%.2f" in 20-90."""
    h = 2000 + (k * 7919 + fi * 1237 + 13) % 7001
    return f"{h // 100}.{h % 100:02d}"


# ------------------------------------------------------------ line builders --
def _rec_prefix(n, k, fi):
    """A chr1... record of n >= 24 bytes (no newline) with 6-digit coordinates,
    key index k < 899; long ones get their length from the chromosome name."""
    assert n >= 24 and 0 <= k < 899
    s = 100000 + 1000 * k
    ln = f"chr1{'_' * (n - 24)}\t{s}\t{s + 1000}\t{_depth(fi, k)}"
    assert len(ln) == n
    return ln + "\n"


_NAME0 = "1Xc#:|~"


def _rec_any(n, k, fi):
    """A record of n >= 23 bytes with 7-digit coordinates and a chromosome
    field of n - 22 bytes (no prefix mode: any name), key index k <= 17998."""
    assert n >= 23 and 0 <= k <= 17998
    s = 1000000 + 500 * k
    ln = f"{_NAME0[k % len(_NAME0)]}{'_' * (n - 23)}\t{s}\t{s + 500}\t{_depth(fi, k)}"
    assert len(ln) == n
    return ln + "\n"


_FILL_BODY = "#filler " + "chr2\t100\t200\t5.00 xyz\t" * 16
_FILL_LENS = (7, 31, 64, 100, 257, 16, 1, 200, 128, 65, 255, 48, 17, 256, 90)


def _filler(total):
    """A filler line of ``total`` >= 1 bytes with its newline: ASCII, at most
    256 bytes before the newline, not starting with chr1."""
    assert 1 <= total <= MAXLINE + 1
    return _FILL_BODY[:total - 1] + "\n"


class _Fill:
    """Fills a gap of bytes with whole lines: fillers (prefix mode; any gap),
    or real records with keys of their own (no prefix mode; a gap of 0, or of
    at least 48 bytes)."""
    _REC_LENS = (23, 24, 31, 40, 63, 64, 65, 90, 127, 128, 129, 180, 222, 255, 256)

    def __init__(self, fi, records):
        self.fi, self.records, self.k, self.c = fi, records, 0, 0

    def take_key(self):
        self.k += 1
        return self.k - 1

    def __call__(self, gap):
        out = []
        assert gap >= 0, gap
        if not self.records:
            while gap > 0:
                n = min(_FILL_LENS[self.c % len(_FILL_LENS)], gap)
                self.c += 1
                out.append(_filler(n))
                gap -= n
            return out
        assert gap == 0 or gap >= 48, gap
        while gap > 2 * (MAXLINE + 1):
            n = self._REC_LENS[self.c % len(self._REC_LENS)]
            self.c += 1
            out.append(_rec_any(n, self.take_key(), self.fi))
            gap -= n + 1
        if gap > MAXLINE + 1:
            a = gap // 2
            out.append(_rec_any(a - 1, self.take_key(), self.fi))
            gap -= a
        if gap:
            out.append(_rec_any(gap - 1, self.take_key(), self.fi))
        return out


# ---------------------------------------------------------------- a. chunks --
_NEAR = (-1, 0, 1)
SWEEP = ([(24, off) for off in range(-27, 3)]
         + [(n, off) for n in (64, 65) for off in (*range(-66, -61), *_NEAR)]
         + [(n, off) for n in (255, 256) for off in (*range(-258, -253), -129, -128, *_NEAR)])


def chunk_sweep(records=False):
    """One record per chunk boundary B = CH * b, b = 1, 2, ...: record b - 1 of
    SWEEP = (length, off) starts at B + off.  records=False: chrom "chr1", the
    space between is filler lines; True: no chromosome filter, the space is
    real records of varied lengths, so every line of the file is parsed.
    ``placed``: (byte offset, length) of the swept records."""
    files, placed = {}, []
    for fi in range(3):
        fill = _Fill(fi, records)
        lines, pos, placed = [], 0, []
        for b, (n, off) in enumerate(SWEEP, 1):
            at = CH * b + off
            lines += fill(at - pos)
            lines.append(_rec_any(n, fill.take_key(), fi) if records else _rec_prefix(n, b - 1, fi))
            placed.append((at, n))
            pos = at + n + 1
        lines += fill(CH * (len(SWEEP) + 1) - 700 - pos)
        files[f"C{fi:03d}"] = lines
    return _case(files, chrom=None if records else "chr1", placed=placed)


# -------------------------------------------------------------- b. segments --
def segment_sweep():
    """Records of 17...90 bytes in a cycle, no chromosome filter: record starts
    on every residue mod 64 (the thread that owns a line), newlines on every
    residue mod 16 (the bit of the word's mask)."""
    files = {}
    for fi in range(2):
        lines = []
        for k in range(13 * 74):
            n = 17 + k % 74
            body = f"\t{k}\t{k + 1000}\t{_depth(fi, k)}"
            lines.append("c" + "_" * (n - len(body) - 1) + body + "\n")
            assert len(lines[-1]) == n + 1
        files[f"G{fi:03d}"] = lines
    starts = line_starts(text_of(files["G000"]))
    assert {p % SEG for p in starts} == set(range(SEG))
    assert {(p - 1) % WORD for p in starts[1:]} == set(range(WORD))
    return _case(files)


# ----------------------------------------------------------------- c. tails --
def file_tails():
    """About 75 files over a common body (short: inside the first chunk;
    long: into the second) with differing ends.  ``lengths``: sample -> the
    file length the case intends."""
    def rec(k, fi, nl=True):
        return _rec_prefix(24, k, fi)[:None if nl else -1]

    def first(fi, nl=True):
        return f"chr1\t5\t9\t{_depth(fi, 898)}" + ("\n" if nl else "")

    def short(fi):                       # a record at byte 0, then records between fillers
        fill, out = _Fill(fi, False), [first(fi)]
        for k in range(30):
            out += fill(37 + k)
            out.append(rec(k, fi))
        return out

    def long(fi):                        # the same and on into the second chunk; length = short's mod 64
        fill, out = _Fill(fi, False), short(fi)
        n0 = n = sum(map(len, out))
        for k in range(30, 60):
            g = fill((CH + 300 - n0) // 30)
            out += g + [rec(k, fi)]
            n += sum(map(len, g)) + 25
        return out + fill((n0 - n) % 64)

    def upto(body, fi, total, nl):       # body, fillers, then the tail record ending the file at `total`
        n = sum(map(len, body))
        return body + _Fill(fi, False)(total - (24 + nl) - n) + [rec(60, fi, nl)]

    files, lengths = {}, {}

    def add(lines, length=None):
        name = f"T{len(files):03d}"
        files[name] = lines
        lengths[name] = sum(map(len, lines)) if length is None else length
        assert lengths[name] == sum(map(len, lines))
        return name

    ls, ll = sum(map(len, short(0))), sum(map(len, long(0)))
    assert ls < CH - 200 and CH + 64 < ll < 2 * CH - 200 and ls % 64 == ll % 64
    for t in range(68):                  # tail filler of t bytes: every length mod 64 and mod 16
        fi = len(files)
        body = (long if (t // 2) % 2 else short)(fi)
        tail = [] if t == 0 else [_filler(t)] if t % 2 == 0 else [_FILL_BODY[:t]]
        add(body + tail, (ll if (t // 2) % 2 else ls) + t)
    extra = {}
    extra["record_unterminated"] = add(short(len(files)) + [rec(60, len(files), nl=False)])
    for total, nl in ((CH, True), (CH + 1, False), (2 * CH - 1, False), (2 * CH, True)):
        fi = len(files)
        add(upto(short(fi) if total <= CH + 1 else long(fi), fi, total, nl), total)
    extra["tiny"] = add([first(len(files), nl=False)])
    assert lengths[extra["tiny"]] < 16
    extra["filler_only"] = add(_Fill(0, False)(300))
    extra["leading_newline"] = add(["\n"] + short(len(files)))
    return _case(files, chrom="chr1", lengths=lengths, tail_files=list(files)[:68], **extra)


# --------------------------------------------------------------- d. MAXLINE --
def maxline_declines():
    """Lines of more than MAXLINE bytes: each hands its cohort over."""
    def cohort(make):
        return {f"M{fi:03d}": make(fi) for fi in range(2)}

    def body(fi, a=0, b=10):
        return [_rec_prefix(24 + 3 * (k % 5), k, fi) for k in range(a, b)]

    def across(fi):
        fill, head = _Fill(fi, False), body(fi)
        n = sum(map(len, head))
        return head + fill(CH - 150 - n) + ["#" + "y" * 299 + "\n"] + body(fi, 10, 20)

    cases = {
        "record_257": _case(cohort(lambda fi: body(fi) + [_rec_prefix(257, 10, fi)] + body(fi, 11, 20)), chrom="chr1"),
        "filler_257": _case(cohort(lambda fi: body(fi) + ["#" + "y" * 256 + "\n"] + body(fi, 10, 20)), chrom="chr1"),
        "unterminated_257": _case(cohort(lambda fi: body(fi) + [_rec_prefix(257, 10, fi)[:-1]]), chrom="chr1"),
        "across_chunks_300": _case(cohort(across), chrom="chr1"),
    }
    for c in cases.values():
        c["expect"] = "hands_over"
    t = text_of(cases["across_chunks_300"]["files"]["M000"])
    at = t.index(b"#y")
    assert at == CH - 150 and t.index(b"\n", at) - at == 300
    assert len(cases["unterminated_257"]["files"]["M000"][-1]) == 257
    return cases


# --------------------------------------------------------------- e. accepts --
ACCEPT_DEPTHS = ("7", "7.", "7.5", "7.50", "007.5", "0", "0.0", "0.00", "000000000000007.25", "21474835.47")


def grammar_accepts():
    """Every form md_line accepts beside mosdepth's own, no chromosome filter,
    every mean valid (lo 0, hi 1e9).  ``int32_max``: a cohort with
    21474836.47, which the host parser keeps as int32 while the line-by-line
    restatement gives the fp64 matrix -- compared by value."""
    def lines(fi, top):
        out = [f"chr1\t{1000 * (j + 1)}\t{1000 * (j + 2)}\t{d}\n" for j, d in enumerate(ACCEPT_DEPTHS + top)]
        k = 100
        for s, e in (("000200000", "000201000"), ("0000000000300000", "000000000000301000"),
                     ("400000", "0401000")):
            out.append(f"chr1\t{s}\t{e}\t{_depth(fi, k)}\n")
            k += 1
        for c in ("#", "chr:1", "_", "a|b", "~~", "chr1_KI270706v1_random", "!\"$%&'()*+,-./;<=>?@[\\]^`{}"):
            out.append(f"{c}\t{1000 * (k + 400)}\t{1000 * (k + 401)}\t{_depth(fi, k)}\n")
            k += 1
        for s, e in ((10 ** 17, 10 ** 17 + 1000), (10 ** 17 + 1000, 10 ** 18 - 1), (10 ** 18 - 2, 10 ** 18 - 1)):
            out.append(f"chr1\t{s}\t{e}\t{_depth(fi, k)}\n")
            k += 1
        return out

    forms = _case({f"A{fi:03d}": lines(fi, ()) for fi in range(3)}, lo=0, hi=1e9)
    top = _case({f"A{fi:03d}": lines(fi, ("21474836.47",)) for fi in range(3)}, lo=0, hi=1e9, by_value=True)
    return {"forms": forms, "int32_max": top}


# -------------------------------------------------------------- f. declines --
# name -> (the bad line, what the reference does with it: "keeps" the record,
# "skips" the line, or "drops" the whole sample), as test_mdparse_cases_cpu.py
# observes it.  A negative start is an int like any other: with no window the
# reference keeps the record under the key (-5, 6000)
DECLINE_FORMS = {
    "three_decimals": ("chr1\t5000\t6000\t7.123", "keeps"),
    "no_integer_part": ("chr1\t5000\t6000\t.5", "keeps"),
    "plus_sign": ("chr1\t5000\t6000\t+7", "keeps"),
    "five_fields": ("chr1\t5000\t6000\t7.00\textra", "keeps"),
    "trailing_tab": ("chr1\t5000\t6000\t7.00\t", "keeps"),
    "exponent": ("chr1\t5000\t6000\t1e1", "keeps"),
    "carriage_return": ("chr1\t5000\t6000\t7.00\r", "keeps"),
    "start_19_digits": ("chr1\t1000000000000000000\t1000000000000001000\t7.00", "keeps"),
    "chrom_with_space": ("chr 1\t5000\t6000\t7.00", "keeps"),
    "over_int32": ("chr1\t5000\t6000\t21474836.48", "keeps"),
    "negative_depth": ("chr1\t5000\t6000\t-1.00", "skips"),
    "negative_start": ("chr1\t-5\t6000\t7.00", "keeps"),
    "three_fields": ("chr1\t5000\t6000", "skips"),
    "empty_line": ("", "skips"),
    "depth_abc": ("chr1\t5000\t6000\tabc", "drops"),
    "empty_start": ("chr1\t\t6000\t7.00", "drops"),
    "nul_in_depth": ("chr1\t5000\t6000\t7\x00.00", "drops"),
    "prefix_only": ("chr1", "skips"),
}


def grammar_declines():
    """One bad line per cohort of two files, at line 5 of 13: ``<form>-ref`` in
    the larger file (the device's reference file, MODE 0), ``<form>-other`` in
    the other (MODE 1).  ``bad``: the sample holding it; ``bad_key``: the
    (start, end) the reference reads from it, if any.  No chromosome filter,
    except prefix_only: chrom chr1, and in ``-other`` the file is the prefix
    alone, without a newline."""
    def base(fi):
        return [f"chr1\t{1000 * k}\t{1000 * (k + 1)}\t{_depth(fi, k)}\n" for k in range(1, 13)]

    cases = {}
    for name, (bad, does) in DECLINE_FORMS.items():
        f = bad.split("\t")
        key = (int(f[1]), int(f[2])) if len(f) >= 3 and does != "drops" else None
        for where in ("ref", "other"):
            big = base(0) + [f"chr1\t{1000 * k}\t{1000 * (k + 1)}\t33.00\n" for k in (20, 21, 22)]
            small = base(1)
            tgt = big if where == "ref" else small
            if name in ("start_19_digits", "prefix_only"):
                tgt.append(bad + "\n")
            elif name == "empty_line":
                tgt.insert(4, "\n")
            else:
                tgt[4] = bad + "\n"
            if name == "prefix_only" and where == "other":
                small[:] = ["chr1"]
                does_ = "empties"
            else:
                does_ = does
            files = {"D000": big, "D001": small}
            cases[f"{name}-{where}"] = _case(files, chrom="chr1" if name == "prefix_only" else None, lo=0, hi=1e9,
                                             expect="hands_over", bad="D000" if where == "ref" else "D001",
                                             bad_key=key, reference=does_)
            assert len(text_of(big)) > len(text_of(small))
    return cases


# --------------------------------------------------------- g. window / mask --
def _mask_bins(k0):
    """Bins around three masked 1 kb keys k0+10, k0+20, k0+32 (each the only
    masked key its bins can reach): ([(start, end, dropped)], the keys)."""
    k = lambda x: 1000 * (k0 + x)  # noqa: E731
    bins = [
        (k(8), k(9) + 999, False),       # ends one key below k0+10
        (k(9), k(10), True),             # its end is exactly the masked key
        (k(11), k(12), False),           # starts one key above
        (k(18), k(19) + 999, False),
        (k(20) + 999, k(21) + 999, True),   # its start floors to the masked key
        (k(21), k(22), False),
        (k(26), k(31), False),           # 5 kb bins: the masked key strictly inside the middle one
        (k(30), k(35), True),
        (k(33), k(38), False),
    ]
    return bins, {k0 + 10, k0 + 20, k0 + 32}


def window_mask_edges():
    """Cohorts at the edges of the window test (e >= wstart and s <= wend) and
    of the 1 kb repeat-mask test.  ``kept`` / ``dropped``: the (start, end)
    keys the reference must and must not return."""
    def case(bins, chrom_of=lambda j: "chr1", **kw):
        files = {f"W{fi:03d}": [f"{chrom_of(j)}\t{s}\t{e}\t{_depth(fi, j)}\n" for j, (s, e, _) in enumerate(bins)]
                 for fi in range(3)}
        return _case(files, lo=0, hi=1e9, kept=[(s, e) for s, e, d in bins if not d],
                     dropped=[(s, e) for s, e, d in bins if d], **kw)

    def window(ws, we):
        bins = [(ws - 1001, ws - 1, True), (ws - 1000, ws, False), (we, we + 1000, False), (we + 1, we + 1001, True)]
        if we - ws >= 4000:
            bins += [(ws + 1000, ws + 2000, False)]
        bins += [(we + 5000, we + 6000, True)]
        if ws >= 7000:
            bins += [(ws - 6000, ws - 5000, True)]
        return sorted(b for b in bins if b[0] >= 0)

    cases = {}
    windows = {"window": (50000, 80000), "window_point": (60000, 60000), "window_from_zero": (0, 5000)}
    for name, (ws, we) in windows.items():
        bins = window(ws, we)
        if ws == 0:
            bins = sorted(bins + [(0, 0, False), (0, 1000, False)])
        cases[name] = case(bins, chrom="chr1", start=ws, end=we)
    # the mask alone, under chr1's raw prefix: chr10's lines pass it and have a mask of their own
    b1, m1 = _mask_bins(100)
    b10, m10 = _mask_bins(300)
    n1 = len(b1)
    # (a key of one chromosome's kept bins masked on the others only drops nothing)
    cases["mask_prefix"] = case(b1 + b10, chrom="chr1", chrom_of=lambda j: "chr1" if j < n1 else "chr10",
                                excluded={"chr1": m1 | {308, 311}, "chr10": m10 | {108, 111}, "chr2": {108, 111, 308}})
    # no chromosome filter: chr1, chr2, chr10 and the bare names 1, 2, 10 under a mask keyed chr*
    names = ("chr1", "chr2", "chr10", "1", "2", "10")
    bins, ex = [], {"chr1": set(), "chr2": set(), "chr10": set()}
    for t, nm_ in enumerate(names):
        b, m = _mask_bins(1000 * (t + 1))
        bins += b
        ex["chr" + nm_.replace("chr", "")] |= m
    # a key masked on another chromosome only does not drop a bin
    ex["chr2"] |= {1008, 1011}
    ex["chr1"] |= {2008, 3011, 6011}
    ex["chr10"] |= {4008, 1011}
    cases["mask_names"] = case(bins, excluded=ex, chrom_of=lambda j: names[j // n1])
    # window and mask together
    bw = window(150000, 190000)
    bm, mm = _mask_bins(150)
    cases["window_and_mask"] = case(sorted(bw + bm), chrom="1", start=150000, end=190000, excluded={"chr1": mm})
    return cases


# ----------------------------------------------------------- h. VT after LF --
VT_CHUNKS = (0, 3, 5)


def vt_after_newline():
    """chrom chr1.  Filler lines that begin with 0x0B placed so that "\\n\\x0b"
    lies inside one aligned 32-bit word, in the first chunk and again several
    chunks later, records after each: the newline count per chunk must be the
    count of newline bytes.  ``pairs``: the byte offsets of those newlines."""
    files, pairs = {}, []
    for fi in range(2):
        fill, lines, pos, pairs, k = _Fill(fi, False), [], 0, [], 0
        for c in VT_CHUNKS:
            for j, (r, vts) in enumerate(((0, 1), (1, 1), (2, 1), (0, 3), (1, 2))):
                # the newline that ends a 24-byte record at an offset = r mod 4, the filler's 0x0B bytes behind it
                at = CH * c + 1024 + 256 * j
                at += (r - (at + 24)) % 4
                lines += fill(at - pos)
                lines += [_rec_prefix(24, k, fi), "\x0b" * vts + "#vt\n"]
                pairs.append(at + 24)
                pos = at + 25 + vts + 4
                k += 1
                for _ in range(3):
                    lines.append(_rec_prefix(24 + k % 9, k, fi))
                    pos += len(lines[-1])
                    k += 1
        lines += fill(CH * (VT_CHUNKS[-1] + 2) + 100 - pos)
        lines.append(_rec_prefix(24, k, fi))
        files[f"V{fi:03d}"] = lines
    return _case(files, chrom="chr1", pairs=pairs)


@functools.lru_cache(maxsize=None)
def device_cases():
    """name -> case, every case the device parser must read itself (built once:
    read only)."""
    cases = {"chunk_sweep": chunk_sweep(), "chunk_sweep_records": chunk_sweep(records=True),
             "segment_sweep": segment_sweep(), "file_tails": file_tails(), "vt_after_newline": vt_after_newline()}
    cases.update({f"accepts_{k}": v for k, v in grammar_accepts().items()})
    cases.update({f"edges_{k}": v for k, v in window_mask_edges().items()})
    return cases


@functools.lru_cache(maxsize=None)
def handover_cases():
    """name -> case, every case that hands over: a line over MAXLINE bytes, or
    one bad line (DECLINE_FORMS)."""
    cases = {f"maxline_{k}": v for k, v in maxline_declines().items()}
    cases.update({f"declines_{k}": v for k, v in grammar_declines().items()})
    return cases
