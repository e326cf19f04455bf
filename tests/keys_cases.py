"""Cohorts whose files repeat a (start, end) key or list keys out of order --
the inputs of the device ingest's general key mode (test_gpu_ingest_keys.py)
and of the CPU tests that pin what they mean (test_ingest_keys_cpu.py: the
host parser against the line-by-line restatement of the reference).

The reference keys a record by (start, end) alone and filters lines with a
raw ``startswith(chrom)``: under ``chrom: chr1`` the lines of chr10..chr19 are
kept too, their bins repeat chr1's coordinates, and the last kept line of a
key wins.  Every repeat here carries a depth of its own, so which line won
shows in the matrix."""
import numpy as np

from tests.test_ingest_cpu import _rand_lines


def _depth(line, d):
    """The line with another depth text."""
    return line.rsplit("\t", 1)[0] + f"\t{d}\n"


def _chrom(line, c):
    return c + "\t" + line.split("\t", 1)[1]


def _redo(rng, lines, chrom=None):
    """The same bins with fresh depths (on another chromosome: decoy lines)."""
    out = [_depth(ln, f"{rng.uniform(5.0, 120.0):.2f}") for ln in lines]
    return [_chrom(ln, chrom) for ln in out] if chrom else out


def small_cases():
    """name -> dict(files: {sample: lines}, chrom, excluded).  2-4 files of
    800-3,000 lines; the reference file (most text) is named in the comments."""
    rng = np.random.default_rng(3)
    base = _rand_lines(rng, 800)           # the `unsorted` and `dup` inputs of test_gpu_ingest.py
    cases = {
        "unsorted": dict(files={"A": [base[5]] + base[:5] + base[6:], "B": base}),
        "dup": dict(files={"A": base, "B": base[:100] + [base[50]] + base[100:]}),
    }
    rng = np.random.default_rng(31)

    def cohort(n, nfiles):
        return [_rand_lines(rng, n) for _ in range(nfiles)]

    # decoys AFTER the chr1 lines: the decoy wins; 3 decoy bins past chr1's last are new keys
    fs = {}
    for i, lines in enumerate(cohort(2000, 3)):
        decoy = _redo(rng, lines[100:400], "chr10") + _redo(rng, _rand_lines(rng, 2003)[2000:], "chr10")
        fs[f"S{i}"] = lines + decoy + ["chr2\t0\t1000\t50.00\n"]
    cases["decoy_after"] = dict(files=fs, chrom="chr1")

    # the same key three times, far apart and adjacent
    fs = {}
    for i, lines in enumerate(cohort(1500, 2)):
        out = list(lines)
        for j in (10, 700, 1499):
            out.insert(min(j + 200, len(out)), _redo(rng, [lines[j]])[0])
            out.append(_redo(rng, [lines[j]])[0])
        out += _redo(rng, [lines[3]]) + _redo(rng, [lines[3]])      # adjacent repeats
        fs[f"S{i}"] = out
    cases["triple"] = dict(files=fs)

    # a last repeat with depth 0.00 does not displace the earlier kept line
    fs = {}
    for i, lines in enumerate(cohort(1200, 3)):
        out = list(lines)
        for j in range(50, 1200, 97):
            out.append(_depth(lines[j], "0.00"))
        out.insert(600, _depth(lines[20], "0.00"))
        fs[f"S{i}"] = out
    cases["last_zero"] = dict(files=fs)

    # a last repeat masked on ITS OWN chromosome only (chr10's mask) does not
    # displace chr1's line; a decoy whose bin is masked on chr1 only wins over nothing
    fs = {}
    for i, lines in enumerate(cohort(1000, 3)):
        fs[f"S{i}"] = lines + _redo(rng, lines[200:260], "chr10")
    cases["last_masked"] = dict(files=fs, chrom="chr1",
                                excluded={"chr10": set(range(210, 231)), "chr1": {240, 241, 500}})

    # repeats in a file that is not the reference file (R: most text, no repeat)
    ref = _rand_lines(rng, 3000)
    other = _redo(rng, ref[:2000])
    other = other + _redo(rng, other[5:400:7]) + _redo(rng, other[1990:2000])
    cases["dup_nonref"] = dict(files={"O": other, "R": ref, "P": _redo(rng, ref[:2500])})

    # lines shifted against the reference's: the line -> K-index map misses, the binary search runs
    ref = _rand_lines(rng, 2500)
    sh = _redo(rng, ref[7:2400])
    sh = sh[:900] + _redo(rng, sh[100:130]) + sh[900:] + _redo(rng, sh[:40])
    cases["shifted"] = dict(files={"R": ref + _redo(rng, ref[40:60]), "S": sh})

    # keys with start >= 2^32 (two radix sorts over the whole int64 range)
    big = [f"chr1\t{(1 << 32) + i * 1000}\t{(1 << 32) + (i + 1) * 1000}\t{rng.uniform(5.0, 120.0):.2f}\n"
           for i in range(400)]
    huge = [f"chr1\t{10 ** 17 + i}\t{10 ** 17 + i + 7}\t{rng.uniform(20.0, 90.0):.2f}\n" for i in range(5)]
    fs = {}
    for i, lines in enumerate(cohort(800, 2)):
        b = _redo(rng, big) + _redo(rng, huge)
        fs[f"S{i}"] = b[200:] + lines + b[:200] + _redo(rng, b[150:250]) + _redo(rng, lines[:30])
    cases["big_start"] = dict(files=fs)
    return cases


def distances_case():
    """One file of ~50,000 lines (~80 parse chunks of 16 KiB, ~30 bytes a
    line) with repeats 1 line apart (one thread parses both), ~64 B apart
    (neighbouring segments), ~16 KiB apart (neighbouring chunks) and ~1 MB
    apart."""
    rng = np.random.default_rng(41)
    lines = _rand_lines(rng, 50_000, lo=20.0, hi=100.0)
    nbytes = sum(len(x) for x in lines) / len(lines)
    gaps = {"line": 1, "64B": max(2, int(round(64 / nbytes))), "16KiB": int(16384 / nbytes), "1MB": int(1e6 / nbytes)}
    ins = []                                  # (position in the original list, line)
    for k, gap in enumerate(gaps.values()):
        for t in range(12):
            j = 100 + 37 * k + 1100 * t
            ins.append((j + gap, _redo(rng, [lines[j]])[0]))
            if t % 3 == 0:                    # and once more the same distance on: three of a key
                ins.append((j + 2 * gap, _redo(rng, [lines[j]])[0]))
    out = list(lines)
    for pos, ln in sorted(ins, key=lambda x: -x[0]):
        out.insert(pos, ln)
    return dict(files={"D": out}), gaps


def pipelined_case():
    """8 files of 5,000 lines with a chr10 decoy tail (BGZF in the GPU test:
    the pipelined batches), zero-depth bins per file."""
    rng = np.random.default_rng(51)
    base = _rand_lines(rng, 5000)
    fs = {}
    for i in range(8):
        lines = _redo(rng, base)
        for j in rng.choice(len(lines), 40, replace=False):
            lines[j] = _depth(lines[j], "0.00")
        tail = _redo(rng, base[:600], "chr10")
        for j in rng.choice(len(tail), 10, replace=False):
            tail[j] = _depth(tail[j], "0.00")
        fs[f"S{i:03d}"] = lines + tail + _redo(rng, _rand_lines(rng, 5004)[5000:], "chr10")
    return dict(files=fs, chrom="chr1")


def decline_cases():
    """Still outside the device path in general mode."""
    rng = np.random.default_rng(3)
    base = _rand_lines(rng, 800)
    return {
        # each file holds a key the other lacks: outside K whichever is larger
        "extra_key": dict(files={"A": base[:-2] + [base[-1]] + [base[3]], "B": base[:-1] + [base[4]]}),
        "exotic": dict(files={"A": base + [base[3]], "B": base[:10] + ["chr1\t9999000\t9999100\t3e1\n"] + base[10:]}),
    }
