"""Hand-framed normalised-matrix files for the device reader's tests
(tests/test_ntext_cpu.py, tests/test_gpu_ntext.py): gzip members built in
Python with the 32-byte 'GR' header of grid_amd/csrc/textio.cpp, so a test
chooses the member count, the rows per member and the deflate block type."""
import struct
import zlib

import numpy as np

MISSING = -(2 ** 31)
IMAX = 2 ** 31 - 1


def member(text, first_row, level=6):
    """One gzip member with FEXTRA 'GR' = {member size u64, first row i64}."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(text) + co.flush()
    total = 32 + len(body) + 8
    head = (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", 20) + b"GR" +
            struct.pack("<H", 16) + struct.pack("<Qq", total, first_row))
    return head + body + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def header_text(n, means, ratios):
    f = lambda v: "NA" if np.isnan(v) else f"{v:.3f}"
    return "".join(f"{n}\t{len(means)}\t" + "\t".join(f(v) for v in vals) + "\n" for vals in (means, ratios)).encode()


def token(q, rng):
    """A text the grammar accepts for hundredths q (a random spelling)."""
    if q == MISSING:
        return "NA" if rng.random() < 0.5 else "nan"
    neg, a = q < 0, abs(int(q))
    ip, fp = f"{a // 100}", f"{a % 100:02d}"
    if len(ip) < 8 and rng.random() < 0.2:
        ip = ip.rjust(int(rng.integers(len(ip), 9)), "0")          # leading zeros, up to 8 integer digits
    if a == 0 and rng.random() < 0.3:
        neg = True                                                  # "-0.00"
    return ("-" if neg else "") + ip + "." + fp


def cells(n, r, seed):
    """(tokens [n][r], expected int32 [n][r]): every cell width -- 0.00, -0.00,
    NA, nan, leading zeros, 1- to 8-digit integers, both int32 extremes."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-30000, 30000, (n, r)).astype(np.int64)
    k = rng.random((n, r))
    q[k < 0.05] = 0
    q[(k >= 0.05) & (k < 0.10)] = MISSING
    wide = (k >= 0.10) & (k < 0.16)
    q[wide] = rng.integers(-IMAX, IMAX, int(wide.sum()))
    seven = (k >= 0.16) & (k < 0.20)
    q[seven] = rng.integers(100000000, 999999999, int(seven.sum())) * rng.choice([-1, 1], int(seven.sum()))
    flat = q.reshape(-1)
    for i, v in enumerate((IMAX, -IMAX, 0, MISSING, 2000000000, -5)[: flat.size]):
        flat[(i * 7919) % flat.size] = v
    toks = [[token(v, rng) for v in row] for row in q]
    return toks, q.astype(np.int32)


def row_text(rid, scale, toks):
    return (rid + "\t" + scale + "\t" + "\t".join(toks) + "\n").encode()


def build(ids, scales, toks, rows_per_member, means, ratios, level=6):
    """File bytes and the row members' (text, first row): rows_per_member is a
    list of counts that sums to len(ids)."""
    assert sum(rows_per_member) == len(ids)
    out = [member(header_text(len(ids), means, ratios), -1, level)]
    texts, row = [], 0
    for cnt in rows_per_member:
        t = b"".join(row_text(ids[i], scales[i], toks[i]) for i in range(row, row + cnt))
        texts.append((t, row))
        out.append(member(t, row, level))
        row += cnt
    return b"".join(out), texts


def case(n, r, seed, rows_per_member=None, level=6, id_len=None):
    """A whole seeded file: (bytes, member texts, expected zq)."""
    rng = np.random.default_rng(seed + 1)
    toks, exp = cells(n, r, seed)
    if id_len is None:
        ids = [f"S{i:04d}" for i in range(n)]
    else:
        ids = [(f"{i:x}" * id_len)[:id_len] for i in range(n)]
    scales = [f"{v:.2f}" for v in rng.uniform(0, 90, n)]
    if n > 1:
        scales[1] = "NA"
    if n > 2:
        scales[2] = f"{1e300:.2f}"
    means, ratios = rng.uniform(0.5, 2, r), rng.uniform(0, 9, r)
    means[0] = np.nan
    data, texts = build(ids, scales, toks, rows_per_member or [n], means, ratios, level)
    return data, texts, exp
