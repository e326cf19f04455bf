"""The committed records bench.py reads at run time (CPU only): the PMC traffic
summary behind roofline.traffic and the CPU-baseline sweep must be in the tree
and hold what the line takes from them, or the driver's bench line silently
reports traffic / the sweep as null."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_const(name):
    src = open(os.path.join(ROOT, "bench.py")).read()
    m = re.search(rf'^{name} = "([^"]+)"', src, re.M)
    assert m, name
    return m.group(1)


def test_traffic_record_has_the_gram_kernel():
    path = os.path.join(ROOT, _bench_const("TRAFFIC_JSON"))
    tj = json.load(open(path))
    gram = _bench_const("GRAM_KERNEL")
    hits = [v for k, v in tj["kernels"].items() if k.startswith(gram)]
    assert len(hits) == 1
    # per-launch HBM bytes of the dominant kernel: fetch + write, both positive
    h = hits[0]
    assert h["fetch_bytes"] > 0 and h["write_bytes"] > 0
    assert abs(h["traffic_bytes"] - (h["fetch_bytes"] + h["write_bytes"])) <= 1e-6 * h["traffic_bytes"]


def test_cpu_sweep_record_has_the_config2_fit():
    sw = json.load(open(os.path.join(ROOT, _bench_const("CPU_SWEEP_JSON"))))
    assert sw["points"] and sw["fit_seconds_per_unit"]
    assert set(sw["fit_seconds_per_unit"]) == set(sw["fit_units"])


def test_plain_and_full_options_exist():
    """A plain run times the headline only; --full and --dump-outputs are
    options of the command line."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert re.search(r'add_argument\("--full", action="store_true"', src)
    assert re.search(r'add_argument\("--dump-outputs"', src)
    # every measurement beside the headline is gated by --full
    for leg in ("inflate_roofline(files_paths", "cpu_baseline(qh", "run_workload(args, 50_000"):
        at = src.index(leg)
        gate = src.rfind("\n    if ", 0, at)
        assert "args.full" in src[gate:at], leg


def test_dump_files_outputs_parses_the_output_files(tmp_path):
    """--dump-outputs from files: the arrays hold what the output files say,
    rows in samples order, the normalised rows at the seeded columns."""
    import gzip

    import numpy as np

    import bench
    ids = ["S0", "S1", "S2"]
    out = tmp_path / "out"
    out.mkdir()
    with gzip.open(out / "neighbors.zMax2.0.tsv.gz", "wt") as f:
        f.write("S1\t1.50\tS0\t2.50\t0.25\tS2\t3.50\t0.75\n")
        f.write("S0\t2.50\tS2\t3.50\t0.10\n")
        f.write("S2\t3.50\tS1\t1.50\t0.75\tS0\t2.50\t0.10\n")
    (out / "dipcn.tsv").write_text("Sample\tNorm_Reads\nS2\t1.25\nS0\t0.5\n")
    (out / "haploid.tsv").write_text("ID\tIRRs\thap1phased\thap2phased\thap1imp\thap2imp\n"
                                     "S0\t0.50\t0.20\t0.30\t0.21\t0.31\nS2\t1.25\t0.60\t0.65\tnan\t0.66\n")
    with gzip.open(out / "normalized.tsv.gz", "wt") as f:
        f.write("3\t5\t10.000\t11.000\t12.000\tNA\t14.000\n")
        f.write("3\t5\t1.000\t1.100\t1.200\tNA\t1.400\n")
        f.write("S0\t30.25\t0.10\t-0.20\tNA\t0.40\t0.50\n")
        f.write("S1\t31.25\t1.10\t-1.20\t1.30\t1.40\t1.50\n")
        f.write("S2\t32.25\t2.10\t-2.20\t2.30\t2.40\tNA\n")
    (out / "counts.tsv").write_text("Sample\tchr1\nS0\t1\n")
    dump = tmp_path / "dump"
    bench.dump_files_outputs(str(out), ids, str(dump))
    got = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    nan = np.nan
    eq = lambda a, b: np.array_equal(a, np.array(b, dtype=a.dtype), equal_nan=True)  # noqa: E731
    assert eq(got["neighbors_scale"], [2.5, 1.5, 3.5])
    assert eq(got["neighbors_index"], [[2, nan], [0, 2], [1, 0]])
    assert eq(got["neighbors_nbr_scale"], [[3.5, nan], [2.5, 3.5], [1.5, 2.5]])
    assert eq(got["neighbors_distance"], [[0.10, nan], [0.25, 0.75], [0.75, 0.10]])
    assert eq(got["dipcn"], [0.5, nan, 1.25])
    assert eq(got["haploid"], [[0.5, 0.2, 0.3, 0.21, 0.31], [nan] * 5, [1.25, 0.6, 0.65, nan, 0.66]])
    assert eq(got["normalized_shape"], [3, 5])
    assert eq(got["normalized_columns"], [0, 1, 2, 3, 4])          # fewer than DUMP_COLS: every column
    assert eq(got["normalized_means"], [10, 11, 12, nan, 14])
    assert eq(got["normalized_ratios"], [1, 1.1, 1.2, nan, 1.4])
    assert eq(got["normalized_rows"], [0, 1, 2, nan])
    assert eq(got["normalized_row_means"], [30.25, 31.25, 32.25, nan])
    assert eq(got["normalized_z"], [[0.1, -0.2, nan, 0.4, 0.5], [1.1, -1.2, 1.3, 1.4, 1.5], [2.1, -2.2, 2.3, 2.4, nan],
                                    [nan] * 5])


def test_gen_cohort_line_encoder_writes_the_same_text(tmp_path):
    """tools/gen_cohort's own BGZF encoder against its libdeflate path: the
    same text from both, over START/END digit counts 1 to 8 and their carries;
    every block a gzip member of 65280 bytes of text (the last one shorter)
    with the BGZF length field, then the end-of-file member."""
    import gzip
    import struct
    import subprocess
    import zlib
    gen = os.path.join(ROOT, "tools", "gen_cohort")
    assert os.path.exists(gen), "build() compiles tools/gen_cohort"
    n, m = 3, 12000
    texts = {}
    for mode, env in (("line", {}), ("libdeflate", {"GEN_COHORT_LIBDEFLATE": "1"})):
        d = tmp_path / mode
        d.mkdir()
        subprocess.run([gen, str(d), str(n), str(m), "20260821", "2", "0", "bgzf"], check=True,
                       env=dict(os.environ, **env), stderr=subprocess.DEVNULL)
        texts[mode] = [gzip.open(d / f"S{i:05d}.regions.bed.gz").read() for i in range(n)]
    assert texts["line"] == texts["libdeflate"]
    lines = texts["line"][1].split(b"\n")
    assert len(lines) == m + 1 and lines[0].startswith(b"chr1\t0\t1000\t")
    assert lines[m - 1].startswith(b"chr1\t11999000\t12000000\t")
    blob = (tmp_path / "line" / "S00001.regions.bed.gz").read_bytes()
    pos, total = 0, 0
    sizes = []
    while pos < len(blob):
        assert blob[pos:pos + 4] == b"\x1f\x8b\x08\x04" and blob[pos + 12:pos + 16] == b"BC\x02\x00"
        bsize = struct.unpack("<H", blob[pos + 16:pos + 18])[0] + 1
        member = blob[pos:pos + bsize]
        text = zlib.decompress(member[18:-8], -15)
        crc, isize = struct.unpack("<II", member[-8:])
        assert isize == len(text) <= 65280 and crc == zlib.crc32(text)
        sizes.append(len(text))
        total += len(text)
        pos += bsize
    assert sizes[-1] == 0 and len(sizes) > 3 and total == len(texts["line"][1])
    assert all(v == 65280 for v in sizes[:-2]) and 0 < sizes[-2] <= 65280
    # the encoder's use: about libdeflate level 1's size or less
    lib = os.path.getsize(tmp_path / "libdeflate" / "S00001.regions.bed.gz")
    assert len(blob) <= 1.1 * lib
