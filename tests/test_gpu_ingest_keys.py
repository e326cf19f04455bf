"""The device ingest's general key mode (ingest_device.py ``keys="general"``:
grid_md_parse_ref_general's sorted unique columns, grid_md_parse_map_general's
tag and resolve passes) against the host parser on cohorts that repeat
(start, end) keys or list them out of order (tests/keys_cases.py; that the
host parser is the reference's last-wins result on them is shown without a
GPU in test_ingest_keys_cpu.py): the same ids, regions and matrix, bit for
bit.  Then the switch above it: ``ingest(device_keys=)``, the pipeline on the
golden cohort g1 and the distributed drop-in, none of which leaves the device
for g1's decoy lines any more."""
import os

import numpy as np
import pytest
import yaml

from grid_amd import _abi
from grid_amd.utils import ingest_device
from grid_amd.utils import normalize_mosdepth as nm
from tests import keys_cases
from tests.test_gpu_dist_wgs import FILES, _content, _run, _stage
from tests.test_ingest_cpu import _bgzf, _cohort

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    import torch
    d = _abi.Device(0)
    d.set_stream(torch.cuda.current_stream())
    return d


def _general_vs_host(dev, d, samples, chrom=None, excluded=None, lo=20, hi=100):
    m = nm.map_mosdepth_files_to_samples(d, samples)
    inds = {s: m[s] for s in samples if s in m}
    ex = excluded or {}
    a = nm._ingest_dev(dev, inds, d, chrom, None, None, ex, lo, hi, 4, keys="general")
    b = nm.ingest_native(inds, d, chrom, None, None, ex, lo, hi, 4)
    assert a[0] == b[0], (a[0], b[0])
    assert a[1] == b[1]
    qa = a[2].numpy() if isinstance(a[2], _abi.DevBuf) else a[2]
    assert qa.shape == b[2].shape and np.array_equal(qa, b[2])
    return a[0], a[1], qa


def _golden(name):
    c = yaml.safe_load(open(os.path.join(G, name, "config.yaml")))
    src = os.path.join(G, name, "inputs")
    samples = [s.strip() for s in open(os.path.join(src, "samples.txt")) if s.strip()]
    ex = nm.load_repeat_mask(os.path.join(src, "mask.bed"))
    n = c["mosdepth"]["normalize"]
    return (os.path.join(src, "mosdepth"), samples, c.get("chrom"), c.get("start_bp"), c.get("end_bp"), ex,
            n["min_depth"], n["max_depth"])


def test_g1_golden_on_the_device(dev):
    """g1 (plain gzip): chr10 decoy lines before the chr1 lines, 30 keys
    collide, 3 are new.  Strict mode declines it; general mode gives the host
    parser's matrix."""
    d, samples, chrom, _, _, ex, lo, hi = _golden("g1")
    inds = nm.map_mosdepth_files_to_samples(d, samples)
    with pytest.raises(ingest_device.DeviceIngestKeys):
        nm._ingest_dev(dev, inds, d, chrom, None, None, ex, lo, hi, 2)
    ids, regions, q = _general_vs_host(dev, d, samples, chrom, ex, lo, hi)
    assert len(ids) > 10 and q.shape[1] > 100


@pytest.mark.parametrize("name", ["g1b", "g1c"])
def test_goldens_without_repeats_are_the_same_in_both_modes(dev, name):
    d, samples, chrom, start, end, ex, lo, hi = _golden(name)
    m = nm.map_mosdepth_files_to_samples(d, samples)
    inds = {s: m[s] for s in samples if s in m}
    s = nm._ingest_dev(dev, inds, d, chrom, start, end, ex, lo, hi, 2)
    g = nm._ingest_dev(dev, inds, d, chrom, start, end, ex, lo, hi, 2, keys="general")
    assert s[0] == g[0] and s[1] == g[1]
    assert np.array_equal(s[2].numpy(), g[2].numpy())
    b = nm.ingest_native(inds, d, chrom, start, end, ex, lo, hi, 2)
    assert g[0] == b[0] and g[1] == b[1] and np.array_equal(g[2].numpy(), b[2])


@pytest.mark.parametrize("name", sorted(keys_cases.small_cases()))
def test_small_cases(dev, tmp_path, name):
    case = keys_cases.small_cases()[name]
    d = _cohort(tmp_path, case["files"])
    ids, regions, q = _general_vs_host(dev, d, list(case["files"]), case.get("chrom"), case.get("excluded"))
    assert len(ids) == len(case["files"]) and q.shape[1] > 100
    starts = [r[0] for r in regions]
    assert starts == sorted(starts)
    if name in ("unsorted", "dup"):
        # strict mode still declines them, with the key-order exception
        m = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
        with pytest.raises(ingest_device.DeviceIngestKeys):
            nm._ingest_dev(dev, {k: m[k] for k in case["files"]}, d, None, None, None, {}, 20, 100, 2)
    if name == "big_start":
        assert regions[-1][0] >= 10 ** 17 and sum(s >= 1 << 32 for s in starts) > 100


def test_repeat_distances_and_determinism(dev, tmp_path):
    """Repeats 1 line, ~64 B, ~16 KiB and ~1 MB apart in one file of ~80 parse
    chunks: one thread, neighbouring segments, neighbouring chunks, far
    workgroups.  Twice: the matrices are equal byte for byte (the result does
    not depend on the order the atomics arrive in)."""
    case, gaps = keys_cases.distances_case()
    d = _cohort(tmp_path, case["files"])
    a = _general_vs_host(dev, d, ["D"], lo=0, hi=1e9)
    b = _general_vs_host(dev, d, ["D"], lo=0, hi=1e9)
    assert a[2].shape == (1, 50_000)
    assert a[2].tobytes() == b[2].tobytes() and a[1] == b[1]


SPLITS = {
    "gpu": lambda self, files, text, bgzf: (sorted(files), []),
    "cpu": lambda self, files, text, bgzf: ([], sorted(files)),
    "alternate": lambda self, files, text, bgzf: (sorted(files)[0::2], sorted(files)[1::2]),
}


@pytest.mark.parametrize("split", sorted(SPLITS))
def test_pipelined_batches(dev, tmp_path, monkeypatch, split):
    """8 BGZF files with a decoy tail in batches of a file or two: under the
    gpu split the pipelined batches (_Async.batch: tag and resolve pass back to
    back before the batch's `done` event), under cpu the synchronous loop with
    host-inflated text, under alternate both.  A truncated file is dropped."""
    monkeypatch.setattr(ingest_device, "BATCH_IN", 48 << 10)
    monkeypatch.setattr(ingest_device, "STAGE", 64 << 10)
    monkeypatch.setattr(ingest_device._Split, "plan", SPLITS[split])
    case = keys_cases.pipelined_case()
    d = tmp_path / "md"
    d.mkdir()
    for name, lines in case["files"].items():
        (d / f"{name}.regions.bed.gz").write_bytes(_bgzf("".join(lines).encode()))
    good = (d / "S002.regions.bed.gz").read_bytes()
    (d / "T000.regions.bed.gz").write_bytes(good[: len(good) // 2])     # truncated: dropped
    samples = sorted(case["files"])
    samples = samples[:3] + ["T000"] + samples[3:]
    calls = []
    orig = ingest_device._Async.batch

    def counted(self, *a, **k):
        calls.append(self.parse_map)
        return orig(self, *a, **k)

    monkeypatch.setattr(ingest_device._Async, "batch", counted)
    ids, regions, q = _general_vs_host(dev, d, samples, case["chrom"])
    assert len(ids) == 8 and "T000" not in ids
    # a batch whose files all go to the GPU is pipelined (under `alternate` a one-file batch is)
    assert set(calls) <= {"grid_md_parse_map_general"}, calls
    assert len(calls) >= 2 if split == "gpu" else (not calls or split == "alternate"), calls


@pytest.mark.parametrize("name", sorted(keys_cases.decline_cases()))
def test_general_mode_still_declines(dev, tmp_path, name):
    """A key outside K and a line outside the grammar hand over in general
    mode too -- not as a key-order case -- and ingest() reads the cohort on the
    host, releasing the device ingest's buffers and staging."""
    case = keys_cases.decline_cases()[name]
    d = _cohort(tmp_path, case["files"])
    m = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
    inds = {k: m[k] for k in case["files"]}
    why = "a key outside K" if name == "extra_key" else "outside the mosdepth grammar"
    with pytest.raises(ingest_device.DeviceIngestUnsupported, match=why) as e:
        nm._ingest_dev(dev, inds, d, None, None, None, {}, 20, 100, 2, keys="general")
    assert not isinstance(e.value, ingest_device.DeviceIngestKeys)
    for mode in ("auto", "general"):
        got = nm.ingest(inds, d, None, None, None, {}, 20, 100, 2, dev=dev, device_keys=mode)
        exp = nm.ingest_py(inds, d, None, None, None, {}, 20, 100, 2)
        assert got[0] == exp[0] and got[1] == exp[1]
        assert np.array_equal(np.asarray(got[2]), np.asarray(exp[2]))
        assert dev.cached_bytes() == 0 and ingest_device.staging_bytes() == 0


def test_ingest_switch_on_g1(dev, capsys):
    """ingest(dev=) on g1.  auto: the strict attempt declines, one warning, the
    general mode's device matrix.  strict: today's hand-over to the host
    parser.  general: no strict attempt."""
    d, samples, chrom, _, _, ex, lo, hi = _golden("g1")
    inds = nm.map_mosdepth_files_to_samples(d, samples)
    exp = nm.ingest_native(inds, d, chrom, None, None, ex, lo, hi, 2)
    capsys.readouterr()
    for mode in ("auto", "general"):
        got = nm.ingest(inds, d, chrom, None, None, ex, lo, hi, 2, dev=dev, device_keys=mode)
        out = capsys.readouterr().out
        assert isinstance(got[2], _abi.DevBuf)
        assert got[0] == exp[0] and got[1] == exp[1] and np.array_equal(got[2].numpy(), exp[2])
        assert "using the host parser" not in out
        assert out.count("repeated or unsorted keys; using the general key mode") == (1 if mode == "auto" else 0)
    got = nm.ingest(inds, d, chrom, None, None, ex, lo, hi, 2, dev=dev, device_keys="strict")
    out = capsys.readouterr().out
    assert "device mosdepth parser: the reference file's keys are not strictly increasing; using the host parser" \
        in out and "general key mode" not in out
    assert isinstance(got[2], np.ndarray)
    assert got[0] == exp[0] and got[1] == exp[1] and np.array_equal(got[2], exp[2])
    assert dev.cached_bytes() == 0 and ingest_device.staging_bytes() == 0


def test_g1_end_to_end_stays_on_the_device(tmp_path, capsys):
    """`grid wgs` on g1: every output file equals the reference's after gunzip,
    and step 4 never hands the cohort to the host parser."""
    from grid_amd.pipeline import run_wgs_pipeline
    c, p = _stage("g1", tmp_path)
    run_wgs_pipeline(console=None, config=p)
    out = capsys.readouterr().out
    assert "using the host parser" not in out and "using the general key mode" in out, out
    exp = os.path.join(G, "g1", "expected")
    for f in FILES:
        assert _content(os.path.join(c["output_dir"], f)) == _content(os.path.join(exp, f)), f


def test_g1_distributed_stays_on_the_device(tmp_path):
    """g1 at world 2 on the shared GPU: rank 0's reference keys retry in general
    mode, the mode travels in the control header, every rank parses its slice
    with the tag and resolve passes -- no rank-0 fallback."""
    c, p = _stage("g1", tmp_path)
    logs = _run(2, p, tmp_path)
    assert "Failed" not in logs and "rank 0 reads the cohort" not in logs, logs
    exp = os.path.join(G, "g1", "expected")
    for f in FILES:
        assert _content(os.path.join(c["output_dir"], f)) == _content(os.path.join(exp, f)), (f, logs)
