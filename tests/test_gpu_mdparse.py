"""The device mosdepth parse (grid_amd/csrc/mosdepth_dev.hip: k_md_count,
k_md_scan, k_md_parse) on text placed at its own edges (tests/
mdparse_cases.py; what every case means is settled without a GPU in
test_mdparse_cases_cpu.py): records at every offset around a chunk boundary,
on every segment and word residue, files ending at every length, every form
the grammar accepts, the window and mask edges -- the device matrix equals the
host parser's bit for bit, in both key modes, and the device never hands such
a cohort over.  A line over 256 bytes or outside the grammar always does, and
``ingest`` then gives the host result.  And the line numbers themselves, which
the matrix does not show: the reference pass's line -> key map against the
text's own line count and record lines."""
import gzip

import numpy as np
import pytest

from grid_amd import _abi
from grid_amd.device import release_ingest_buffers
from grid_amd.utils import ingest_device
from grid_amd.utils import normalize_mosdepth as nm
from tests import mdparse_cases as mc
from tests.test_gpu_ingest import SPLITS, _dev_vs_host
from tests.test_ingest_cpu import _bgzf

pytestmark = pytest.mark.gpu

DEVICE, HANDOVER = mc.device_cases(), mc.handover_cases()


@pytest.fixture(scope="module")
def dev():
    import torch
    d = _abi.Device(0)
    d.set_stream(torch.cuda.current_stream())
    return d


def _write(tmp_path, case, pack=lambda data: gzip.compress(data, 1), only=None):
    d = tmp_path / "md"
    d.mkdir()
    for name, lines in case["files"].items():
        if only is None or name in only:
            (d / f"{name}.regions.bed.gz").write_bytes(pack(mc.text_of(lines)))
    return d


def _kw(case):
    return dict(chrom=case["chrom"], start=case["start"], end=case["end"], excluded=case["excluded"],
                lo=case["lo"], hi=case["hi"])


def _values(q):
    q = q.numpy() if isinstance(q, _abi.DevBuf) else np.asarray(q)
    return q if q.dtype == np.float64 else np.where(q == _abi.MISSING, np.nan, q / 100.0)


@pytest.mark.parametrize("keys", ingest_device.KEY_MODES)
@pytest.mark.parametrize("name", sorted(DEVICE))
def test_device_reads_the_case(dev, tmp_path, name, keys):
    """No hand-over (``_ingest_dev`` raises on one), and the host parser's ids,
    regions and matrix bit for bit."""
    case = DEVICE[name]
    a = _dev_vs_host(dev, _write(tmp_path, case), list(case["files"]), keys=keys, **_kw(case))
    assert len(a[0]) >= 2 and len(a[1]) >= 2


@pytest.mark.parametrize("split", ["gpu", "cpu"])
@pytest.mark.parametrize("name", ["chunk_sweep", "chunk_sweep_records", "file_tails"])
def test_bgzf_text_inflated_on_either_side(dev, tmp_path, monkeypatch, name, split):
    """The same text as BGZF members, inflated in HBM by the GPU or copied there
    from the host threads: the parse reads what either leaves in d_text."""
    monkeypatch.setattr(ingest_device._Split, "plan", SPLITS[split])
    case = DEVICE[name]
    a = _dev_vs_host(dev, _write(tmp_path, case, pack=_bgzf), list(case["files"]), **_kw(case))
    assert len(a[0]) >= 2


@pytest.mark.parametrize("keys", ingest_device.KEY_MODES)
@pytest.mark.parametrize("name", sorted(HANDOVER))
def test_line_outside_the_limits_hands_over(dev, tmp_path, name, keys):
    """A line over 256 bytes (even one the prefix test would skip) or outside
    md_line's grammar: never parsed or skipped on the device."""
    case = HANDOVER[name]
    d = _write(tmp_path, case)
    m = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
    inds = {k: m[k] for k in case["files"]}
    args = (inds, d, case["chrom"], case["start"], case["end"], case["excluded"], case["lo"], case["hi"], 2)
    with pytest.raises(ingest_device.DeviceIngestUnsupported, match="outside the mosdepth grammar") as e:
        nm._ingest_dev(dev, *args, keys=keys)
    assert not isinstance(e.value, ingest_device.DeviceIngestKeys)
    got = nm.ingest(*args, dev=dev, device_keys=keys)
    exp = nm.ingest(*args)
    assert got[0] == exp[0] and list(got[1]) == list(exp[1])
    assert np.asarray(got[2]).dtype == np.asarray(exp[2]).dtype
    assert np.array_equal(_values(got[2]), _values(exp[2]), equal_nan=True)
    assert dev.cached_bytes() == 0


@pytest.mark.parametrize("keys", ingest_device.KEY_MODES)
@pytest.mark.parametrize("name", ["chunk_sweep", "chunk_sweep_records", "segment_sweep", "vt_after_newline"])
def test_line_numbers_of_the_reference_pass(dev, tmp_path, name, keys):
    """``keys_only`` on one file: ref_nlines is the text's line count, kidx is
    >= 0 exactly at the 0-based line numbers of the records the prefix keeps
    (their K index, in order) and -1 elsewhere, K is their (start, end) --
    k_md_count's newlines per chunk and k_md_parse's per-segment counts number
    the same lines."""
    case = DEVICE[name]
    sample = next(iter(case["files"]))
    d = _write(tmp_path, case, only=[sample])
    prefix = nm.norm_chrom(case["chrom"]) if case["chrom"] else None
    K, kidx, nlines = ingest_device.ingest_device(dev, [str(d / f"{sample}.regions.bed.gz")], prefix, None, {},
                                                  case["lo"], case["hi"], keys_only=True, keys=keys)
    release_ingest_buffers(dev)
    n, kept = mc.ref_lines(mc.text_of(case["files"][sample]), prefix)
    assert nlines == n and len(kidx) == n
    assert np.flatnonzero(kidx >= 0).tolist() == [i for i, _, _ in kept]
    assert kidx[kidx >= 0].tolist() == list(range(len(kept)))
    assert K.tolist() == [[s, e] for _, s, e in kept]
