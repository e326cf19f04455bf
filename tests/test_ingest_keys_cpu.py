"""What the inputs of the device ingest's general key mode mean (tests/
keys_cases.py): for every case the host C++ parser equals the line-by-line
restatement of the reference, so the GPU tests' expected matrices (the host
parser's) are the reference's last-wins results.  And the host side of the
key-mode switch: the exception hierarchy and the config value."""
import numpy as np
import pytest

from grid_amd.utils import ingest_device
from grid_amd.utils import normalize_mosdepth as nm
from tests import keys_cases
from tests.test_ingest_cpu import _cohort


def _native_vs_py(tmp_path, case, lo=20, hi=100):
    d = _cohort(tmp_path, case["files"])
    inds = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
    inds = {k: inds[k] for k in case["files"]}
    args = (inds, d, case.get("chrom"), None, None, case.get("excluded") or {}, lo, hi, 2)
    a, b = nm.ingest_native(*args), nm.ingest_py(*args)
    assert a[0] == b[0] and a[1] == b[1]
    assert a[2].shape == b[2].shape and np.array_equal(a[2], b[2])
    return a


@pytest.mark.parametrize("name", sorted(keys_cases.small_cases()))
def test_small_cases_native_equals_py(tmp_path, name):
    a = _native_vs_py(tmp_path, keys_cases.small_cases()[name])
    assert len(a[0]) >= 2 and a[2].shape[1] > 100


def test_repeats_change_the_matrix(tmp_path):
    """The repeats of the cases are visible: without its decoy lines a cohort
    gives another matrix (so a first-wins or any-wins placement fails them)."""
    case = keys_cases.small_cases()["decoy_after"]
    a = _native_vs_py(tmp_path, case)
    plain = {k: [ln for ln in v if not ln.startswith("chr10")] for k, v in case["files"].items()}
    (tmp_path / "plain").mkdir()
    b = _native_vs_py(tmp_path / "plain", dict(case, files=plain))
    assert a[1] != b[1]                                   # the decoys' bins past chr1's last are columns
    sa, sb = set(a[1]), set(b[1])
    ja = [j for j, r in enumerate(a[1]) if r in sb]
    jb = [j for j, r in enumerate(b[1]) if r in sa]
    assert not np.array_equal(a[2][:, ja], b[2][:, jb])   # and the decoys' depths won


def test_distances_and_pipelined_cases_native_equals_py(tmp_path):
    case, gaps = keys_cases.distances_case()
    assert gaps["line"] == 1 and gaps["64B"] >= 2 and gaps["16KiB"] > 400 and gaps["1MB"] > 25_000
    (tmp_path / "a").mkdir()
    a = _native_vs_py(tmp_path / "a", case, lo=0, hi=1e9)
    assert a[2].shape == (1, 50_000)
    (tmp_path / "b").mkdir()
    b = _native_vs_py(tmp_path / "b", keys_cases.pipelined_case())
    assert len(b[0]) == 8


@pytest.mark.parametrize("name", sorted(keys_cases.decline_cases()))
def test_decline_cases_read_on_the_host(tmp_path, name):
    case = keys_cases.decline_cases()[name]
    d = _cohort(tmp_path, case["files"])
    inds = nm.map_mosdepth_files_to_samples(d, list(case["files"]))
    got = nm.ingest(inds, d, None, None, None, {}, 20, 100, 2)
    exp = nm.ingest_py(inds, d, None, None, None, {}, 20, 100, 2)
    assert got[0] == exp[0] and got[1] == exp[1] and np.array_equal(got[2], exp[2])


def test_key_mode_exceptions_and_values(tmp_path):
    assert issubclass(ingest_device.DeviceIngestKeys, ingest_device.DeviceIngestUnsupported)
    assert ingest_device.KEY_MODES == ("strict", "general")
    assert nm.DEVICE_KEYS == ("auto", "strict", "general")
    for v in nm.DEVICE_KEYS:
        assert nm.check_device_keys(v) == v
    for bad in ("", "Auto", "last", None, 1, True):
        with pytest.raises(ValueError, match="device_keys"):
            nm.check_device_keys(bad)
    with pytest.raises(ValueError, match="device_keys"):
        nm.ingest({}, tmp_path, None, None, None, {}, 20, 100, 1, device_keys="last-wins")
    with pytest.raises(ValueError, match="keys"):
        ingest_device.ingest_device(None, [], None, None, {}, 20, 100, keys="auto")


def test_bad_device_keys_is_a_config_error(tmp_path, capsys):
    """mosdepth.normalize.device_keys outside auto / strict / general: the
    step reports a config error and returns, as for its other bad values."""
    (tmp_path / "samples.txt").write_text("A\n")
    cfg = {"samples_file": str(tmp_path / "samples.txt"), "output_dir": str(tmp_path / "out"),
           "mosdepth": {"work_dir": str(tmp_path), "normalize": {"output_file_prefix": "n", "device_keys": "fast"}}}
    assert nm.normalize_mosdepth(cfg, None) is None
    out = capsys.readouterr().out
    assert "Config error" in out and "device_keys" in out
    assert not (tmp_path / "out").exists()
