#!/usr/bin/env python3
"""Generate tests/golden/g8_phase.json by running the REFERENCE implementation
(caterer-z-t/GRiD, read-only at /root/reference) on every case of
tests/phase_cases.py: hi_inference._run_phasing and _compute_imp.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_phase.py

Per case the file holds the name, n, the mean as a hex float ("nan" for a NaN)
and the SHA-256 digests of hap [2n] and imp [2n] (tests/phase_ops.py digest).
pysam is stubbed as in make_golden.py.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path
from unittest.mock import MagicMock

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent

sys.modules.setdefault("pysam", MagicMock())
sys.path.insert(0, str(REF))
sys.path.insert(0, str(HERE.parent.parent))

from rich.console import Console  # noqa: E402

import grid.cli  # noqa: E402
from grid.utils import hi_inference as ref_hi  # noqa: E402

from tests import phase_cases  # noqa: E402
from tests.phase_ops import digest, mean_hex  # noqa: E402

CONSOLE = Console(theme=grid.cli.grid_theme, quiet=True)

HEADER = ("hi_inference._run_phasing / _compute_imp of the reference on tests/phase_cases.py.  hap_sha256 / "
          "imp_sha256: SHA-256 of the little-endian float64 bytes of hap [2n] / imp [2n] (imp as i0, i1 per "
          "sample), every NaN first replaced by the one bit pattern 0x7ff8000000000000 -- the reference and the "
          "kernels both produce the default quiet NaN, and a NaN irr would carry its own payload.  mean: hex "
          "float, 'nan' for a NaN.")


def main():
    out = []
    for c in phase_cases.CASES:
        hap, mean = ref_hi._run_phasing(list(c.irr), c.hn, c.min_nbr, c.iters, CONSOLE)
        imp = [x for i in range(c.n) for x in ref_hi._compute_imp(i, hap, c.hn, mean)]
        out.append({"name": c.name, "n": c.n, "mean": mean_hex(mean), "hap_sha256": digest(hap),
                    "imp_sha256": digest(imp)})
    (HERE / "g8_phase.json").write_text(json.dumps({"header": HEADER, "cases": out}, indent=1) + "\n")
    print(f"g8_phase: {len(out)} cases")


if __name__ == "__main__":
    main()
