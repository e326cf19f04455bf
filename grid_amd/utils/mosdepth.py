"""The half of the reference's mosdepth step that needs no CRAM, pysam or
mosdepth binary (reference grid/utils/mosdepth.py): a region's coverage from a
sample's existing ``*.regions.bed.gz`` (compute_region_coverage :264-297), the
two-column coverage file compute_mosdepth writes from it (:16-105,
write_coverage_result :126-140) -- what step 6 reads as its counts -- and the
cleanup helper step 4 calls (remove_intermediate_files :300-326).  Running
mosdepth itself (step 3) is out of scope.

``compute_region_coverages`` is the step: one region (``chrom`` / ``start_bp``
/ ``end_bp``) or every region of ``mosdepth.coverage.loci_file``, for every
sample of ``samples_file`` that has a file in ``mosdepth.work_dir``.  The
files are inflated and parsed on the device (coverage_device.py: one pass over
the text serves every region); ``mosdepth.coverage.device: false`` runs the
host restatement below instead, which also takes every file the device hands
over (a line outside the canonical mosdepth grammar)."""
from __future__ import annotations

import gzip
from bisect import bisect_left
from pathlib import Path

from .utils import get_samples, log, setup_output_file


def remove_intermediate_files(work_dir, console=None, include_region_bed_gz: bool = False) -> None:
    suffixes = ["mosdepth.global.dist.txt", "mosdepth.region.dist.txt", "regions.bed.gz.csi"]
    if include_region_bed_gz:
        suffixes.append("regions.bed.gz")
    for f in Path(work_dir).glob("*"):
        if any(f.name.endswith(s) for s in suffixes):
            try:
                f.unlink()
            except Exception as e:
                log(console, f"Failed to remove intermediate file {f}: {e}", style="warning")


# ---------------------------------------------------------------------------
# compute_region_coverage (:264-297), restated for many regions in one walk of
# the file.  The reference walks the file once per region; per line it splits
# and converts all four fields BEFORE it looks at the chromosome, so a line it
# cannot read fails every region, while a depth of nan or inf fails only the
# regions it overlaps (at the final round).  Per region the sums take the
# overlapping lines in file order: region_cov += mean_cov * overlap (float *
# int, then one add), covered_bp += overlap.

def _loci_index(loci):
    """chrom -> (starts sorted, ends, columns, longest locus) of its loci."""
    by = {}
    for col, (chrom, start, end) in enumerate(loci):
        by.setdefault(chrom, []).append((start, end, col))
    out = {}
    for chrom, lst in by.items():
        lst.sort(key=lambda t: t[0])
        out[chrom] = ([t[0] for t in lst], [t[1] for t in lst], [t[2] for t in lst],
                      max(max(t[1] - t[0], 0) for t in lst))
    return out


def region_sums(regions_file, loci):
    """``loci``: (chrom, start, end) triples.  Returns (region_cov, covered_bp,
    error) lists, one entry per locus: the reference's two sums after its walk
    of ``regions_file`` for that region, and the exception its walk ends with
    (None when it reaches the end of the file)."""
    n = len(loci)
    cov, bp, err = [0.0] * n, [0] * n, [None] * n
    index = _loci_index(loci)
    try:
        with gzip.open(regions_file, "rt") as f:
            for line in f:
                r_chr, r_start, r_end, mean_cov = line.strip().split("\t")[:4]
                r_start, r_end = int(r_start), int(r_end)
                mean_cov = float(mean_cov)
                tab = index.get(r_chr)
                if tab is None:
                    continue
                starts, ends, cols, longest = tab
                # loci that start below r_end, down to those too far left to reach r_start
                j = bisect_left(starts, r_end) - 1
                hits = []
                while j >= 0 and starts[j] > r_start - longest:
                    overlap = min(ends[j], r_end) - max(starts[j], r_start)
                    if overlap > 0:
                        hits.append((cols[j], overlap))
                    j -= 1
                for col, overlap in hits:
                    if err[col] is not None:
                        continue
                    try:
                        cov[col] += mean_cov * overlap
                        bp[col] += overlap
                    except Exception as e:           # float * (an int no float holds)
                        err[col] = e
    except Exception as e:                           # gzip, decoding, a line that does not read
        err = [e if x is None else x for x in err]
    return cov, bp, err


def coverage_value(region_cov, covered_bp):
    """:297"""
    return int(round(100 * (region_cov / covered_bp))) if covered_bp > 0 else 0


def region_coverages(regions_file, loci):
    """The reference's compute_region_coverage for every locus of ``loci``: a
    list of ints, with the exception in place of the value where its call
    raises (run_mosdepth_single_cram :189 turns any into "Error")."""
    cov, bp, err = region_sums(regions_file, loci)
    out = []
    for c, b, e in zip(cov, bp, err):
        if e is None:
            try:
                e = coverage_value(c, b)
            except Exception as x:                   # round(nan), round(inf)
                e = x
        out.append(e)
    return out


def compute_region_coverage(regions_file, chrom: str, start: int, end: int) -> int:
    """:264-297 -- the average depth of [start, end) on ``chrom``, times 100,
    rounded half to even; raises what the reference raises."""
    v = region_coverages(regions_file, [(chrom, start, end)])[0]
    if isinstance(v, Exception):
        raise v
    return v


def write_coverage_results(output_file, rows) -> None:
    """``sample\\tcoverage`` lines appended to ``output_file`` (:126-140, the
    file opened once for all ``rows`` of (sample, coverage); one writer here,
    so no lock)."""
    with open(output_file, "a", newline="") as f:
        f.write("".join(f"{sample}\t{coverage}\n" for sample, coverage in rows))


def write_coverage_result(output_file, sample_name, coverage) -> None:
    """:126-140"""
    write_coverage_results(output_file, [(sample_name, coverage)])


def _coverage_config(config):
    """(loci as read_loci_file gives them, output path per locus, files per
    sample in samples-file order, the coverage section)."""
    from .hi_inference import _locus_path, read_loci_file
    from .normalize_mosdepth import map_mosdepth_files_to_samples
    md = config.get("mosdepth", {})
    cc = md.get("coverage", {}) or {}
    ftype = config.get("output_file_type", "tsv")
    output_dir = config.get("output_dir", ".")
    prefix = md.get("output_file_prefix", None)
    samples = get_samples(config["samples_file"])
    files = map_mosdepth_files_to_samples(Path(md["work_dir"]).expanduser(), samples)
    if cc.get("loci_file"):
        loci = read_loci_file(cc["loci_file"])
        if not loci:
            raise ValueError(f"loci file {cc['loci_file']}: no region")
        tmpl = cc.get("loci_output", "{output_dir}/{prefix}.{locus}.{type}")
        outs = [_locus_path(tmpl, lc, output_dir=output_dir, prefix=prefix, type=ftype) for lc in loci]
        if len(set(outs)) != len(outs):
            raise ValueError("loci_output names collide (add {index} or {start} to the template)")
    else:
        chrom, start, end = config["chrom"], int(config["start_bp"]), int(config["end_bp"])
        loci = [{"chrom": chrom, "start": start, "end": end, "gene": f"{chrom}_{start}_{end}", "index": 0}]
        outs = [Path(f"{output_dir}/{prefix}.{ftype}")]
    return loci, outs, samples, files, cc


def compute_region_coverages(config, console, comm=None):
    """The step (compute_mosdepth :16-105 from the point where a sample's
    regions file exists).  Per region one file ``Sample\\t{chrom}:{start}-{end}``
    then ``sample\\tcoverage`` rows in samples-file order (the reference's
    order at ``threads: 1``); a sample with no file, or whose file gives no
    value (the reference's "Error"), is logged and left out.  One region
    writes ``{output_dir}/{mosdepth.output_file_prefix}.{type}``; with
    ``mosdepth.coverage.loci_file`` every region of the table writes
    ``loci_output`` (default ``{output_dir}/{prefix}.{locus}.{type}``, the
    form step 6's ``counts_file`` template reads).  Under torch.distributed
    rank 0 runs the step.  Returns the per-file path record (sample ->
    "device", "device:host-inflate", "host" or "failed"), None on a config
    error."""
    try:
        loci, outs, samples, files, cc = _coverage_config(config)
    except Exception as e:
        log(console, f"Config error: {e}", style="danger")
        return None
    if comm is None:
        from .dist_step4 import dist_comm
        comm = dist_comm()
    if comm is not None:
        from .dist_step4 import rank0_step
        box = []
        rank0_step(comm, lambda: box.append(_cover(config, console, loci, outs, samples, files, cc)))
        return box[0] if box else None
    return _cover(config, console, loci, outs, samples, files, cc)


def _cover(config, console, loci, outs, samples, files, cc):
    have = [s for s in samples if s in files]
    for s in samples:
        if s not in files:
            log(console, f"✗ {s}: no regions.bed.gz file", style="danger")
    triples = [(lc["chrom"], lc["start"], lc["end"]) for lc in loci]
    paths = [files[s] for s in have]
    log(console, f"Computing coverage of {len(loci)} region(s) for {len(have)} samples")
    if cc.get("device", True):
        from ..device import get_device
        from .coverage_device import cover_files
        res = cover_files(get_device(config), paths, triples, batch_files=int(cc.get("batch_files", 0)) or None,
                          hit_capacity=int(cc.get("hit_capacity", 0)) or None)
        values, record = res.coverage, res.path
    else:
        values = [[None if isinstance(v, Exception) else v for v in region_coverages(p, triples)] for p in paths]
        record = ["host"] * len(paths)
    for col, (lc, out) in enumerate(zip(loci, outs)):
        out = setup_output_file(out, lc["chrom"], lc["start"], lc["end"])
        write_coverage_results(out, [(s, values[k][col]) for k, s in enumerate(have) if values[k][col] is not None])
    for k, s in enumerate(have):
        bad = sum(v is None for v in values[k])
        if bad:
            log(console, f"✗ {s} failed" + (f" ({bad} of {len(loci)} regions)" if bad < len(loci) else ""),
                style="danger")
    log(console, f"Coverage results written to {outs[0] if len(outs) == 1 else f'{len(outs)} files'}", style="success")
    return dict(zip(have, record))
