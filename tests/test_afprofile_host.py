"""The host side of the allele-frequency profiles: qm_vcf_scan_af against literal lines and against Python's
regex engine run with the R pattern over the golden family, the table writers on a hand-made grid.  CPU only."""
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

# scripts/mutation_context_profile.R:26 -- gsub(".*AF=([01]\\.[0-9]+);.*$", "\\1", INFO, perl=T)
R_PATTERN = re.compile(rb".*AF=([01]\.[0-9]+);.*$")
HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def line(info, pos=b"100", tail=b"", fields=8):
    cols = [b"chr", pos, b".", b"A", b"C", b"50", b"PASS", info]
    return b"\t".join(cols[:fields]) + tail


def scan(text):
    from quasimodo_amd.vcfio import scan_vcf
    sv = scan_vcf(text)
    af, info = sv.scan_af()
    return sv, af, info


def f32(s):
    return np.float32(float(s))


def same(got, want):
    """bit for bit, NaN == NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    m = ~np.isnan(want)
    assert np.array_equal(got[m].view(np.uint32), want[m].view(np.uint32)), (got, want)


LITERALS = [
    (b"DP=10;AF=0.1;X=1;AF=0.25;", "0.25"),           # the leading .* is greedy: the last occurrence
    (b"MAF=0.3;", "0.3"),                              # no word boundary in the pattern
    (b"DP=4;AF=0.5", None),                            # the field's last entry without ';'
    (b"AF=1.5;", "1.5"),                               # [01]\.[0-9]+ : not a frequency, but what R reads
    (b"AF=2.0;", None),
    (b"AF=0.;", None),
    (b"AF=.5;", None),
    (b"AF=1e-1;", None),
    (b"AF=0.5;AF=0.7", "0.5"),                         # the last place that MATCHES, not the last "AF="
    (b"AF=0.25x;DP=3;", None),
    (b"AF=0.1000000014901161193847656250001;", "0.1000000014901161193847656250001"),   # just above the tie of two floats
    (b"AF=0.10000000149011611938476562500;DP=1", "0.10000000149011611938476562500"),    # the tie itself: to even
    (b"AF=0.0;", "0.0"),
    (b"AF=1.0;SB=2", "1.0"),
    (b"AAF=0.125;AF=;", "0.125"),
    (b".", None),
    (b"0.75", None),                                   # R's as.numeric would read the field itself: the stated divergence
    (b"", None),
]


def test_literal_info_fields():
    text = HEAD + b"".join(line(i) + b"\n" for i, _ in LITERALS)
    sv, af, info = scan(text)
    assert sv.n_records == len(LITERALS)
    want = [np.float32(np.nan) if w is None else f32(w) for _, w in LITERALS]
    same(af, want)
    assert info == (sum(w is not None for _, w in LITERALS), 0)
    assert f32("0.1000000014901161193847656250001") == np.float32(0.1)     # float32(0.1) + 1e-31: the excess is below half a double's ulp
    for (i, w), got in zip(LITERALS, af):              # the same through the regex engine
        m = R_PATTERN.match(i)
        assert (m is None) == (w is None) and (m is None or m.group(1).decode() == w), i
        assert math.isnan(got) if w is None else got == f32(w)


def test_double_then_float_rounding():
    """the captured text becomes a correctly rounded double, then a float (as.numeric, then the column): just above the middle of
    two floats the double IS the middle, and the tie goes to the even float -- a conversion straight to float would go up"""
    from decimal import Decimal, getcontext
    getcontext().prec = 80
    lo = np.float32(0.3)
    hi = np.nextafter(lo, np.float32(1))
    mid = (Decimal(float(lo)) + Decimal(float(hi))) / 2
    above = format(mid + Decimal("1e-40"), "f")
    below = format(mid - Decimal("1e-40"), "f")
    even = lo if (lo.view(np.uint32) & 1) == 0 else hi
    assert float(above) == float(below) == float(mid) and f32(above) == even == f32(below)
    text = HEAD + b"".join(line(b"AF=" + v.encode() + b";") + b"\n" for v in (above, below, format(mid, "f")))
    sv, af, info = scan(text)
    same(af, [even, even, even])


def test_field_borders_short_lines_and_line_ends():
    rows = [
        (line(b"DP=3;", tail=b"\tAF=0.9;"), None, False),              # a 9th field is not read
        (line(b"AF=0.4;", tail=b"\tGT\t0/1"), "0.4", False),
        (line(b"", fields=7), None, True),                               # 7 fields: no INFO
        (line(b"", fields=7) + b"\t", None, False),                       # an empty 8th field is a field
        (line(b"", fields=5), None, True),
        (line(b"AF=0.6;") + b"\r", "0.6", False),                         # CRLF: the '\r' belongs to the field, behind the ';'
        (line(b"AF=0.6") + b"\r", None, False),
        (line(b"AF=0.6;\r", tail=b"\tx"), "0.6", False),
    ]
    text = HEAD + b"".join(r + b"\n" for r, _, _ in rows)
    for t in (text, text[:-1]):                                           # with and without the last newline
        sv, af, info = scan(t)
        same(af, [np.float32(np.nan) if w is None else f32(w) for _, w, _ in rows])
        assert info == (sum(w is not None for _, w, _ in rows), sum(s for _, _, s in rows))
    sv, af, info = scan(HEAD + line(b"X=1;AF=0.125;"))                    # the only data line, no newline at all
    same(af, [f32("0.125")])
    crlf = HEAD.replace(b"\n", b"\r\n") + b"".join(line(i) + b"\r\n" for i, _ in LITERALS)
    sv, af, info = scan(crlf)
    want = [np.float32(np.nan) if R_PATTERN.match(i + b"\r") is None else f32(R_PATTERN.match(i + b"\r").group(1).decode()) for i, _ in LITERALS]
    same(af, want)
    assert np.array_equal(np.isnan(af), [w is None for _, w in LITERALS])


def test_record_order_with_header_kinds_and_host_lines():
    """one float per line that owns a record, in record order: '#' lines in the middle of the data (kinds 1 and 3) own none,
    QM_LINE_DATA_HOST lines (POS not a canonical decimal) own one"""
    body = [
        line(b"AF=0.11;"),
        b"#late comment\tAF=0.99;",
        line(b"AF=0.22;", pos=b"007"),                                    # kind 2
        b"#chr\t5\t.\tA\tC\t50\tPASS\tAF=0.88;",                          # a '#' line that passes the filter: kind 3
        line(b"DP=1;"),
        line(b"AF=0.33;", pos=b"+12"),
        line(b"AF=0.44;"),
    ]
    text = HEAD + b"\n".join(body) + b"\n"
    sv, af, info = scan(text)
    kinds = list(sv.line_kind)
    assert kinds[:2] == [1, 1] and kinds[3] == 1 and kinds[5] == 3 and kinds[4] == 2 and kinds[7] == 2 and sv.n_records == 5
    same(af, [f32("0.11"), f32("0.22"), np.float32(np.nan), f32("0.33"), f32("0.44")])
    assert info == (4, 0)
    before = (sv.line_off.copy(), sv.line_kind.copy(), sv.pos.copy(), sv.flags.copy())
    sv.scan_af()
    assert all(np.array_equal(a, b) for a, b in zip(before, (sv.line_off, sv.line_kind, sv.pos, sv.flags)))


def test_empty_and_header_only_texts():
    for t in (b"", HEAD):
        sv, af, info = scan(t)
        assert af.shape == (0,) and info == (0, 0)


GOLDEN_VCFS = sorted(glob.glob(os.path.join(GOLDEN, "hcmv", "input", "**", "*.vcf"), recursive=True))


def test_golden_family_against_the_regex_engine():
    """every input VCF of the hcmv family: the scanner against re.sub with the R pattern on the 8th field -- another engine, not
    the scanner written twice.  A field the pattern leaves as it is: NaN (R: as.numeric of the field, NA for every field here)."""
    assert len(GOLDEN_VCFS) >= 30
    occurrences = values = carrying = 0
    for path in GOLDEN_VCFS:
        text = open(path, "rb").read()
        sv, af, info = scan(text)
        want = []
        occurrences += text.count(b"AF=")
        carrying += b"AF=" in text
        for ln in text.split(b"\n"):
            if not ln or ln[:1] == b"#":
                continue
            c = ln.split(b"\t")
            if len(c) < 8:
                want.append(np.float32(np.nan))
                continue
            out, n = R_PATTERN.subn(rb"\1", c[7])
            want.append(f32(out.decode()) if n else np.float32(np.nan))
            if not n:
                with pytest.raises(ValueError):
                    float(c[7])                       # no field here is a number by itself: the divergence does not show
        assert not ((sv.line_kind != 0) & (sv.line_kind != 1) & (sv.line_kind != 2) & (sv.line_kind != 5)).any()
        same(af, want)
        assert info[0] == int(np.count_nonzero(~np.isnan(np.asarray(want)))) and info[1] == 0
        values += info[0]
    assert occurrences == 3450 and carrying == 30 and values > 1000      # what the family holds: 30 of its files carry AF=


# ---- the table writers ---------------------------------------------------------------------------------------------------
def _hand():
    grid = np.zeros((2, 4, 3), np.uint64)
    grid[0, 0, 0] = 2
    grid[0, 3, 2] = 5
    grid[1, 1, 1] = 7
    grid[1, 3, 0] = 1
    extra = np.array([[1, 0, 7], [0, 2, 8]], np.uint64)
    return grid, extra


def test_profile_grid_writer(tmp_path):
    from quasimodo_amd import afprofile
    grid, extra = _hand()
    only_fp = np.zeros_like(grid)
    only_fp[1, 2, 1] = 3
    path = tmp_path / "TM.lofreq.snp.profile.tsv"
    afprofile.write_profile_grid(str(path), [("TM-1-10", grid, extra), ("TM-0-1", only_fp, np.array([[0, 0, 0], [4, 0, 3]]), ("FP",))], window=1000)
    assert path.read_text().split("\n") == [
        "sample\ttype\taf_lo\taf_hi\tpos_lo\tpos_hi\tcount",
        "TM-1-10\tTP\t0\t0.25\t1\t1000\t2",
        "TM-1-10\tTP\t0.75\t1\t2001\t3000\t5",
        "TM-1-10\tFP\t0.25\t0.5\t1001\t2000\t7",
        "TM-1-10\tFP\t0.75\t1\t1\t1000\t1",
        "TM-0-1\tFP\t0.5\t0.75\t1001\t2000\t3",
        "# sample\ttype\tno_af\toutside\tin_grid",
        "# TM-1-10\tTP\t1\t0\t7",
        "# TM-1-10\tFP\t0\t2\t8",
        "# TM-0-1\tFP\t4\t0\t3",
        "",
    ]
    assert not list(tmp_path.glob("*.tmp.*"))
    with pytest.raises(ValueError):
        afprofile.write_profile_grid(str(path), [("x", grid[0], extra)])


def test_af_sweep_writer(tmp_path):
    from quasimodo_amd import afprofile
    grid, extra = _hand()
    sw = afprofile.af_sweep(grid)
    assert sw.tolist() == [[7, 5, 5, 5], [8, 8, 1, 1]]          # TP(af >= a / 4), FP(af >= a / 4)
    assert sw[0, 0] == extra[0, 2] and sw[1, 0] == extra[1, 2]
    path = tmp_path / "TM.lofreq.snp.profile.afsweep.tsv"
    afprofile.write_af_sweep(str(path), [("TM-1-10", grid, extra), ("TM-0-1", grid, extra, ("FP",))])
    assert path.read_text().split("\n") == [
        "sample\taf_min\tTP\tFP",
        "TM-1-10\t0\t7\t8", "TM-1-10\t0.25\t5\t8", "TM-1-10\t0.5\t5\t1", "TM-1-10\t0.75\t5\t1",
        "TM-0-1\t0\t0\t8", "TM-0-1\t0.25\t0\t8", "TM-0-1\t0.5\t0\t1", "TM-0-1\t0.75\t0\t1",
        "",
    ]
    rows = afprofile.sample_rows({"TM-1-0": None, "TM-1-10": dict(af_grid=grid, af_extra=extra), "TM-0-1": dict(af_grid=grid, af_extra=extra)})
    assert [(r[0], r[3]) for r in rows] == [("TM-0-1", ("FP",)), ("TM-1-10", ("TP", "FP"))]


def test_profile_and_truthside_do_not_combine(tmp_path, capsys):
    from quasimodo_amd import workflow
    from quasimodo_amd.extract import Job, extract_many
    jobs = [Job("s.%d.vcf" % i, "t.vcf", "custom", "o", "c%d" % i) for i in range(2)]
    prof = {"want": [1, 1], "window": 1024, "n_pos_bins": 256, "n_af_bins": 20}
    with pytest.raises(ValueError, match="profile"):
        extract_many(jobs, fn=True, profile=prof)
    jobs = [Job("s.%d.vcf" % i, "t.vcf", "custom", "o", "c%d" % i) for i in range(2)]
    with pytest.raises(ValueError, match="profile"):
        extract_many(jobs, groups=[[0, 1]], profile=prof)
    jobs = [Job("s.%d.vcf" % i, "t.vcf", "custom", "o", "c%d" % i) for i in range(2)]
    with pytest.raises(ValueError, match="entries"):
        extract_many(jobs, profile={"want": [1]})
    from quasimodo_amd.engine import Engine
    with pytest.raises(ValueError, match="profile"):       # the binding refuses before it touches the library
        Engine.extract_files(object.__new__(Engine), [], truthside={"fn": [], "group": []}, profile={"want": []})
    with pytest.raises(workflow.WorkflowError, match="truth-side"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), dryrun=True, truth_side=True, snp_profile=True)


def test_workflow_dryrun_names_the_profile_tables(tmp_path, capsys):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    assert workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"), dryrun=True, snp_profile={"window": 500}) is None
    out = capsys.readouterr().out.splitlines()
    assert "snp_profile\tTM\tlofreq" in out and "snp_profile\tTA\tclc" in out
    assert not (tmp_path / "out").exists()
    with pytest.raises(workflow.WorkflowError, match="8192"):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"), dryrun=True, snp_profile={"n_pos_bins": 1000})
