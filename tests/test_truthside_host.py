"""Host side of the truth-side view (quasimodo_amd/truthside.py): region naming, the table writer, the rule that
selects the rows of a missed-variant list -- on literal hand-written texts -- and the refusal of a group of more than five.
The golden hcmv family gives the figures for TM-1-1 that the text restatement of make_snp_vector must reach."""
import os

import pytest

from conftest import GOLDEN
from quasimodo_amd import truthside as ts


def test_region_names_and_mask_order():
    names = ts.set_names(["lofreq", "varscan", "clc"])
    assert names == ["Genome", "LoFreq", "VarScan2", "CLC"]
    assert ts.region_name(1, names) == "Genome"
    assert ts.region_name(0b1011, names) == "Genome&LoFreq&CLC"
    assert ts.region_name(0b1111, names) == "Genome&LoFreq&VarScan2&CLC"
    assert ts.region_name(0b0110, names) == "LoFreq&VarScan2"
    for bad in (0, 16, -1):
        with pytest.raises(ValueError):
            ts.region_name(bad, names)
    assert ts.set_names(["mycaller"]) == ["Genome", "mycaller"]           # a label CALLER_MAP does not know keeps its spelling
    assert ts.venn_callers(["clc", "bcftools", "lofreq"]) == ["lofreq", "clc"]
    assert ts.venn_callers(["gatk"]) == []


def test_group_larger_than_five_is_refused():
    with pytest.raises(ValueError, match="1 to 5"):
        ts.set_names(["a", "b", "c", "d", "e", "f"])
    with pytest.raises(ValueError, match="1 to 5"):
        ts.check_group([])
    with pytest.raises(ValueError, match="twice"):
        ts.check_group(["lofreq", "clc", "lofreq"])
    assert ts.check_group("abcde") == list("abcde")


def test_venn_counts_and_table(tmp_path):
    # two callers.  truth side: slot m = truth keys hit by exactly the callers of m; callers' side: fp_overlap's slots
    truth_regions = [3, 5, 7, 11] + [0] * 28      # missed by both, caller 0 only, caller 1 only, both
    fp_regions = [0, 13, 17, 19]                  # (slot 0 is never read), caller 0 only, caller 1 only, both
    got = ts.venn_counts(truth_regions, fp_regions, 2)
    #               Genome  c0       G&c0    c1       G&c1    c0&c1    G&c0&c1
    assert got == [(1, 3), (2, 13), (3, 5), (4, 17), (5, 7), (6, 19), (7, 11)]
    with pytest.raises(ValueError):
        ts.venn_counts([1, 2], fp_regions, 2)
    path = tmp_path / "caller_snp_venn.tsv"
    ts.write_caller_snp_venn(str(path), {"TM-1-10": (truth_regions, fp_regions), "TA-1-1": ([1, 2, 3, 4], [0, 0, 0, 9])}, ["lofreq", "clc"])
    lines = path.read_text().split("\n")
    assert lines[0] == "sample\tregion\tcount"
    assert lines[1:8] == ["TA-1-1\tGenome\t1", "TA-1-1\tLoFreq\t0", "TA-1-1\tGenome&LoFreq\t2", "TA-1-1\tCLC\t0", "TA-1-1\tGenome&CLC\t3",
                          "TA-1-1\tLoFreq&CLC\t9", "TA-1-1\tGenome&LoFreq&CLC\t4"]
    assert lines[8] == "TM-1-10\tGenome\t3" and lines[14] == "TM-1-10\tGenome&LoFreq&CLC\t11"
    assert lines[15:] == [""] and len(lines) == 16          # 2 samples x (2^3 - 1) regions
    assert not [p for p in os.listdir(tmp_path) if ".tmp." in p]


TRUTH = (b"##fileformat=VCFv4.2\n"
         b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
         b"chr\t10\t.\tA\tC\t.\t.\t.\n"          # hit by the VCF
         b"chr\t20\t.\tC\tG\t.\t.\t.\n"          # missed
         b"chr\t20\t.\tC\tG\t.\t.\tagain\n"      # the same key on a second row: written again
         b"chr\t30\t.\tAT\tA\t.\t.\t.\n"         # an indel row: never in Genome
         b"chr\t40\t.\tg\tt\t.\t.\t.\n"          # lower-case alleles: make_snp_vector's %in% is case sensitive
         b"chr\t50\t.\tG\tT,A\t.\t.\t.\n"        # multi-allelic ALT: not a single base
         b"#chr\t60\t.\tG\tT\t.\t.\t.\n"         # a '#' row in the body: a header line to the writer, a comment to R
         b"chr\t070\t.\tT\tA\t.\t.\t.\n"         # R keeps POS as text: '070' is not '70'
         b"chr\t80\t.\tT\tC\n"                   # five columns suffice
         b"chr\t90\t.\tT\n")                     # fewer do not


def test_fn_row_selection_on_literal_text():
    assert ts.snp_key(b"chr\t10\t.\tA\tC\t.\t.\t.") == (b"10", b"A", b"C")
    assert ts.snp_key(b"chr\t30\t.\tAT\tA") is None and ts.snp_key(b"chr\t40\t.\tg\tt") is None and ts.snp_key(b"#x\t1\t.\tA\tC") is None
    assert ts.snp_keys(TRUTH) == {(b"10", b"A", b"C"), (b"20", b"C", b"G"), (b"070", b"T", b"A"), (b"80", b"T", b"C")}
    kept = {(b"10", b"A", b"C"), (b"70", b"T", b"A"), (b"999", b"A", b"G")}
    assert ts.fn_text(TRUTH, kept) == (b"##fileformat=VCFv4.2\n"
                                       b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                                       b"#chr\t60\t.\tG\tT\t.\t.\t.\n"
                                       b"chr\t20\t.\tC\tG\t.\t.\t.\n"
                                       b"chr\t20\t.\tC\tG\t.\t.\tagain\n"
                                       b"chr\t070\t.\tT\tA\t.\t.\t.\n"
                                       b"chr\t80\t.\tT\tC\n")
    # nothing missed: the header lines alone; no final newline in the input: the last row still ends in one
    assert ts.fn_text(b"#h\nchr\t1\t.\tA\tC", {(b"1", b"A", b"C")}) == b"#h\n"
    assert ts.fn_text(b"#h\nchr\t1\t.\tA\tC", set()) == b"#h\nchr\t1\t.\tA\tC\n"
    assert ts.fn_text(b"", set()) == b""


def test_golden_tm_1_1_figures():
    """TM-1-1 of the golden hcmv family through the text restatement: Genome = 160 keys, 11 populated regions of
    Genome + LoFreq + VarScan2 + CLC, all four = 46, Genome only = 3 (the figures the feature's issue states)."""
    fam = os.path.join(GOLDEN, "hcmv")
    rd = lambda rel: open(os.path.join(fam, rel), "rb").read()
    truth = rd("input/nucmer/TM.maskrepeat.variants.vcf")
    genome = ts.snp_keys(truth)
    assert len(genome) == 160
    callers = ts.venn_callers(["bcftools", "clc", "freebayes", "gatk", "lofreq", "varscan"])
    assert callers == ["lofreq", "varscan", "clc"]
    sets = [genome] + [ts.snp_keys(rd("expected/%s/TM-1-1.Merlin.%s.filtered.vcf" % (c, c))) for c in callers]
    count = {}
    for k in set().union(*sets):
        m = sum(1 << i for i, s in enumerate(sets) if k in s)
        count[m] = count.get(m, 0) + 1
    names = ts.set_names(callers)
    by_name = {ts.region_name(m, names): c for m, c in count.items()}
    assert len(by_name) == 11
    assert by_name["Genome&LoFreq&VarScan2&CLC"] == 46 and by_name["Genome"] == 3
    # the same numbers through venn_counts: the truth side's slots are the regions with the Genome bit, the others fp_overlap's
    tr = [count.get((m << 1) | 1, 0) for m in range(8)]
    fr = [count.get(m << 1, 0) for m in range(8)]
    assert sum(tr) == 160
    assert dict(ts.venn_counts(tr, fr, 3)) == {m: count.get(m, 0) for m in range(1, 16)}
    # the missed-by-all list holds exactly the rows of the `Genome`-only keys
    missed = ts.fn_text(truth, set().union(*sets[1:]))
    rows = [ln for ln in missed.split(b"\n") if ln and not ln.startswith(b"#")]
    assert {ts.snp_key(r) for r in rows} == {k for k in genome if all(k not in s for s in sets[1:])} and len(rows) >= 3


def test_reorder_regions():
    # slots over [clc, lofreq] (bit 0 = clc) as slots over [lofreq, clc]
    assert ts.reorder_regions([7, 1, 2, 3], ["clc", "lofreq"], ["lofreq", "clc"]) == [7, 2, 1, 3]
    have, want = ["clc", "lofreq", "varscan"], ["lofreq", "varscan", "clc"]
    got = ts.reorder_regions(list(range(8)), have, want)
    assert got[0b100] == 0b001 and got[0b001] == 0b010 and got[0b011] == 0b110 and got[0b111] == 0b111
    with pytest.raises(ValueError):
        ts.reorder_regions([0, 0], ["a"], ["b"])


def test_crlf_rows_key_the_same_in_both_functions():
    t = b"#h\r\nchr\t5\t.\tA\tC\r\n"
    assert ts.snp_keys(t) == {(b"5", b"A", b"C")}
    assert ts.fn_text(t, {(b"5", b"A", b"C")}) == b"#h\r\n"
    assert ts.fn_text(t, set()) == t


def test_dryrun_lists_the_truth_side_steps(tmp_path, capsys):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    assert workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"), dryrun=True) is None
    plain = capsys.readouterr().out
    assert "truthside" not in plain and "caller_snp_venn" not in plain
    assert workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"), dryrun=True, truth_side=True) is None
    out = capsys.readouterr().out
    assert out.startswith(plain)
    extra = out[len(plain):].splitlines()
    assert sum(ln.startswith("truthside_fn\t") for ln in extra) == 36            # 6 mixed samples x 6 callers
    assert "truthside_fn\tlofreq\tTM-1-1" in extra
    assert "missed_by_all\tTM-1-1\tlofreq,varscan,clc" in extra and sum(ln.startswith("missed_by_all\t") for ln in extra) == 6
    assert extra[-1] == "caller_snp_venn\tlofreq,varscan,clc"
    assert not (tmp_path / "out").exists()
    assert workflow.run_vareval(["a.vcf", "b.vcf"], "x.snps", str(tmp_path / "o2"), labels=["a", "b"], dryrun=True, truth_side=True) is None
    assert capsys.readouterr().out.splitlines()[-3:] == ["truthside_fn\ta", "truthside_fn\tb", "caller_snp_venn\ta,b"]


def test_extract_many_refuses_a_group_of_six():
    from quasimodo_amd.extract import Job, extract_many
    jobs = [Job("s.%d.vcf" % i, "t.vcf", "custom", "o", "c%d" % i) for i in range(6)]
    with pytest.raises(ValueError, match="1 to 5"):
        extract_many(jobs, groups=[[0, 1, 2, 3, 4, 5]])
