"""The haplotype pass on the device (qmvt_haplo.hip) against the restatement of quasimodo_amd.haplo, exactly, on
the edge families of haplo_edges.py: the 255|256 seams of k_hap_sites and its carried maximum, more than 8192 sites (two steps of
k_hap_rank, two blocks of k_hap_pairs, the rank carried over a change of truth set), sites of 65, 128 and 129 entries (a second
and a third gather round of k_hap_replay), windows clipped at 1 and at L + 1 on genomes that do not fill a packed word, bytes
that are no base, every pair of inline allele lengths through hp_trim, overlapping windows.  Per family and gap: both count
blocks, the class bytes, the site indices, the entry classes and qm_truth_sites; the ties of test_gpu_haplo.py; sorted against
shuffled; and, on the single-variant sites, the normal-form pass of 4.17 as an independent kernel.  Every comparison is exact:
these are integers.  (What the families plant is asserted by haplo_edges.PRESENT on the restatement fed with the batch's own
masks; tests/test_haplo_edges_host.py judges the restatement itself.)"""
import numpy as np
import pytest

import haplo_edges as he
from quasimodo_amd import haplo as hp
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

S_NPASS, S_TP_LINES = 0, 1
R, T = he.R, he.T


def run_family(engine, name, extra=None):
    e = he.family(name)
    gid = engine.genome_load(e.genome.encode("latin-1"))
    tids, b = [], None
    try:
        for t in e.tcodes:
            tids.append(engine.truth_load(*t))
        for w, tid in enumerate(tids):                          # the table order the families read their indices from
            got = engine.truth_entries(tid)
            assert list(zip(*[x.tolist() for x in got])) == e.order[w], "%s: the table of truth set %d" % (name, w)
        b = engine.batch([len(c[0]) for c in e.cols], [tids[v[1]] for v in e.vcfs], alleles=True)
        for v, c in enumerate(e.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        masks = []
        for v in range(b.n_vcf):
            m = b.cls(v)
            masks.append(((m & 1).astype(bool), (m & 2).astype(bool)))
        scal = b.scalars()
        _, ttru = b.vartype()
        genome_of = [gid if v[3] else -1 for v in e.vcfs]
        want, got = {}, {}
        for gap in e.gaps:
            rec, tru = b.haplotypes(genome_of, gap=gap, columns=True)
            for v, vc in enumerate(e.vcfs):
                case = "%s/%s, gap %d" % (name, vc[0], gap)
                if not vc[3]:
                    assert not rec[v].any() and not tru[v].any(), case      # a VCF without a genome keeps zero rows
                    with pytest.raises(QmvtError, match="named no genome"):
                        b.haplotyped(v)
                    continue
                wrec, wtru, wcls, wsite, wecls, detail = want[(v, gap)] = e.restate(v, gap, masks[v])
                cls, site, ecls = got[(v, gap)] = b.haplotyped(v)
                np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of " + case)
                np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of " + case)
                np.testing.assert_array_equal(cls, wcls, err_msg="classes of " + case)
                np.testing.assert_array_equal(site, wsite, err_msg="sites of " + case)
                np.testing.assert_array_equal(ecls, wecls, err_msg="entry classes of " + case)
                kept, tp = masks[v]
                assert int(rec[v][R["kept"]]) == int(kept.sum()) == int(scal[v][S_NPASS]), case
                assert int(rec[v][R["tp"]]) == int((kept & tp).sum()) == int(scal[v][S_TP_LINES]), case
                assert int(rec[v][R["tp_h"]]) - int(rec[v][R["tp"]]) == int(rec[v][R["rescued"]]), case
                assert int(tru[v][T["found"]]) == int(ttru[v][:, 1].sum()), case       # FOUND is the found count of the variant-type pass
                assert int(tru[v][T["found_h"]]) >= int(tru[v][T["found"]]) and int(tru[v][T["entries"]]) == len(e.order[vc[1]]), case
            for t, (v, perm) in e.twin.items():                 # sorted and shuffled: the same counts, the same outcome line by line
                case = "%s/%s against its shuffled twin, gap %d" % (name, e.vcfs[v][0], gap)
                np.testing.assert_array_equal(rec[v], rec[t], err_msg="rec of " + case)
                np.testing.assert_array_equal(tru[v], tru[t], err_msg="tru of " + case)
                np.testing.assert_array_equal(got[(v, gap)][0][perm], got[(t, gap)][0], err_msg="classes of " + case)
                np.testing.assert_array_equal(got[(v, gap)][1][perm], got[(t, gap)][1], err_msg="sites of " + case)
                np.testing.assert_array_equal(got[(v, gap)][2], got[(t, gap)][2], err_msg="entry classes of " + case)
            for w, tid in enumerate(tids):
                sites = engine.truth_sites(tid, gid, gap)
                for x, y, what in zip(sites, hp.truth_sites(e.genome, e.tcodes[w], gap), ("first entries", "window starts", "window ends")):
                    np.testing.assert_array_equal(x, y, err_msg="qm_truth_sites, %s of %s, truth set %d, gap %d" % (what, name, w, gap))
        he.PRESENT[name](e, want)                               # what the family plants arrived (the restatement on the batch's own masks)
        if extra is not None:
            extra(e, b, engine, gid, tids, got)
    finally:
        if b is not None:
            b.close()
        for t in tids:
            engine.truth_release(t)
        engine.genome_release(gid)


def normal_form_tie(e, b, engine, gid, tids, got):
    """Through an independent kernel (4.17).  A tried site with one open line and one open entry holds one variant per side; both
    passes read the same genome, here pure ACGT with every variant behind position 1, so both variants have a normal form, and
    two variants give one sequence iff their normal forms are equal (Tan et al. 2015).  Every line of this family is kept with ID
    '.', and a tried line is no TP line, so it is rescued by normal form iff its form is some entry's.  Hence, for a line in such
    a site whose normal-form row IS the site's entry: rescued there => MATCH here, and MISMATCH here => not rescued there; the
    converse of the first holds by the same argument and is asserted too.  Left out by rule: lines that are not tried here (their
    entry is found by spelling -- the normal-form pass still counts them --, or their footprint lies in no window), and lines
    whose normal-form row is an entry of another site."""
    rec, tru = b.normalize([gid] * b.n_vcf, columns=True)
    for v in (0, 1):
        npos, nref, nalt, ncls, nrow = b.normalized(v)
        for gap in e.gaps:
            he.check_normal_form_tie(e, v, gap, got[(v, gap)], engine.truth_sites(tids[0], gid, gap)[0], ncls, nrow)


def test_trim_arithmetic_at_every_inline_length_pair(engine):
    run_family(engine, "trim", normal_form_tie)


def test_the_seams_of_the_site_scan(engine):
    run_family(engine, "seams")


def test_rank_and_pairs_across_words_steps_and_vcfs(engine):
    run_family(engine, "rank")


def test_sites_with_more_than_64_entries(engine):
    run_family(engine, "dense")


@pytest.mark.parametrize("name", ["ends0", "ends1", "ends7"])
def test_both_ends_of_the_genome(engine, name):
    run_family(engine, name)


def test_bytes_that_are_no_base(engine):
    run_family(engine, "nobase")


def test_overlapping_windows(engine):
    run_family(engine, "overlap")
