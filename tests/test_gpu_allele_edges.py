"""The three allele passes on the device -- normal form (qmvt_norm.hip), atomisation (qmvt_atom.hip; 4.18), type and
size (qmvt_types.hip; 4.19) -- against the restatements of quasimodo_amd.normalize, .atomize and .vartype, exactly, on the edge
families of allele_edges.py: every pair of inline allele lengths at every extreme of the common prefix and suffix (vt_row,
at_reason / at_next, nm_normalize), one long allele of 14 to 60 bases against every inline length at three sets of size edges,
both open-addressing tables exactly half full, wrapped over their last slot and contended by more entries of one form than two
workgroups hold, the span walk of all three record kernels on VCFs of 16 384, 16 385, 65 536 and 65 537 records with a planted
record on either side of every step, both ends of genomes that do not fill a packed word, bytes that are no base.  Per family ONE
finished batch runs all three passes: both count blocks of each, the class bytes, the normal-form columns and rows, the atom
counts and hit masks, the type rows, qm_truth_normalized, qm_truth_atoms and qm_truth_entries; sorted against shuffled; the ties
that hold between kernels that share no code (allele_edges.check_ties, check_partition); neutrality.  Every comparison is exact:
these are integers.  (What the families plant is asserted by allele_edges.PRESENT on the restatements fed with the batch's own
masks; tests/test_allele_edges_host.py judges the restatements themselves.)"""
import time

import numpy as np
import pytest

import allele_edges as ae
from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

S_NPASS, S_TP_LINES = 0, 1


def equal(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def run_family(engine, name, partition=()):
    f = ae.family(name)
    gids, tids, b = [], [], None
    t0 = time.perf_counter()
    try:
        gids = [engine.genome_load(g.encode("latin-1")) for g in f.genomes]
        for t in f.tcodes:
            tids.append(engine.truth_load(*t))
        for w, tid in enumerate(tids):                          # the three truth-side getters, from the kernels the passes use
            case = "%s, truth set %d" % (name, w)
            got = engine.truth_entries(tid)
            assert list(zip(*[x.tolist() for x in got])) == f.order[w], "qm_truth_entries of " + case
            got = engine.truth_normalized(tid, gids[f.tgen[w]])
            assert list(zip(*[x.tolist() for x in got])) == sorted(nz.truth_forms(f.genomes[f.tgen[w]], *f.tcodes[w])[0]), "qm_truth_normalized of " + case
            assert engine.truth_atoms(tid).tolist() == sorted(at.truth_atoms(*f.tcodes[w])[2]), "qm_truth_atoms of " + case
        b = engine.batch([len(c[0]) for c in f.cols], [tids[v[1]] for v in f.vcfs], alleles=True)
        for v, c in enumerate(f.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        before = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
        masks = [((m & 1).astype(bool), (m & 2).astype(bool)) for m in before[0]]
        genome_of = [gids[f.tgen[vc[1]]] if vc[3] else -1 for vc in f.vcfs]
        nrec, ntru = b.normalize(genome_of, columns=True)
        arec, atru = b.atomize(columns=True)
        typed = {}
        for e in f.edges:
            trec, ttru = b.vartype(e, f.shapes, columns=True)
            typed[e] = (trec, ttru, [b.vartyped(v) for v in range(b.n_vcf)])
        got_n = [b.normalized(v) if vc[3] else None for v, vc in enumerate(f.vcfs)]
        got_a = [b.atomized(v) for v in range(b.n_vcf)]
        scal = b.scalars()
        t_call = time.perf_counter() - t0
        want = {}
        for v, vc in enumerate(f.vcfs):
            case = "%s/%s" % (name, vc[0])
            wn, wa, wt = want[v] = f.restate(v, masks[v])
            kept, tp = masks[v]
            if vc[3]:
                equal(nrec[v], wn[0], "normal form, rec of " + case)
                equal(ntru[v], wn[1], "normal form, tru of " + case)
                gp, gr, ga, gcls, grow = got_n[v]
                for x, y, what in zip((gcls, gp, gr, ga, grow), wn[2:], ("classes", "positions", "REFs", "ALTs", "truth rows")):
                    equal(x, y, "normal form, %s of %s" % (what, case))
                assert int(nrec[v][ae.NR["kept"]]) == int(kept.sum()) == int(scal[v][S_NPASS]), case
                assert int(nrec[v][ae.NR["tp"]]) == int((kept & tp).sum()) == int(scal[v][S_TP_LINES]), case
            else:
                assert not nrec[v].any() and not ntru[v].any(), case         # a VCF without a genome keeps zero rows
                with pytest.raises(QmvtError, match="named no genome"):
                    b.normalized(v)
            equal(arec[v], wa[0], "atoms, rec of " + case)
            equal(atru[v], wa[1], "atoms, tru of " + case)
            for x, y, what in zip(got_a[v], wa[2:], ("classes", "atom counts", "hit masks")):
                equal(x, y, "atoms, %s of %s" % (what, case))
            for e in f.edges:
                equal(typed[e][0][v], wt[e][0], "types at %r, rec of %s" % (e, case))
                equal(typed[e][1][v], wt[e][1], "types at %r, tru of %s" % (e, case))
                equal(typed[e][2][v], wt[e][2], "types at %r, rows of %s" % (e, case))
                assert int(typed[e][1][v][:, 1].sum()) == int(atru[v][ae.AT["found"]]), case       # found entries: two kernels, one number
        for t, (v, perm) in f.twin.items():                     # sorted and shuffled: the same counts, the same outcome line by line
            case = "%s/%s against its shuffled twin" % (name, f.vcfs[v][0])
            for x in (nrec, ntru, arec, atru) + tuple(typed[e][k] for e in f.edges for k in (0, 1)):
                equal(x[v], x[t], "counts of " + case)
            for x, y in zip(got_n[v] + got_a[v] + tuple(typed[e][2][v] for e in f.edges), got_n[t] + got_a[t] + tuple(typed[e][2][t] for e in f.edges)):
                equal(x[perm], y, "columns of " + case)
        ae.PRESENT[name](f, want)                               # what the family plants arrived (the restatements on the batch's own masks)
        for v, vc in enumerate(f.vcfs):                         # the ties between kernels that share no code, on the device's output
            if vc[3]:
                gp, gr, ga, gcls, grow = got_n[v]
                ae.check_ties(f, v, (gp, gr, ga), gcls, got_a[v][1], typed[f.edges[0]][2][v])
                if vc[0] in partition:
                    assert ae.check_partition(f, v, (gp, gr, ga), gcls, grow) > 0
        for v in range(b.n_vcf):                                # neutrality: the batch's masks, scalars and ROC are what they were
            equal(b.cls(v), before[0][v], "class masks of %s, VCF %d" % (name, v))
        equal(b.scalars(), before[1], "scalars of " + name)
        equal(b.roc(), before[2], "ROC of " + name)
        print("\n%s: call phase %.3f s, restatement and checks %.3f s" % (name, t_call, time.perf_counter() - t0 - t_call))
    finally:
        if b is not None:
            b.close()
        for t in tids:
            engine.truth_release(t)
        for g in gids:
            engine.genome_release(g)


def test_every_pair_of_inline_lengths(engine):
    run_family(engine, "pairs", partition=("respelled", "respelled_shuffled"))


def test_one_long_allele_against_every_inline_length(engine):
    run_family(engine, "longshort")


def test_both_hash_tables_half_full_wrapped_and_contended(engine):
    run_family(engine, "tables", partition=("contended", "contended_reversed", "contended_shuffled", "wrap1024"))


def test_the_span_walk_on_its_seams(engine):
    run_family(engine, "walk")


@pytest.mark.parametrize("name", ["ends0", "ends1", "ends7"])
def test_both_ends_of_the_genome(engine, name):
    run_family(engine, name, partition=("homopolymer", "dinucleotide"))


def test_bytes_that_are_no_base(engine):
    run_family(engine, "nobase", partition=("blocks", "run"))
