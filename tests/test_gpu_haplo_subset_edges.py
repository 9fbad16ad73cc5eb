"""The subset search on the device (k_hap_subsets in qmvt_haplo.hip) against the restatement of
quasimodo_amd.haplo, exactly, on the edge families of haplo_subset_edges.py: subset hashes composed across every seam of the power
table and of the scanned prefix hashes, colliding candidates that only the symbol loop refutes (behind its first stride, and
behind offset 256), the order of forms inside one q, every (n_S, n_T) in 1 .. 8 x 1 .. 8 with optima in every quarter of the
masks, the four levels of the order key, items against forms over two truth sets and three gather rounds, windows of 253 .. 257
bases and windows clipped at 1 and at L + 1.  Per family, VCF and gap: the count block, both second class arrays, the list of
PARTIAL sites and their masks; the narrow-hash mode against the normal one bit for bit; the four identities; the haplotype
pass's own answers before and after; sorted against shuffled.  Every comparison is exact: these are integers.  (What the families
plant is asserted by haplo_subset_edges.PRESENT on the restatement fed with the batch's own masks;
tests/test_haplo_subset_edges_host.py judges the restatement itself.)"""
import numpy as np
import pytest

import haplo_subset_edges as se
import haplo_subsets as hs
from quasimodo_amd import haplo as hp
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

U = {name: k for k, name in enumerate(hp.SUB_COLS)}
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}


class Setup:
    def __init__(self, engine, name):
        self.engine = engine
        self.e = e = se.family(name)
        self.gid = engine.genome_load(e.genome.encode("latin-1"))
        self.tids = [engine.truth_load(*t) for t in e.tcodes]
        self.b = b = engine.batch([len(c[0]) for c in e.cols], [self.tids[v[1]] for v in e.vcfs], alleles=True)
        for v, c in enumerate(e.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        self.masks = []
        for v in range(b.n_vcf):
            m = b.cls(v)
            self.masks.append(((m & 1).astype(bool), (m & 2).astype(bool)))
        self.genome_of = [self.gid if v[3] else -1 for v in e.vcfs]

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        self.engine.genome_release(self.gid)


def fetch(b, vs):
    return b.hapsubset_counts().copy(), {v: b.hapsubsetted(v) for v in vs}


def run_family(engine, name):
    s = Setup(engine, name)
    try:
        check_family(s)
    finally:
        s.close()


def check_family(setup):
    b, e = setup.b, setup.e
    with_genome = [v for v, vc in enumerate(e.vcfs) if vc[3]]
    want = {}
    for gap in e.gaps:
        rec, tru = b.haplotypes(setup.genome_of, gap=gap, columns=True)
        pass_before = (rec.copy(), tru.copy(), [b.haplotyped(v) for v in with_genome])
        base = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
        sub = b.hapsubsets(columns=True)
        assert sub.shape == (b.n_vcf, 8) and sub.dtype == np.uint64
        normal = fetch(b, with_genome)
        for v, vc in enumerate(e.vcfs):
            case = "%s/%s, gap %d" % (e.name, vc[0], gap)
            if not vc[3]:
                assert not sub[v].any(), case                           # a VCF without a genome keeps a zero row
                with pytest.raises(QmvtError, match="named no genome"):
                    b.hapsubsetted(v)
                continue
            res, (wsub, wcls, wecls, chosen) = want[(v, gap)] = hs.restate(e, v, gap, setup.masks[v])
            cls_s, ecls_s, site_s, sm, tm = normal[1][v]
            got = list(zip(site_s.tolist(), sm.tolist(), tm.tolist()))
            assert got == [d[:3] for d in chosen], "sites and masks of %s: %r against %r" % (
                case, sorted(set(got) - {d[:3] for d in chosen}), sorted({d[:3] for d in chosen} - set(got)))
            np.testing.assert_array_equal(sub[v], wsub, err_msg="sub of " + case)
            np.testing.assert_array_equal(cls_s, wcls, err_msg="second classes of " + case)
            np.testing.assert_array_equal(ecls_s, wecls, err_msg="second entry classes of " + case)
            assert len(ecls_s) == len(e.order[vc[1]]), case              # the entry classes of this VCF's own truth set
            # the identities
            cls, site, ecls = pass_before[2][with_genome.index(v)]
            s = [int(x) for x in sub[v]]
            assert s[U["searched"]] == s[U["partial"]] + s[U["nosubset"]], case
            kept = setup.masks[v][0]
            tried = {int(x) for x in site[kept & ((cls == hp.MISMATCH) | (cls == hp.CONFLICT))]}
            assert s[U["searched"]] == len(tried), case
            partial = np.isin(site, site_s) & np.isin(cls, (hp.MISMATCH, hp.CONFLICT))
            assert s[U["rescued_s"]] + s[U["left_lines"]] == int(partial.sum()), case
            open_ents = int(np.isin(ecls_s, (hp.SUBSET, hp.LEFT)).sum())
            assert s[U["found_s"]] - int(tru[v][T["found_h"]]) + s[U["left_entries"]] == open_ents, case
            assert int((cls_s == hp.SUBSET).sum()) == s[U["rescued_s"]] and int((cls_s == hp.LEFT).sum()) == s[U["left_lines"]], case
            same = ~np.isin(cls_s, (hp.SUBSET, hp.LEFT))
            np.testing.assert_array_equal(cls_s[same], cls[same])            # outside PARTIAL sites: the pass's own bytes
            same = ~np.isin(ecls_s, (hp.SUBSET, hp.LEFT))
            np.testing.assert_array_equal(ecls_s[same], ecls[same])
            assert s[U["tp_s"]] >= int(rec[v][R["tp_h"]]) and s[U["found_s"]] >= int(tru[v][T["found_h"]]), case
        # sorted and shuffled: the same counts, the same sites and masks, the same rescued (POS, REF, ALT)
        for t, (v, perm) in e.twin.items():
            np.testing.assert_array_equal(sub[v], sub[t])
            for k in (2, 3, 4):
                np.testing.assert_array_equal(normal[1][v][k], normal[1][t][k])
            np.testing.assert_array_equal(normal[1][v][0][perm], normal[1][t][0])
            np.testing.assert_array_equal(normal[1][v][1], normal[1][t][1])
            spelled = lambda w: sorted(zip(*[x[normal[1][w][0] == hp.SUBSET].tolist() for x in e.cols[w][:3]]))
            assert spelled(v) == spelled(t)
        # the narrow hashes: more candidates collide, the answers are the same bit for bit
        sub_n = b.hapsubsets(columns=True, narrow_hash=True)
        narrow = fetch(b, with_genome)
        for v in with_genome:
            case = "%s/%s, gap %d, narrow against normal" % (e.name, e.vcfs[v][0], gap)
            assert list(zip(*[x.tolist() for x in narrow[1][v][2:]])) == list(zip(*[x.tolist() for x in normal[1][v][2:]])), case
            for x, y in zip(narrow[1][v], normal[1][v]):
                np.testing.assert_array_equal(x, y, err_msg=case)
        np.testing.assert_array_equal(sub_n, sub)
        # the pass's own answers, and the batch, are what they were
        rec2, tru2 = b.haplotype_counts()
        np.testing.assert_array_equal(rec2, pass_before[0])
        np.testing.assert_array_equal(tru2, pass_before[1])
        for k, v in enumerate(with_genome):
            for x, y in zip(b.haplotyped(v), pass_before[2][k]):
                np.testing.assert_array_equal(x, y)
        for v in range(b.n_vcf):
            np.testing.assert_array_equal(b.cls(v), base[0][v])
        np.testing.assert_array_equal(b.scalars(), base[1])
        np.testing.assert_array_equal(b.roc(), base[2])
    se.PRESENT[e.name](e, want)                                         # what the family plants arrived (the batch's own masks)


def test_subset_hashes_across_the_seams_of_the_prefix_tables(engine):
    run_family(engine, "hash")


def test_colliding_candidates_are_refuted_behind_the_first_stride(engine):
    run_family(engine, "verify")


def test_the_rank_of_a_form_inside_one_q(engine):
    run_family(engine, "order")


def test_every_pair_of_form_counts_and_every_quarter_of_the_masks(engine):
    run_family(engine, "rounds")


def test_the_four_levels_of_the_order_key(engine):
    run_family(engine, "ties")


def test_items_against_forms_two_truth_sets_three_gather_rounds(engine):
    run_family(engine, "items")


def test_windows_of_253_to_257_bases_no_base_bytes_and_position_1(engine):
    run_family(engine, "edges")


@pytest.mark.parametrize("name", ["right260", "right263", "right264"])
def test_a_window_clipped_behind_the_last_base(engine, name):
    run_family(engine, name)
