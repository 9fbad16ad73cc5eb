"""The match ladder per variant type and size on the device (qm_batch_ladder_types; k_ltype_records / k_ltype_truth; DESIGN.md
4.24) against the restatement of quasimodo_amd.laddertypes, exactly, rec and tru: the bincount over the row bytes the type pass
left and the mask bytes the ladder left (both compared with their own restatements in test_gpu_vartype.py / test_gpu_ladder.py),
the entries typed on the host -- on VCFs around the lane's 16-record step and the span seams with a kept line that is no TP
planted on either side of every seam and at every VCF's end, several VCFs per truth set, 1, 8 and 16 size bins, with and without
a shape table, truth sets of 1, 65 and 2000 entries, VCFs without a genome in either call or in both, with and without the subset
search, sorted and shuffled; the planted family; 4096 lines in one cell and 70 000 in the hot one; the identities against
qm_batch_get_ladder and qm_batch_get_types; the state rules."""
import numpy as np
import pytest

from quasimodo_amd import _lib
from quasimodo_amd import ladder as ld
from quasimodo_amd import laddertypes as lt
from quasimodo_amd import normalize as nz
from quasimodo_amd import vartype as vt
from quasimodo_amd._lib import QmvtError
from haplo_family import truth_codes
from ladder_family import LadderFamily
import rescueroc_family as fam

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
K, S, N, A, H, B = ld.M_K, ld.M_S, ld.M_N, ld.M_A, ld.M_H, ld.M_B
REACHED = (0, N, A, H, B, N | H, A | H, N | B)      # tests/test_laddertypes_host.py asserts them of the draw
SIZES = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 16384, 16385, 300, 40]
WHICH = [0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1]
SEAMS = (16, 1024, 16384)
NORM_NONE, HAP_NONE = (11, 12), (5, 12)             # VCF 11: no genome in the normalisation call, 5: in the haplotype call, 12: in both
PLANT = ("ACGTAC", "A")                             # a deletion of 5 bases no truth set holds and no genome spells: kept, open, cell 0
NEXT = ("AC", "GT")                                 # what the first records of the next VCF are: another row


def shape_table(n=128):
    """a row for every dictionary id the draws use (ids below n): 14 or more bases each, no two alike"""
    return vt.shapes_of(["ACGT"[i % 4] * (14 + i % 5) + "ACGT"[(i // 4) % 4] * (i % 3) for i in range(n)])


def plant(cols, sizes):
    """a kept line that is no TP on either side of every seam a VCF has and as its last record; the first records of every VCF
    spelled for another row.  Positions stay as they are: a sorted VCF stays sorted."""
    at = []
    for v, (c, n) in enumerate(zip(cols, sizes)):
        pos, ref, alt, qual, flags = c
        mine = [n - 1] + [i for s in SEAMS for i in (s - 1, s) if i < n]
        first = [i for i in range(min(n, 16)) if i not in mine]
        for i in first:
            ref[i], alt[i], flags[i] = nz.code(NEXT[0]), nz.code(NEXT[1]), 3
        for i in mine if n else []:
            ref[i], alt[i], flags[i] = nz.code(PLANT[0]), nz.code(PLANT[1]), 3
        if n > 40:                                       # behind the grid: two long alleles, no variant, no key -- kept lines all
            ref[20], alt[20], flags[20] = nz.DICT | 1, nz.DICT | 2, 3
            ref[21], alt[21], flags[21] = nz.code("ACG"), nz.code("ACG"), 3
            flags[22] = 3 | 4
        at.append(sorted(set(mine)) if n else [])
    return at


class Run:
    """one finished allele-extended batch with the four rescues (with their columns) behind it"""

    def __init__(self, engine, genomes, truths, cols, which, norm_none=(), hap_none=(), gap=None):
        self.engine = engine
        self.tids = [engine.truth_load(*t) for t in truths]
        self.gids = [engine.genome_load(g.encode()) for g in genomes]
        self.truths, self.which = truths, which
        self.b = engine.batch([len(c[0]) for c in cols], [self.tids[w] for w in which], alleles=True)
        try:
            for v, c in enumerate(cols):
                self.b.upload(v, *c)
            self.b.run()
            self.b.finish()
            self.gids_n = [-1 if v in norm_none else self.gids[w] for v, w in enumerate(which)]
            self.gids_h = [-1 if v in hap_none else self.gids[w] for v, w in enumerate(which)]
            self.gap = gap
        except Exception:
            self.close()
            raise

    def rescues(self):
        b = self.b
        b.normalize(self.gids_n, columns=True, fetch=False)
        b.atomize(columns=True, fetch=False)
        b.haplotypes(self.gids_h, gap=self.gap, columns=True, fetch=False)
        b.hapsubsets(columns=True, fetch=False)

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        for g in self.gids:
            self.engine.genome_release(g)


def compare(run, edges, shapes, subsets=True):
    """types and ladder with their columns, the pass, and its blocks against the restatement on the bytes the two left; the
    identities against their getters.  Returns (rec, tru, the bytes per VCF)."""
    b = run.b
    edges = vt.check_edges(edges)
    nr = vt.n_rows(edges)
    trec, ttru = b.vartype(edges, shapes, columns=True)
    lrec, ltru = b.ladder(subsets=subsets, columns=True)
    rec, tru = b.ladder_types()
    assert rec.shape == tru.shape == (b.n_vcf, nr, 18) and rec.dtype == np.uint64
    erows = [lt.entry_rows(t, edges, shapes) for t in run.truths]
    got = []
    for v in range(b.n_vcf):
        mask, emask = b.laddered(v)
        rows = b.vartyped(v)
        wrec, wtru = lt.counts(mask, emask, rows, erows[run.which[v]], nr)
        np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
        np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
        lt.identities(rec[v], tru[v], ladder=(lrec[v], ltru[v]), types=(trec[v], ttru[v]), edges=edges)
        got.append((mask, emask, rows))
    return rec, tru, got


# ---- the device against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_against_the_restatement(engine, sorted_):
    """13 VCFs on two truth sets (2000 entries on the planted genome, 65 on the 17-base one): two workgroups share the rows of
    the VCFs of 16 384 and 16 385 records, one workgroup meets several of the small ones; 8 bins with a shape table, 16 bins (84
    rows) without one, 1 bin without the subset search"""
    tvs, truths, cols = fam.family(43, sorted_, sizes=SIZES, which=WHICH)
    planted = plant(cols, SIZES)
    run = Run(engine, fam.GENOMES, truths, cols, WHICH, norm_none=NORM_NONE, hap_none=HAP_NONE)
    try:
        run.rescues()
        edges = vt.DEFAULT_EDGES
        names = vt.row_names(edges)
        rec, tru, got = compare(run, edges, shape_table())
        for v, at in enumerate(planted):                     # the planted lines: kept, open, in the row of their spelling
            mask, _, rows = got[v]
            for i in at:
                assert mask[i] & K and not mask[i] & S and names[rows[i]] == "DEL:5", (v, i)
            if SIZES[v] > 40:
                assert all(names[r] == "MNP:2" for r in rows[:8])
            if at and v + 1 < len(SIZES) and SIZES[v + 1]:
                assert int(rec[v + 1][names.index("MNP:2"), ld.KEPT]) >= 1
        assert all(int(rec[v][names.index("DEL:5"), ld.CELL0]) >= len(at) for v, at in enumerate(planted))
        assert not rec[0].any() and int(tru[0][:, ld.KEPT].sum()) == 2000          # the empty VCF: no line, every entry
        off = 5 * len(edges)
        assert sum(int(r[off + vt.LONGPAIR, ld.KEPT]) for r in rec) >= 1 and sum(int(r[off + vt.NOVAR, ld.KEPT]) for r in rec) >= 1
        assert sum(int(r[off + vt.NOKEY, ld.KEPT]) for r in rec) >= 1 and not any(r[off + vt.NOSHAPE].any() for r in rec)
        assert sum(int(r[:, ld.CELL0 + N].sum()) for r in rec) > 100 and sum(int(r[:, ld.CELL0 + A].sum()) for r in rec) > 100
        for v in NORM_NONE:
            assert not rec[v][:, [ld.CELL0 + m for m in range(16) if m & N]].any()
        for v in HAP_NONE:
            assert not rec[v][:, [ld.CELL0 + m for m in range(16) if m & (H | B)]].any()
        rec16, _, _ = compare(run, tuple(range(1, 17)), None)                      # 16 bins, 84 rows, no shape table
        assert rec16.shape[1] == 84 and sum(int(r[80 + vt.NOSHAPE, ld.KEPT]) for r in rec16) >= 1
        rec1, _, _ = compare(run, (1,), shape_table(), subsets=False)              # one bin; without the search
        assert rec1.shape[1] == 9 and not rec1[:, :, [ld.CELL0 + m for m in range(16) if m & B]].any()
        np.testing.assert_array_equal(rec1.sum(axis=1)[:, :2], rec.sum(axis=1)[:, :2])
    finally:
        run.close()


@pytest.mark.parametrize("seed", [7, 8])
def test_planted_family(engine, seed):
    """every cell the ladder reaches on the family (tests/test_laddertypes_host.py checks the draw) in at least one row: sorted,
    shuffled, a VCF without a genome in the normalisation call, one without in the haplotype call, every other record"""
    f = LadderFamily(seed)
    truth = truth_codes(f.truth)
    rng = np.random.default_rng(seed)
    cols = [f.columns(), f.columns(rng), f.columns(rng), f.columns(), f.columns(keep=range(0, len(f.recs), 2))]
    run = Run(engine, [f.genome], [truth], cols, [0] * 5, norm_none=(2,), hap_none=(3,))
    try:
        run.rescues()
        edges = vt.DEFAULT_EDGES
        rec, tru, got = compare(run, edges, None)
        for m in REACHED:
            assert rec[0][:, ld.CELL0 + m].any(), ld.set_name(m)
        np.testing.assert_array_equal(rec[0], rec[1])                               # shuffled: the same blocks
        np.testing.assert_array_equal(tru[0], tru[1])
        off = 5 * len(edges)
        assert int(rec[0][off + vt.NOSHAPE, ld.KEPT]) >= 1 and int(tru[0][off + vt.NOSHAPE, ld.KEPT]) >= 1
        rec_s, tru_s, _ = compare(run, edges, shape_table(256))                     # with a shape table: the long alleles get their rows
        assert not rec_s[0][off + vt.NOSHAPE].any() and not tru_s[0][off + vt.NOSHAPE].any()
        np.testing.assert_array_equal(rec_s.sum(axis=1), rec.sum(axis=1))
    finally:
        run.close()


@pytest.mark.parametrize("n", [1, 65])
def test_truth_set_sizes(engine, n):
    """truth sets of n entries on both genomes: one workgroup of k_ltype_truth per VCF, one lane or 65 of them at work"""
    rng = np.random.default_rng(700 + n)
    tvs = [fam.truth_set(g, rng, n) for g in fam.GENOMES]
    truths = [fam.codes(v) for v in tvs]
    assert all(len(nz.truth_order(*t)) == n for t in truths)
    which = [0, 1, 0, 1]
    cols = [fam.records(fam.GENOMES[w], rng, m, tvs[w], bool(v & 1)) for v, (m, w) in enumerate(zip([400, 400, 257, 1030], which))]
    run = Run(engine, fam.GENOMES, truths, cols, which)
    try:
        run.rescues()
        _, tru, _ = compare(run, (1, 2, 6), shape_table())
        assert all(int(t[:, ld.KEPT].sum()) == n for t in tru)
    finally:
        run.close()


def test_4096_lines_in_one_cell_and_70000_in_the_hot_one(engine):
    """the deletion of one A from the 70-base run at 101, spelled at sixteen places, 4096 times: cell N of DEL:1 takes them all;
    one truth SNV called 70 000 times: (SNV:1, TP), past 16 bits"""
    g = fam.G600
    n, m = 4096, 70000
    pos = np.array([101 + (i * 7) % 16 for i in range(n)], np.int32)
    dels = (pos, np.full(n, nz.code("AA"), np.int32), np.full(n, nz.code("A"), np.int32), np.full(n, 50, np.float32), np.full(n, 3, np.uint8))
    alt = "ACGT"[("ACGT".index(g[299]) + 1) % 4]
    snvs = (np.full(m, 300, np.int32), np.full(m, nz.code(g[299]), np.int32), np.full(m, nz.code(alt), np.int32), np.full(m, 50, np.float32),
            np.full(m, 3, np.uint8))
    truth = fam.codes([(100, "TA", "T"), (300, g[299], alt)])
    run = Run(engine, [g], [truth], [dels, snvs], [0, 0])
    try:
        run.rescues()
        edges = vt.DEFAULT_EDGES
        names = vt.row_names(edges)
        rec, tru, got = compare(run, edges, None)
        want = np.zeros((len(names), 18), np.uint64)
        want[names.index("DEL:1"), [ld.KEPT, ld.CELL0 + N]] = n
        np.testing.assert_array_equal(rec[0], want)
        want[:] = 0
        want[names.index("SNV:1"), [ld.KEPT, ld.TP]] = m
        np.testing.assert_array_equal(rec[1], want)
        assert int(tru[0][names.index("DEL:1"), ld.CELL0 + N]) == 1 and int(tru[0][names.index("SNV:1"), ld.CELL0]) == 1
        assert int(tru[1][names.index("SNV:1"), ld.TP]) == 1 and int(tru[1][names.index("DEL:1"), ld.CELL0]) == 1
    finally:
        run.close()


# ---- state and argument errors ------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    tvs, truths, cols = fam.family(49, True, sizes=[40, 40], which=[0, 0], truth_n=[50, 20])
    run = Run(engine, fam.GENOMES, truths, cols, [0, 0])
    b = run.b
    sb = engine.batch([40], [run.tids[0]])                     # a single-base batch
    none = "qm_batch_get_ladder_types: no qm_batch_ladder_types behind the latest run of its producers"
    no_types = "qm_batch_ladder_types: needs qm_batch_types(.., QM_TYPE_COLUMNS) behind the latest run"
    no_ladder = "qm_batch_ladder_types: needs qm_batch_ladder(.., QM_LADDER_COLUMNS) behind the latest run of its producers"
    try:
        code, msg = refused(b.ladder_type_counts)               # before the pass
        assert code == QM_E_STATE and msg.endswith(none)
        # each producer missing, or run without its columns: the first one missing, types before ladder, is named
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and msg.endswith(no_types)
        run.rescues()
        b.ladder(subsets=True, columns=True)
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and msg.endswith(no_types)
        b.vartype()                                             # without the row bytes: not the producer
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and msg.endswith(no_types)
        b.vartype(columns=True)
        b.ladder(subsets=True)                                  # without the mask bytes: not the producer
        before = b.device_bytes
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and msg.endswith(no_ladder)
        assert b.device_bytes == before                         # a refused call allocates nothing
        b.ladder(subsets=True, columns=True)
        full = b.ladder_types()                                 # served behind both
        assert b.device_bytes > before                          # the pass's array is counted
        for x, y in zip(b.ladder_type_counts(), full):
            np.testing.assert_array_equal(x, y)
        nr = _lib.C.c_int(0)
        assert b._L.qm_batch_get_ladder_types(b._h, None, None, _lib.C.byref(nr)) == 0 and nr.value == 44
        # behind each of the six calls underneath made again: refused until the pass is run again
        again = {"types": lambda: b.vartype(columns=True), "ladder": lambda: b.ladder(subsets=True, columns=True),
                 "normalize": lambda: b.normalize(run.gids_n, columns=True), "atomize": lambda: b.atomize(columns=True),
                 "haplotypes": lambda: b.haplotypes(run.gids_h, columns=True), "hapsubsets": lambda: b.hapsubsets(columns=True)}
        for name, call in again.items():
            call()
            code, msg = refused(b.ladder_type_counts)
            assert code == QM_E_STATE and msg.endswith(none), name
            if name in ("normalize", "atomize", "haplotypes", "hapsubsets"):   # ... which forgot the ladder too
                code, msg = refused(b.ladder_types)
                assert code == QM_E_STATE and msg.endswith(no_ladder), name
                if name == "haplotypes":
                    b.hapsubsets(columns=True)
                b.ladder(subsets=True, columns=True)
            for x, y in zip(b.ladder_types(), full):
                np.testing.assert_array_equal(x, y)
        code, msg = refused(b.ladder_type_timings)              # the timings with timing off
        assert code == QM_E_STATE and msg.endswith("qm_batch_ladder_types_timings: timing is off")
        b.set_timing(True)
        b.ladder_types()
        ms = b.ladder_type_timings()
        assert set(ms) == {"ltype_records_ms", "ltype_truth_ms"} and all(x >= 0 for x in ms.values())
        b.set_timing(False)
        b.run()                                                 # behind a new run
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and "qm_batch_finish first" in msg
        b.finish()
        code, msg = refused(b.ladder_types)
        assert code == QM_E_STATE and msg.endswith(no_types)
        code, msg = refused(b.ladder_type_counts)
        assert code == QM_E_STATE and msg.endswith(none)
        code, msg = refused(b.ladder_type_timings)
        assert code == QM_E_STATE and "no qm_batch_ladder_types behind the latest run of its producers" in msg
        sb.upload(0, *[x if i < 1 or i > 2 else (x & 3).astype(np.int32) for i, x in enumerate(cols[0])])
        sb.run()
        sb.finish()
        code, msg = refused(sb.ladder_types)
        assert code == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b._L.qm_batch_get_ladder_types(None, None, None, None) == QM_E_INVAL
        assert b._L.qm_batch_ladder_types(None, None) == QM_E_STATE
    finally:
        sb.close()
        run.close()
