"""The edge families of allele_edges.py on the host: every planted case is present in the restatements'
output -- the wrap of both hash tables among them, from the hashes and the slot rule restated in Python --; and the restatements
are not the only judges of these shapes: vt.shape_codes against vt.shape on strings, nz.normalize against sequence equality by
plain slicing, the atom restatement against a loop over characters, the simulated tables against a Python set, and the ties that
hold between the three passes.  No GPU: this file passes before a device run is worth making."""
import numpy as np
import pytest

import allele_edges as ae
from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd import vartype as vt


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name):
        if name not in cache:
            f = ae.family(name)
            cache[name] = (f, {v: f.restate(v) for v in range(len(f.vcfs))})
        return cache[name]
    return get


@pytest.mark.parametrize("name", ae.NAMES)
def test_the_planted_cases_are_present(restated, name):
    f, res = restated(name)
    ae.PRESENT[name](f, res)
    for v, (nzc, atc, ty) in res.items():                       # the ties of the tables among themselves
        if nzc is not None:
            assert int(nzc[0][ae.NR["tp_n"]]) - int(nzc[0][ae.NR["tp"]]) == int(nzc[0][ae.NR["rescued"]]), (name, v)
            assert int(nzc[0][ae.NR["kept"]]) == int(atc[0][ae.AR["kept"]]) == int(ty[f.edges[0]][0][:, 0].sum())
        assert int(atc[0][ae.AR["tp_a"]]) - int(atc[0][ae.AR["tp"]]) == int(atc[0][ae.AR["rescued"]]), (name, v)
        assert int(atc[1][ae.AT["found"]]) == int(ty[f.edges[0]][1][:, 1].sum())


@pytest.mark.parametrize("name", ae.NAMES)
def test_the_ties_between_the_passes(restated, name):
    """type and size are invariant under normalisation, so are the atoms of equal-length records; no record is left out by rule"""
    f, res = restated(name)
    judged = 0
    for v, vc in enumerate(f.vcfs):
        if vc[3]:
            nzc, atc, ty = res[v]
            judged += ae.check_ties(f, v, nzc[3:6], nzc[2], atc[3], ty[f.edges[0]][2])
    left_out = sum(f.reasons[vc[0]] for vc in f.vcfs if vc[3]) if f.reasons else 0
    assert judged == sum(len(c[0]) for c, vc in zip(f.cols, f.vcfs) if vc[3]) - left_out
    assert judged > 0 or name == "longshort"                    # (every record of that family is LONG to the normal-form pass)


@pytest.mark.parametrize("name", [n for n in ae.NAMES if n not in ("walk", "longshort")])
def test_equal_forms_iff_equal_sequences(restated, name):
    """nz.normalize against brute force: two variants share a form iff substituting them into the genome gives one string"""
    f, res = restated(name)
    n = 0
    for v, vc in enumerate(f.vcfs):
        if vc[3]:
            n += ae.check_partition(f, v, res[v][0][3:6], res[v][0][2], res[v][0][6])
    assert n >= 10                                              # records that share the form of an entry


@pytest.mark.parametrize("name", ["pairs", "longshort"])
def test_shape_codes_against_shape_on_strings(restated, name):
    f, res = restated(name)
    n = 0
    for v in range(len(f.vcfs)):
        rows = {e: res[v][2][e][2] for e in f.edges}
        for i, ((_, r, a), rc, ac) in enumerate(zip(f.strings(v), f.cols[v][1].tolist(), f.cols[v][2].tolist())):
            if r is None or a is None or r == a or (len(r) > 13 and len(a) > 13):
                assert vt.shape_codes(rc, ac, f.shapes)[0] is None
                continue
            kind, size = vt.shape(r, a)
            assert vt.shape_codes(rc, ac, f.shapes) == (kind, size), (name, i, r, a)
            for e in f.edges:
                assert rows[e][i] == vt.row_of(kind, size, vt.check_edges(e)), (name, i, e)
            n += 1
    assert n >= 2900


@pytest.mark.parametrize("name", [n for n in ae.NAMES if n not in ("walk", "longshort")])
def test_the_atom_restatement_against_a_loop_over_characters(restated, name):
    f, res = restated(name)
    n_multi = 0
    for v in range(len(f.vcfs)):
        w = f.vcfs[v][1]
        held = set()
        for p, r, a in f.order[w]:
            r, a = nz.spell(r), nz.spell(a)
            if r is not None and a is not None and len(r) == len(a):
                held |= {(p + k, r[k], a[k]) for k in range(len(r)) if r[k] != a[k]}
        _, _, cls, na, hm = res[v][1]
        for i, (p, r, a) in enumerate(f.strings(v)):
            ok = r is not None and a is not None and len(r) <= 13 and len(a) <= 13 and len(r) == len(a) and r != a and not f.cols[v][4][i] & nz.F_NOKEY
            if not ok:
                assert cls[i] >= at.RESCUED and na[i] == 0 and hm[i] == 0, (name, v, i)
                continue
            assert na[i] == ae.hamming(r, a) and hm[i] == sum(1 << k for k in range(len(r)) if r[k] != a[k] and (p + k, r[k], a[k]) in held), (name, v, i)
            n_multi += na[i] >= 2
    assert n_multi >= 6 or name not in ("pairs", "tables")     # (the other families hold no MNP)


def test_the_simulated_tables_against_a_set(restated):
    """the probe of the simulated tables finds a key iff a Python set holds it: every record's form and atoms, every entry's"""
    f, res = restated("tables")
    hit = miss = 0
    for v, vc in enumerate(f.vcfs):
        if not vc[3]:
            continue
        (fs, ft), (as_, atab) = ae.tables_of(f, vc[1])
        forms, atoms = set(ft.values()), set(atab.values())
        assert len(forms) == len(ft) <= fs // 2 and len(atoms) == len(atab) <= as_ // 2
        nzc = res[v][0]
        for i, (p, r, a) in enumerate(zip(*[x.tolist() for x in nzc[3:6]])):
            slot = ae.probe(ft, fs, ae.FORM_HOME, (p, r, a))[0]
            assert (slot >= 0) == ((p, r, a) in forms) == (nzc[6][i] >= 0), (vc[0], i)
            hit, miss = hit + (slot >= 0), miss + (slot < 0)
        for p, r, a in f.strings(v):
            for k in range(len(r)) if len(r) == len(a) else ():
                if r[k] != a[k]:
                    key = at.atom_key(p + k, r[k], a[k])
                    assert (ae.probe(atab, as_, ae.ATOM_HOME, key)[0] >= 0) == (key in atoms)
    assert hit >= 800 and miss >= 300


@pytest.mark.parametrize("name", ae.NAMES)
def test_shuffled_records_give_the_same_counts_and_rows(restated, name):
    f, res = restated(name)
    assert f.twin
    for t, (v, perm) in f.twin.items():
        a, b = res[v], res[t]
        for x, y in zip(a[0][:2] + a[1][:2], b[0][:2] + b[1][:2]):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a[0][2:] + a[1][2:], b[0][2:] + b[1][2:]):
            np.testing.assert_array_equal(x[perm], y)
        for e in f.edges:
            np.testing.assert_array_equal(a[2][e][0], b[2][e][0])
            np.testing.assert_array_equal(a[2][e][1], b[2][e][1])
            np.testing.assert_array_equal(a[2][e][2][perm], b[2][e][2])
