"""The edge families of haplo_edges.py on the host: every planted case is present in the restatement's output;
and the restatement is not the only judge of these shapes -- MATCH holds iff substituting each side's variants into the whole
genome by plain slicing gives one string, the trimmed forms equal a loop over characters, the site partition equals a direct
loop over the definition, and a record's site equals a linear search for the first window that ends at or behind it.  No GPU:
this file passes before a device run is worth making."""
import numpy as np
import pytest

import haplo_edges as he
from quasimodo_amd import haplo as hp

R, T = he.R, he.T


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name):
        if name not in cache:
            e = he.family(name)
            cache[name] = (e, {(v, gap): e.restate(v, gap) for v, vc in enumerate(e.vcfs) if vc[3] for gap in e.gaps})
        return cache[name]
    return get


@pytest.mark.parametrize("name", he.NAMES)
def test_the_planted_cases_are_present(restated, name):
    e, res = restated(name)
    he.PRESENT[name](e, res)
    assert max(len(o) for o in e.order) <= 10500 and max(len(v[2]) for v in e.vcfs) <= 40000 and len(e.genome) <= 100000
    for (v, gap), (rec, tru, cls, site, ecls, detail) in res.items():    # the ties of the tables among themselves
        assert int(rec[R["tp_h"]]) - int(rec[R["tp"]]) == int(rec[R["rescued"]]), (name, v, gap)
        assert int(tru[T["tried"]]) == len(detail) and int(tru[T["matched"]]) == sum(d[3] == hp.MATCH for d in detail)


def form(v):
    """the trimmed form of a spelling, by the loop over characters"""
    p, ref, alt = v
    cp, cs = he.strip(ref, alt)
    return p + cp, ref[cp:len(ref) - cs], alt[cp:len(alt) - cs]


def whole(G, forms):
    """the whole genome with trimmed forms applied from the right by plain slicing (insertions at one point behind a replaced
    base keep the order (q, |r|) of the definition)"""
    s = G
    for q, r, a in sorted(forms, key=lambda t: (t[0], len(t[1])), reverse=True):
        assert s[q - 1:q - 1 + len(r)] == r
        s = s[:q - 1] + a + s[q - 1 + len(r):]
    return s


@pytest.mark.parametrize("name", he.NAMES)
def test_match_iff_the_whole_genomes_are_equal(restated, name):
    e, res = restated(name)
    G = hp.symbols(e.genome)
    seen = set()
    for (v, gap), (rec, tru, cls, site, ecls, detail) in res.items():
        c, ent = e.cols[v], e.order[e.vcfs[v][1]]
        for s, ws, we, what, recs, ents, x, y in detail:
            if what not in (hp.MATCH, hp.MISMATCH):
                continue
            a = whole(G, {form((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i]))) for i in recs})
            b = whole(G, {form((ent[j][0], hp.spell(ent[j][1]), hp.spell(ent[j][2]))) for j in ents})
            assert (a == b) == (what == hp.MATCH), (name, e.vcfs[v][0], gap, s, ws, we)
            seen.add(what)
    assert seen == {hp.MATCH, hp.MISMATCH}, name


def test_trimmed_forms_against_the_loop_over_characters(restated):
    e, res = restated("trim")
    ent = [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[0]]
    for p, ref, alt, cp, cs in e.planted["forms"]:
        assert hp.trim(p, ref, alt) == (p + cp, ref[cp:len(ref) - cs], alt[cp:len(alt) - cs]) == form((p, ref, alt))
    for p, ref, alt, _, _ in e.vcfs[0][2]:
        if len(ref) <= hp.INLINE_MAX and len(alt) <= hp.INLINE_MAX:
            assert hp.trim(p, ref, alt) == form((p, ref, alt))
    # g = 0: the window of a single-entry site is the entry's footprint -- q and |r| come back through the site table
    first, lo, hi = hp.truth_sites(e.genome, e.tcodes[0], 0)
    usable = [j for j, v in enumerate(ent) if v[1] is not None and v[2] is not None]
    assert first.tolist() == usable and len(usable) == len(e.planted["forms"])
    for j, a, b in zip(usable, lo.tolist(), hi.tolist()):
        q, r, _ = form(ent[j])
        assert (a, b) == (q, max(q, q + len(r) - 1)), ent[j]
    assert {len(form(v)[1]) for v in ent if v[1] is not None and v[2] is not None} == set(range(14))


def usable_by_definition(G, v):
    p, ref, alt = v
    return ref is not None and alt is not None and ref != alt and p >= 1 and p + len(ref) - 1 <= len(G) and all(G[p - 1 + k] == c for k, c in enumerate(ref))


def partition(G, ent, gap):
    """The definition, walked directly: the usable entries in table order; an entry joins the current site iff its lo <= the
    largest hi so far + 2 g.  Returns (the site of every entry or -1, [(first entry, window lo, window hi)])."""
    site_of, out, top = [], [], None
    for j, v in enumerate(ent):
        if not usable_by_definition(G, v):
            site_of.append(-1)
            continue
        q, r, _ = form(v)
        lo, hi = q, max(q, q + len(r) - 1)
        if top is not None and lo <= top + 2 * gap:
            f, a, b = out[-1]
            out[-1] = (f, min(a, lo), max(b, hi))
        else:
            out.append((j, lo, hi))
        top = hi if top is None else max(top, hi)
        site_of.append(len(out) - 1)
    return site_of, [(f, max(1, a - gap), min(len(G) + 1, b + gap)) for f, a, b in out]


@pytest.mark.parametrize("name", he.NAMES)
def test_the_site_partition_against_the_definition(restated, name):
    e, res = restated(name)
    G = hp.symbols(e.genome)
    for w, order in enumerate(e.order):
        ent = [(p, hp.spell(r), hp.spell(a)) for p, r, a in order]
        for gap in e.gaps:
            site_of, table = partition(G, ent, gap)
            assert hp.sites(G, ent, gap) == (site_of, table), (name, w, gap)
            first, lo, hi = hp.truth_sites(e.genome, e.tcodes[w], gap)
            assert list(zip(first.tolist(), lo.tolist(), hi.tolist())) == table
            assert all(b[2] >= a[2] for a, b in zip(table, table[1:]))          # window ends never descend
            for v, vc in enumerate(e.vcfs):                     # a record's site: the first window that ends at or behind its hi, if it holds it
                if vc[1] != w or not vc[3] or len(vc[2]) * len(table) > 5000000:      # (the linear search is quadratic: not on the largest family)
                    continue
                got = res[(v, gap)][3].tolist()
                for i, (p, ref, alt, _, extra) in enumerate(vc[2]):
                    long = len(ref) > hp.INLINE_MAX or len(alt) > hp.INLINE_MAX
                    want = -1
                    if not long and not extra & hp.F_NOKEY and usable_by_definition(G, (p, ref, alt)):
                        q, r, _ = form((p, ref, alt))
                        k = next((k for k, t in enumerate(table) if t[2] >= max(q, q + len(r) - 1)), None)
                        want = k if k is not None and table[k][1] <= q else -1
                    assert got[i] == want, (name, vc[0], gap, i)


@pytest.mark.parametrize("name", he.NAMES)
def test_shuffled_records_give_the_same_counts_and_classes(restated, name):
    e, res = restated(name)
    assert e.twin
    for t, (v, perm) in e.twin.items():
        for gap in e.gaps:
            a, b = res[(v, gap)], res[(t, gap)]
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2][perm], b[2])
            np.testing.assert_array_equal(a[3][perm], b[3])
            np.testing.assert_array_equal(a[4], b[4])


def test_one_variant_per_side_is_a_match_iff_the_normal_forms_agree(restated):
    """the tie the device test holds between the two passes, here between the two restatements"""
    from haplo_family import host_masks
    from quasimodo_amd import normalize as nm
    e, res = restated("trim")
    for v in (0, 1):
        c = e.cols[v]
        out = nm.counts(e.genome, e.tcodes[0], c[0], c[1], c[2], c[4], *host_masks(c, e.tcodes[0]))
        for gap in e.gaps:
            rec, tru, cls, site, ecls, detail = res[(v, gap)]
            he.check_normal_form_tie(e, v, gap, (cls, site, ecls), hp.truth_sites(e.genome, e.tcodes[0], gap)[0], out[2], out[6])
