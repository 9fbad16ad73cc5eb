"""The edge families of haplo_subset_edges.py on the host: every planted case is present in the restatement's
output, and the restatement is not the only judge of these shapes -- on every searched site of every family the double loop over
all pairs of subsets, substituting into the whole genome by plain slicing, gives the restatement's masks or None for NOSUBSET.
Beside them: the order of forms against a sort over plain strings, the emulation of the narrow hash against its definition, the
identities of the count block.  No GPU: this file passes before a device run is worth making."""
import numpy as np
import pytest

import haplo_subset_edges as se
from quasimodo_amd import haplo as hp

U = {name: k for k, name in enumerate(hp.SUB_COLS)}
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}
SEARCHED = {"hash": 77, "verify": 6, "order": 15, "rounds": 64, "ties": 4, "items": 7, "edges": 15, "right260": 1, "right263": 1,
            "right264": 1}                                     # the searched sites of the VCFs as planted, at gap 10


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name):
        if name not in cache:
            e = se.family(name)
            cache[name] = (e, se.restate_all(e))
        return cache[name]
    return get


@pytest.mark.parametrize("name", se.NAMES)
def test_the_planted_cases_are_present(restated, name):
    e, res = restated(name)
    se.PRESENT[name](e, res)
    assert len(e.genome) <= 20000
    planted = sum(int(sub[U["searched"]]) for (v, gap), (_, (sub, _, _, _)) in res.items() if gap == se.GAP and v not in e.twin)
    assert planted == SEARCHED[name]


@pytest.mark.parametrize("name", se.NAMES)
def test_the_double_loop_confirms_every_optimum_and_every_nosubset(restated, name):
    e, res = restated(name)
    searched, partial = se.judge(e, res)
    assert searched >= SEARCHED[name] and partial > 0


@pytest.mark.parametrize("name", se.NAMES)
def test_the_identities_of_the_count_block(restated, name):
    e, res = restated(name)
    for (v, gap), ((rec, tru, cls, site, ecls, tried), (sub, cls_s, ecls_s, chosen)) in res.items():
        s = [int(x) for x in sub]
        assert s[U["searched"]] == s[U["partial"]] + s[U["nosubset"]] == sum(d[3] in hp.SEARCHED_OUTCOMES for d in tried)
        assert s[U["rescued_s"]] == int((cls_s == hp.SUBSET).sum()) and s[U["left_lines"]] == int((cls_s == hp.LEFT).sum())
        assert s[U["found_s"]] - int(tru[T["found_h"]]) == int((ecls_s == hp.SUBSET).sum())
        assert s[U["left_entries"]] == int((ecls_s == hp.LEFT).sum())
        flags = e.cols[v][4]
        with_id = sum(bool(flags[i] & hp.F_IDDOT) for d in chosen for i in d[3])
        assert s[U["tp_s"]] - int(rec[R["tp_h"]]) == with_id                   # no planted line is a TP line
        for d in chosen:                                                        # an item is in iff its form is in
            fa = hp.forms(se.site_sides(e, v, [t for t in tried if t[0] == d[0]][0])[0])
            assert sorted({hp.trim(*x) for x in se.spelled(e, v, d[3])}, key=hp.form_key) == hp.subset(fa, d[1])


def test_the_order_of_forms_against_a_sort_over_plain_strings(restated):
    """hp.forms on every side of the `order` family against sorted() on (q, len(r), len(a), a) over plain strings -- and the packed
    number of an ALT, where the highest differing base decides, orders at least one pair of every side of eight the other way"""
    e, res = restated("order")
    (rec, tru, cls, site, ecls, tried), _ = res[(0, se.GAP)]
    n = other_way = 0
    for d in tried:
        for side in se.site_sides(e, 0, d):
            fs = hp.forms(list(side))
            assert fs == sorted(se.plain_forms(side), key=lambda f: (f[0], len(f[1]), len(f[2]), f[2])) == se.plain_forms(side)
            n += 1
            if len(fs) == 8:
                by_number = sorted(fs, key=lambda f: (f[0], len(f[1]), len(f[2]), se.packed(f[2])))
                other_way += by_number != fs
    assert n == 30 and other_way >= 7


def test_the_emulated_narrow_hash_is_the_polynomial_of_the_definition():
    """narrow_hash against the closed form sum(sym_i B^(n - 1 - i)) mod 2^32, top four bits; a hash composed from a prefix, an
    ALT piece and a suffix as k_hap_subsets composes it equals the hash of the whole"""
    B, M = 0x9E3779B1, 1 << 32
    rng = np.random.default_rng(5)
    full = lambda s: sum((se.BASES.index(c) + 1) * pow(B, len(s) - 1 - i, M) for i, c in enumerate(s)) % M
    for n in (1, 4, 63, 64, 65, 257, 352):
        s = "".join(se.BASES[i] for i in rng.integers(0, 4, n))
        assert se.narrow_hash(s) == full(s) >> 28
        i, j = sorted(int(x) for x in rng.integers(0, n + 1, 2))
        h = full(s[:i])
        h = (h * pow(B, j - i, M) + full(s[i:j])) % M
        h = (h * pow(B, n - j, M) + full(s[:n]) - full(s[:j]) * pow(B, n - j, M)) % M
        assert h == full(s)
    assert se.narrow_hash("A") == 0 and se.narrow_hash("T" + "A" * 7) == (4 * pow(B, 7, M) + full("A" * 7)) % M >> 28


def test_every_candidate_of_the_tie_sites():
    """`candidates` lists what `brute` chooses from: its first row is brute's answer on every searched site of `ties` and `items`"""
    for name in ("ties", "items"):
        e = se.family(name)
        res = se.restate_all(e)
        G = hp.symbols(e.genome)
        for (v, gap), ((_, _, _, _, _, tried), _) in res.items():
            for d in tried:
                if d[3] in hp.SEARCHED_OUTCOMES:
                    sides = se.site_sides(e, v, d)
                    cands = se.candidates(G, *sides)
                    assert (cands[0][2:] if cands else None) == se.brute(G, *sides)
                    assert cands == sorted(cands, key=lambda c: (-c[0], -c[1], c[2], c[3])) and len(set(cands)) == len(cands)
