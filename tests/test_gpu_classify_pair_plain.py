"""The plain path of k_classify_pair (a full pair of 512 live, strictly ascending records runs through
specialisations without liveness selects, order tests and the walk of a run) against the oracle, through the public batch path.
Every case starts from strictly ascending, live records -- so the plain path runs -- and plants ONE violation: the pairs around
it stay plain, its own pair must fall back to the general path.  Needs an MI355X."""
import numpy as np
import pytest

from test_gpu_classify_pair import IDDOT, NOKEY, PASS, _cols, _run, _truth, check_vcf

pytestmark = pytest.mark.gpu

TPLINE = 8
N3 = 3000                      # under three tiles: pairs 0 .. 4 full, pair 5 ragged
SPAN = 16384


def _kept(c):
    """the PASS bit as everywhere: single-base and floor(QUAL) >= 20 (NaN: not kept)"""
    snp = (c[1] >= 0) & (c[1] < 4) & (c[2] >= 0) & (c[2] < 4)
    with np.errstate(invalid="ignore"):
        c[4] = ((c[4] & ~np.uint8(PASS)) | (snp & (np.floor(c[3]) >= 20)).astype(np.uint8)).astype(np.uint8)
    return c


def _plain(rng, n, start=50):
    """n live records on strictly ascending positions (steps of 2 .. 5: room for a descent of one), random single-base alleles,
    QUALs on both sides of the threshold, a few IDs other than '.', NOKEY and TPLINE records"""
    pos = (start + np.cumsum(rng.integers(2, 6, n))).astype(np.int32)
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = rng.integers(0, 4, n).astype(np.int32)
    qual = rng.integers(0, 300, n).astype(np.float32)
    flags = ((rng.random(n) > 0.1).astype(np.uint8) * IDDOT) | ((rng.random(n) < 0.03).astype(np.uint8) * NOKEY) | \
            ((rng.random(n) < 0.03).astype(np.uint8) * TPLINE)
    return _kept([pos, ref, alt, qual, flags.astype(np.uint8)])


def _truth_of(rng, c, frac=0.1, extra=()):
    """the keys of a share of the records, keys on a record's position with another allele, keys between two records: about
    175 keys per tile of 1 024 records, under the 256 a slice holds, so that no tile is oversize and its full pairs can be plain"""
    n = len(c[0])
    keys = list(extra)
    if n:
        take = np.nonzero(rng.random(n) < frac)[0]
        keys += [(int(c[0][i]), int(c[1][i]) & 3, int(c[2][i]) & 3) for i in take]
        near = np.nonzero(rng.random(n) < 0.04)[0]
        keys += [(int(c[0][i]), int(c[1][i]) & 3, (int(c[2][i]) + 1) & 3) for i in near]
        keys += [(int(c[0][i]) + 1, 0, 1) for i in np.nonzero(rng.random(n) < 0.03)[0]]
    keys.append((1, 0, 1))                       # never empty
    return _truth([k for k in keys if 0 <= k[0] < (1 << 28)])


def _copy(c):
    return [a.copy() for a in c]


SLICE = 256                    # truth keys a tile's LDS slice holds (K1_SLICE): a tile with more in its range is joined round by round


def _tile_keys(c, t):
    """truth keys in the range of every tile of 1 024 records, counted as the kernel counts them: through the coarse index
    (cells of 1 << shift positions, at most 65 536 of them) over the tile's first and last position, clamped behind the last cell"""
    pos, tpos = np.asarray(c[0]), np.sort(np.asarray(t[0]).astype(np.int64))
    shift = 0
    while (int(tpos[-1]) >> shift) >= (1 << 16):
        shift += 1
    lim = (int(tpos[-1]) >> shift) + 1
    cells = tpos >> shift
    out = []
    for tb in range(0, len(pos), 1024):
        a, b = int(pos[tb]) & 0xffffffff, int(pos[min(tb + 1024, len(pos)) - 1]) & 0xffffffff
        lo = np.searchsorted(cells, min(a >> shift, lim), "left")
        hi = np.searchsorted(cells, min((b >> shift) + 1, lim), "left")
        out.append(max(int(hi - lo), 0))
    return out


def _run_plain(engine, oracle, cols, truths, oversize=(), **kw):
    """_run, behind the host-side check that no tile (but those named in `oversize`) is above the slice cap: otherwise the pair
    loop never asks whether a pair is plain"""
    for c, t in zip(cols, truths):
        for i, k in enumerate(_tile_keys(c, t)):
            assert (k > SLICE) == (i in oversize), ("tile %d holds %d truth keys" % (i, k))
    return _run(engine, oracle, cols, truths, **kw)


# record k and its predecessor: every in-lane slot, the lane seam, the half seam, the pair seam, the tile seam, the span seam
PLACES = {"lane_0|1": 21, "lane_1|2": 22, "lane_2|3": 23, "lane_seam_3|4": 24, "second_half_lane_1|2": 256 + 4 * 63 + 2,
          "half_seam": 256, "pair_seam": 512, "tile_seam": 1024, "span_seam": SPAN}


def _n_for(k):
    return SPAN + 512 if k >= SPAN else N3


@pytest.mark.parametrize("place", sorted(PLACES))
def test_one_equal_position(engine, oracle, place):
    """Record k on its predecessor's position: the same key twice (in the truth set and outside it: the repeated kept key is
    counted once) and two keys on one position."""
    k = PLACES[place]
    rng = np.random.default_rng(3100 + k)
    base = _plain(rng, _n_for(k))
    cols, truths = [], []
    for same_key in (True, False):
        c = _copy(base)
        c[0][k] = c[0][k - 1]
        for i in (k - 1, k):
            c[1][i] = 0; c[2][i] = 1 if same_key or i == k else 2
            c[3][i] = 40 + (i & 7); c[4][i] = PASS | IDDOT
        key = (int(c[0][k]), 0, 1)
        for t in (_truth_of(rng, c, extra=[key]), _truth([x for x in zip(*map(np.ndarray.tolist, _truth_of(rng, c))) if x[0] != key[0]])):
            cols.append(_cols(*c)); truths.append(t)
    _run_plain(engine, oracle, cols, truths, expect_sorted=True)


@pytest.mark.parametrize("place", sorted(PLACES))
def test_one_descent(engine, oracle, place):
    """Record k one below its predecessor: the VCF is flagged and redone, every output as the oracle's."""
    k = PLACES[place]
    rng = np.random.default_rng(3200 + k)
    c = _plain(rng, _n_for(k))
    c[0][k] = c[0][k - 1] - 1
    _run_plain(engine, oracle, [_cols(*c)], [_truth_of(rng, c)], expect_sorted=False)


@pytest.mark.parametrize("lane", [0, 63])
def test_one_dead_allele_byte(engine, oracle, lane):
    """A REF or ALT code that is no single base in each of the lane's eight records of a pair (four per half)."""
    rng = np.random.default_rng(3300 + lane)
    base = _plain(rng, 1500)
    t = _truth_of(rng, base)
    cols = []
    for s in range(8):
        c = _copy(base)
        i = 512 + (256 if s >= 4 else 0) + 4 * lane + (s & 3)          # pair 1 of tile 0: pair 0 before and pair 2 behind stay plain
        if s & 1:
            c[2][i] = 4 + s
        else:
            c[1][i] = 4
        cols.append(_cols(*_kept(c)))
    _run_plain(engine, oracle, cols, [t] * len(cols))


@pytest.mark.parametrize("case", ["tail_2^28", "last_of_pair_2^28", "first_negative", "inner_negative"])
def test_position_out_of_range(engine, case):
    """Positions outside [0, 2^28) that keep the records ascending (a tail at and above 2^28, a negative first record) and one
    that does not: the batch is refused, as on the general path."""
    import quasimodo_amd as q
    rng = np.random.default_rng(3400)
    c = _plain(rng, 1024)
    if case == "tail_2^28":
        c[0][700:] = (1 << 28) + np.arange(1024 - 700, dtype=np.int32)
    elif case == "last_of_pair_2^28":
        c[0][1023] = 1 << 28
    elif case == "first_negative":
        c[0][0] = -5
    else:
        c[0][700] = -1
    t = _truth_of(rng, c)
    assert _tile_keys(c, t)[0] <= SLICE            # not oversize: the pair comes to the plain test, whose position-OR clause refuses it
    tid = engine.truth_load(*t)
    try:
        with pytest.raises(q.QmvtError) as ei:
            engine.classify_batch([_cols(*c)], [tid])
        assert ei.value.code == -5
    finally:
        engine.truth_release(tid)


def test_ragged_ends(engine, oracle):
    """A last pair short of 512 records is never plain; the full pairs before it are."""
    rng = np.random.default_rng(3500)
    cols, truths = [], []
    for n in (511, 512, 513, 767, 1025):
        c = _plain(rng, n)
        cols.append(_cols(*c)); truths.append(_truth_of(rng, c))
    _run_plain(engine, oracle, cols, truths)


EDGE_VARIANTS = {"kept": PASS | IDDOT, "nokey": PASS | IDDOT | NOKEY, "id": PASS, "tpline": PASS | TPLINE, "tpline_dot": PASS | IDDOT | TPLINE,
                 "not_pass": IDDOT}


@pytest.mark.parametrize("seam", [None, 512, 1024])
def test_truth_keys_on_the_first_and_last_record_of_a_pair(engine, oracle, seam):
    """Keys on records 0 and 511 of every pair, matching and on the same position with another allele, the records kept, NOKEY,
    with an ID, TPLINE, not PASS.  With a seam: record `seam` sits on the position of record seam - 1, the last of a plain pair,
    so the run of that key goes on into the next pair (511|512) or the next tile (1 023|1 024)."""
    rng = np.random.default_rng(3600 + (seam or 0))
    base = _plain(rng, N3)
    if seam:
        base[0][seam] = base[0][seam - 1]
    edges = [i for p in range(0, N3, 512) for i in (p, min(p + 511, N3 - 1))]
    cols, truths = [], []
    for name, fl in sorted(EDGE_VARIANTS.items()):
        c = _copy(base)
        for i in edges:
            c[1][i] = 0; c[2][i] = 1; c[4][i] = fl
            c[3][i] = (30 + (i & 63)) if fl & PASS else 7
        match = _truth_of(rng, c, frac=0.1, extra=[(int(c[0][i]), 0, 1) for i in edges])
        edge_pos = {int(c[0][i]) for i in edges}
        other = _truth([k for k in zip(*map(np.ndarray.tolist, _truth_of(rng, c, frac=0.1))) if k[0] not in edge_pos] +
                       [(p, 0, 2) for p in edge_pos])
        for t in (match, other):
            cols.append(_cols(*c)); truths.append(t)
    _run_plain(engine, oracle, cols, truths)


def test_dense_truth_makes_the_middle_tile_oversize(engine, oracle):
    """More truth keys in the middle tile's range than a slice holds: its ascending, live pairs take the round-by-round path,
    the tiles around it (under the cap: asserted on the host) the plain one."""
    rng = np.random.default_rng(3700)
    c = _plain(rng, 3072)
    dense = [(int(c[0][i]), int(c[1][i]), int(c[2][i])) for i in range(1024, 2048) if i % 3] + \
            [(int(c[0][i]) + 1, 0, 1) for i in range(1024, 2048, 2)]
    _run_plain(engine, oracle, [_cols(*c)], [_truth_of(rng, c, extra=dense)], oversize=(1,))


@pytest.mark.parametrize("n_bins", [1, 20, 256])
def test_quals(engine, oracle, n_bins):
    """NaN, negative, -0.0, just under a bin edge, the top bin's edge and far above it; the top bin on 40 consecutive records
    across a pair seam (the ballot-counted path)."""
    rng = np.random.default_rng(3800)
    c = _plain(rng, 1537)
    special = np.array([np.nan, -1.0, -0.0, 19.999, 255.0, 1e9], np.float32)
    at = rng.random(1537) < 0.3
    c[3] = np.where(at, special[rng.integers(0, len(special), 1537)], c[3]).astype(np.float32)
    c[3][492:532] = n_bins + 7
    top = _copy(c); top[3][:] = 1e9
    _run_plain(engine, oracle, [_cols(*_kept(c)), _cols(*_kept(top))], [_truth_of(rng, c)] * 2, n_bins=n_bins)


def test_shuffled_twin_through_the_packed_kernel(engine, oracle):
    """The same records out of order take the sort and k_classify on (key, info) pairs: ROC rows and scalars as the plain run's."""
    rng = np.random.default_rng(3900)
    plain = _plain(rng, 2500)
    planted = _copy(plain)
    planted[0][512] = planted[0][511]
    planted[1][700] = 4
    t = _truth_of(rng, plain)
    cols = [_cols(*plain), _cols(*_kept(planted))]
    shuf = []
    for c in cols:
        o = rng.permutation(len(c[0]))
        shuf.append(tuple(np.ascontiguousarray(a[o]) for a in c))
    assert all(k <= SLICE for c in cols for k in _tile_keys(c, t))
    tid = engine.truth_load(*t)
    try:
        res, _ = engine.classify_batch(cols + shuf, [tid] * 4)
        for a, b, c in zip(res[:2], res[2:], cols):
            check_vcf(oracle, a, c, t, expect_sorted=True)
            assert b["scalars"]["sorted"] == 0
            assert np.array_equal(a["roc"], b["roc"])
            for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "truth_unique", "n_records"):
                assert a["scalars"][k] == b["scalars"][k], k
    finally:
        engine.truth_release(tid)


def test_24_ascending_runs_equal_the_sorted_twin(engine, oracle):
    """The generator's per-contig VCF (24 ascending runs, plain but for the pairs that hold a run's end) against the same records
    in position order, and both against the oracle."""
    from oracle.synth import synth_truth_keys
    L, T, n, tseed, seed = 3072 * 16, 384, 3072, 3, 3000     # (the generator: n | L, and the truth stratum a multiple of the VCF's)
    tid = engine.truth_synth(L, T, tseed)
    truth = synth_truth_keys(L, T, tseed, 0)
    out = {}
    try:
        for runs in (0, 24):
            b = engine.batch([n, n], [tid, tid])
            try:
                b.synth(L, T, tseed, seed, shuffled=runs)
                b.run(); b.finish()
                out[runs] = (b.roc(), b.scalars())
                for v in range(2):
                    cls, roc, sc = oracle.classify_columns(*b.columns(v), *truth)
                    assert np.array_equal(b.cls(v), cls) and np.array_equal(out[runs][0][v], roc)
                    assert [int(x) for x in out[runs][1][v][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
            finally:
                b.close()
    finally:
        engine.truth_release(tid)
    assert np.array_equal(out[0][0], out[24][0]) and np.array_equal(out[0][1][:, :5], out[24][1][:, :5])
    assert out[0][1][:, 5].tolist() == [1, 1] and out[24][1][:, 5].tolist() == [0, 0]
