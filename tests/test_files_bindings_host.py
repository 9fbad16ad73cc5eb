"""Engine._files_<pass>: the entry point each builder returns, every field of the args struct it hands the library (read back
through the byref object: scalars as they are, arrays through their pointers), what unpack(k) gives a wanted row, an unwanted
row and a pure row, and every length and range message, for calls of 0, 1 and 3 jobs.  No device: the builders are called unbound
on a stand-in that has the entry points as names, and the args structs are plain ctypes types."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from quasimodo_amd import _lib
from quasimodo_amd.engine import Engine

ENTRIES = ("motifs", "profile", "truthside", "strata", "context", "normalize", "atomize", "rescue_roc", "types", "haplotypes", "hapsubsets", "boot", "votes",
           "nearmiss", "surface")
STAND = SimpleNamespace(_L=SimpleNamespace(**{"qm_extract_files_" + e: "entry:" + e for e in ENTRIES}), strata_info=lambda sid: {7: (3, 9)}[sid])
U8, I32, I64, U64 = np.uint8, np.int32, np.int64, np.uint64
EDGES = (1, 2, 3, 4, 5, 6, 16, 51)


def at(ptr, dtype, shape):
    """the array a pointer field (an address as int, or a c_void_p) points to"""
    ptr = ptr.value if isinstance(ptr, C.c_void_p) else ptr
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_char * nbytes).from_address(ptr), dtype).reshape(shape)


def want(n):
    return [1, 0, 1][:n]


def gen(n):
    return [5, None, 6][:n]


def paths(n, stem):
    return ["%s%d.tsv" % (stem, k) if k != 1 else None for k in range(n)]


def enc(xs, n):
    """what a c_char_p array of max(n, 1) entries gives back"""
    return [None if x is None else x.encode() for x in xs] + [None] * (1 if n == 0 else 0)


# Per pass, for a call of n jobs (row 0 wanted, row 1 not, row 2 wanted and pure): the spec, the entry point, the struct's scalars,
# its input arrays (field: dtype, values -- one placeholder entry when n is 0), its path arrays, its output arrays (field: dtype, row
# shape, the key unpack serves it under, "job" or "group" rows), the constants unpack adds, and the rows of the three that gain
# (`None`: the keys whose value is None under alleles=True)
def profile(n):
    return dict(spec={"want": want(n), "points": paths(n, "p"), "window": 64, "n_pos_bins": 4, "n_af_bins": 2}, entry="profile", struct=_lib.ProfileArgs,
                scalars=dict(window=64, n_pos_bins=4, n_af_bins=2, reserved=0), ins={"want": (U8, want(n) or [0])}, chars={"points_out": paths(n, "p")},
                outs={"grid": (U64, (2, 2, 4), "af_grid"), "extra": (U64, (2, 3), "af_extra")}, gain=[0, 2])


def profile_defaults(n):
    return dict(spec={"want": want(n)}, entry="profile", struct=_lib.ProfileArgs, scalars=dict(window=1024, n_pos_bins=256, n_af_bins=20, reserved=0),
                ins={"want": (U8, want(n) or [0])}, chars={"points_out": [None] * n}, outs={"grid": (U64, (2, 20, 256), "af_grid"), "extra": (U64, (2, 3), "af_extra")}, gain=[0, 2])


def truthside(n):
    grp = [0, None, 1][:n]
    ng = {0: 0, 1: 1, 3: 2}[n]
    return dict(spec={"fn": paths(n, "fn"), "group": grp, "missed": ["m%d.tsv" % g for g in range(ng)]}, entry="truthside", struct=_lib.TruthSideArgs,
                scalars=dict(n_groups=ng, reserved=0), ins={"group": (I32, [0, -1, 1][:n] or [-1])}, chars={"fn_out": paths(n, "fn"), "missed_out": ["m%d.tsv" % g for g in range(ng)]},
                outs={"regions": (U64, (32,), "truth_regions", "group", I64), "fp_regions": (I64, (32,), "fp_regions", "group")}, gain=[0, 2], groups=ng, group_of=[0, -1, 1])


def truthside_no_missed(n):
    d = truthside(n)
    d["spec"] = {"fn": paths(n, "fn"), "group": d["spec"]["group"]}
    d["chars"]["missed_out"] = [None] * d["groups"]
    return d


def strata(n):
    return dict(spec={"id": 7, "want": want(n)}, entry="strata", struct=_lib.StrataArgs, scalars=dict(strata_id=7, reserved=0), ins={"want": (U8, want(n) or [0])}, chars={},
                outs={"rec": (U64, (5, 3), "strata_rec"), "tru": (U64, (4, 2), "strata_tru")}, gain=[0, 2], none=("strata_tru",))


def context(n):
    return dict(spec={"genomes": gen(n), "half_window": 5, "n_gc": 2}, entry="context", struct=_lib.ContextArgs, scalars=dict(w=5, ng=2), ins={"genome_id": (I32, [5, -1, 6][:n] or [-1])},
                chars={}, outs={"rec": (U64, (34, 3), "context_rec"), "tru": (U64, (33, 2), "context_tru"), "gen": (U64, (33,), "context_gen")}, gain=[0, 2],
                none=("context_tru",), consts={"context_params": (5, 2)})


def context_defaults(n):
    return dict(context(n), spec={"genomes": gen(n)}, scalars=dict(w=50, ng=10), consts={"context_params": (50, 10)},
                outs={"rec": (U64, (162, 3), "context_rec"), "tru": (U64, (161, 2), "context_tru"), "gen": (U64, (161,), "context_gen")})


def normalize(n):
    return dict(spec={"genomes": gen(n), "rescued": paths(n, "r")}, entry="normalize", struct=_lib.NormalizeArgs, scalars={}, ins={"genome_id": (I32, [5, -1, 6][:n] or [-1])},
                chars={"rescued_out": paths(n, "r")}, outs={"rec": (U64, (12,), "norm_rec"), "tru": (U64, (5,), "norm_tru")}, gain=[0])


def atomize(n):
    return dict(spec={"want": want(n), "atoms": paths(n, "a")}, entry="atomize", struct=_lib.AtomizeArgs, scalars={}, ins={"want": (U8, want(n) or [0])},
                chars={"atoms_out": paths(n, "a")}, outs={"rec": (U64, (13,), "atom_rec"), "tru": (U64, (6,), "atom_tru")}, gain=[0, 2])


def rescue_roc(n):
    return dict(spec={"genomes": gen(n), "want": want(n)}, entry="rescue_roc", struct=_lib.RescueRocArgs, scalars={}, n_bins=16,
                ins={"genome_id": (I32, [5, -1, 6][:n] or [-1]), "want": (U8, want(n) or [0])}, chars={},
                outs={"roc_n": (U64, (3, 16), "rroc_n"), "roc_a": (U64, (3, 16), "rroc_a"), "base": (U64, (2,), "rroc_base")}, gain=[0])


def vartype(n):
    return dict(spec={"want": want(n), "edges": (1, 2, 9)}, entry="types", struct=_lib.TypesArgs, scalars=dict(n_bins=3, reserved=0), ins={"want": (U8, want(n) or [0]), "edges": (I32, [1, 2, 9])},
                chars={}, outs={"rec": (U64, (19, 2), "type_rec"), "tru": (U64, (19, 2), "type_tru")}, gain=[0], consts={"type_edges": (1, 2, 9)})


def vartype_defaults(n):
    return dict(vartype(n), spec={"want": want(n)}, scalars=dict(n_bins=8, reserved=0), ins={"want": (U8, want(n) or [0]), "edges": (I32, list(EDGES))},
                outs={"rec": (U64, (44, 2), "type_rec"), "tru": (U64, (44, 2), "type_tru")}, consts={"type_edges": EDGES})


SEQS = [b"ACGT", None, bytearray(b"TTGGCC")]


def haplo(n):
    return dict(spec={"genomes": gen(n), "gap": 4, "sites": paths(n, "s"), "seqs": SEQS[:n]}, entry="haplotypes", struct=_lib.HaplotypesArgs, scalars=dict(gap=4, reserved=0),
                ins={"genome_id": (I32, [5, -1, 6][:n] or [-1]), "genome_len": (I64, [4, 0, 6][:n] or [0])}, chars={"sites_out": paths(n, "s")}, seqs=[b"ACGT", None, b"TTGGCC"][:n],
                outs={"rec": (U64, (16,), "hap_rec"), "tru": (U64, (8,), "hap_tru")}, gain=[0], consts={"hap_gap": 4})


def haplo_defaults(n):
    return dict(haplo(n), spec={"genomes": gen(n)}, scalars=dict(gap=10, reserved=0), ins={"genome_id": (I32, [5, -1, 6][:n] or [-1]), "genome_len": (I64, [0] * max(n, 1))},
                chars={"sites_out": [None] * n}, seqs=[None] * n, consts={"hap_gap": 10})


def hapsub(n):
    d = haplo(n)
    return dict(d, spec=dict(d["spec"], subsets=paths(n, "u")), entry="hapsubsets", struct=_lib.HapsubArgs, chars=dict(d["chars"], subsets_out=paths(n, "u")),
                outs=dict(d["outs"], sub=(U64, (8,), "hap_sub")))


def hapsub_defaults(n):
    d = haplo_defaults(n)
    return dict(d, entry="hapsubsets", struct=_lib.HapsubArgs, chars=dict(d["chars"], subsets_out=[None] * n), outs=dict(d["outs"], sub=(U64, (8,), "hap_sub")))


def boot(n):
    return dict(spec={"want": want(n), "window": 8, "n_win": 4, "n_rep": 3, "seed": -1}, entry="boot", struct=_lib.BootArgs,
                scalars=dict(window=8, n_win=4, n_rep=3, reserved=0, seed=(1 << 64) - 1), ins={"want": (U8, want(n) or [0])}, chars={},
                outs={"cnt": (U64, (6, 4), "boot_cnt"), "rep": (U64, (3, 4), "boot_rep")}, gain=[0, 2])


def boot_no_replicates(n):
    """n_rep 0: the library still gets one row to write to, the row gains none"""
    return dict(boot(n), spec={"want": want(n), "n_rep": 0}, scalars=dict(window=1024, n_win=256, n_rep=0, reserved=0, seed=0),
                outs={"cnt": (U64, (258, 4), "boot_cnt"), "rep": (U64, (1, 4), "boot_rep", "job", U64, 0)})


def votes(n):
    ng = {0: 0, 1: 1, 3: 2}[n]
    return dict(spec={"group": [0, None, 1][:n], "k": [2, 0][:ng], "out": ["c0.vcf", None][:ng]}, entry="votes", struct=_lib.VotesArgs, scalars=dict(n_groups=ng, reserved=0),
                ins={"group": (I32, [0, -1, 1][:n] or [-1]), "consensus_k": (I32, [2, 0][:ng] or [0])}, chars={"consensus_out": ["c0.vcf", None][:ng]},
                outs={"tp_votes": (U64, (33,), "tp_votes", "group"), "fp_votes": (U64, (33,), "fp_votes", "group"), "private_tp": (U64, (32,), "private_tp", "group"),
                      "private_fp": (U64, (32,), "private_fp", "group")}, gain=[0, 2], groups=ng, group_of=[0, -1, 1], consts={"vote_member": 0})


def votes_defaults(n):
    d = votes(n)
    return dict(d, spec={"group": d["spec"]["group"]}, ins=dict(d["ins"], consensus_k=(I32, [0] * max(d["groups"], 1))), chars={"consensus_out": [None] * d["groups"]})


def nearmiss(n):
    return dict(spec={"radius": 3, "want": want(n), "fp_why": paths(n, "fp"), "fn_why": paths(n, "fn")}, entry="nearmiss", struct=_lib.NearmissArgs, scalars=dict(radius=3, reserved=0),
                ins={"want": (U8, want(n) or [0])}, chars={"fp_why_out": paths(n, "fp"), "fn_why_out": paths(n, "fn")},
                outs={"rec": (U64, (6,), "nearmiss_rec", "job", list), "tru": (U64, (5,), "nearmiss_tru", "job", list)}, gain=[0], consts={"nearmiss_radius": 3})


def nearmiss_no_files(n):
    return dict(nearmiss(n), spec={"radius": 0, "want": want(n)}, scalars=dict(radius=0, reserved=0), chars={"fp_why_out": [None] * n, "fn_why_out": [None] * n},
                consts={"nearmiss_radius": 0})


def surface(n):
    return dict(spec={"want": want(n), "q_step": 2, "nq": 3, "na": 5}, entry="surface", struct=_lib.SurfaceArgs, scalars=dict(q_step=2, nq=3, na=5, reserved=0), ins={"want": (U8, want(n) or [0])},
                chars={}, outs={"S": (U64, (3, 3, 5), "surface"), "extra": (U64, (4,), "surface_extra", "job", list)}, gain=[0, 2], consts={"surface_params": (2, 3, 5)})


def surface_defaults(n):
    return dict(surface(n), spec={"want": want(n)}, scalars=dict(q_step=4, nq=64, na=50, reserved=0), outs={"S": (U64, (3, 64, 50), "surface"), "extra": (U64, (4,), "surface_extra", "job", list)},
                consts={"surface_params": (4, 64, 50)})


BUILDERS = {"profile": (profile, profile_defaults), "truthside": (truthside, truthside_no_missed), "strata": (strata,), "context": (context, context_defaults), "normalize": (normalize,),
            "atomize": (atomize,), "rescue_roc": (rescue_roc,), "vartype": (vartype, vartype_defaults), "haplo": (haplo, haplo_defaults), "hapsub": (hapsub, hapsub_defaults),
            "boot": (boot, boot_no_replicates), "votes": (votes, votes_defaults), "nearmiss": (nearmiss, nearmiss_no_files), "surface": (surface, surface_defaults)}
CALLS = [(name, f, n, alleles) for name, fs in BUILDERS.items() for f in fs for n in (0, 1, 3) for alleles in ((False, True) if f(0).get("none") else (False,))]


@pytest.mark.parametrize("name,case,n,alleles", CALLS, ids=["%s-%d%s" % (f.__name__, n, "-alleles" if a else "") for _, f, n, a in CALLS])
def test_struct_and_rows(name, case, n, alleles):
    d = case(n)
    file_jobs = [{"pure": k == 2} for k in range(n)]
    entry, extra, unpack = getattr(Engine, "_files_" + name)(STAND, n, d["spec"], gids=None, alleles=alleles, file_jobs=file_jobs, n_bins=d.get("n_bins", 256))
    assert entry == "entry:" + d["entry"]
    if name == "profile":
        assert extra[:2] == (None, None)
        extra = extra[2:]
    assert len(extra) == 1
    s = extra[0]._obj
    assert type(s) is d["struct"]
    fields = {f for f, _ in s._fields_}
    assert fields == set(d["scalars"]) | set(d["ins"]) | set(d["chars"]) | set(d["outs"]) | ({"genome_seq"} if "seqs" in d else set())
    for f, v in d["scalars"].items():
        assert getattr(s, f) == v, f
    for f, (dt, v) in d["ins"].items():
        assert at(getattr(s, f), dt, (len(v),)).tolist() == v, f
    for f, v in d["chars"].items():
        assert [getattr(s, f)[k] for k in range(max(len(v), 1))] == enc(v, len(v)), f
    if "seqs" in d:
        assert [s.genome_seq[k] for k in range(max(n, 1))] == d["seqs"] + [None] * (n == 0)
    rows = max(d.get("groups", n), 1)
    filled = {}
    for f, out in d["outs"].items():
        a = at(getattr(s, f), out[0], (rows,) + out[1])
        assert not a.any(), f
        a[...] = (np.arange(a.size) % 251 + 1).reshape(a.shape)          # (as the library would: unpack reads these very arrays)
        filled[f] = a.copy()
    for k in range(n):
        r = unpack(k)
        if k not in d["gain"]:
            assert r == {}
            continue
        g = d["group_of"][k] if "groups" in d else k
        consts = dict(d.get("consts", {}))
        assert set(r) == {out[2] for out in d["outs"].values()} | set(consts)
        for key, v in consts.items():
            assert r[key] == v and type(r[key]) is type(v)
        for f, out in d["outs"].items():
            key, kind = out[2], out[4] if len(out) > 4 else out[0]
            if alleles and key in d.get("none", ()):
                assert r[key] is None
            elif kind is list:
                assert r[key] == [int(x) for x in filled[f][g]] and all(type(x) is int for x in r[key])
            else:
                exp = filled[f][g][:out[5]] if len(out) > 5 else filled[f][g]
                assert r[key].dtype == kind and r[key].shape == exp.shape and np.array_equal(r[key], exp.astype(kind))
                r[key][...] = 0                                              # a copy: the row does not alias the call's array
                assert np.array_equal(at(getattr(s, f), out[0], (rows,) + out[1]), filled[f])


def test_vote_member_counts_the_earlier_members():
    _, _, unpack = Engine._files_votes(STAND, 4, {"group": [1, 0, 1, 1]})
    assert [unpack(k)["vote_member"] for k in range(4)] == [0, 0, 1, 2]


@pytest.mark.parametrize("n", [1, 3])
def test_motifs_alone_and_beside_the_profile(n):
    gids = np.array([5, -1, 6][:n], np.int32)
    entry, extra, unpack = Engine._files_motifs(STAND, n, gids, gids=gids, alleles=False, file_jobs=[{}] * n, n_bins=256)
    assert entry == "entry:motifs" and extra[0].value == gids.ctypes.data
    m = at(extra[1], U64, (n, 3, 98))
    assert not m.any()
    m[...] = np.arange(m.size).reshape(m.shape)
    for k in range(n):
        r = unpack(k)
        assert set(r) == {"motifs"} and r["motifs"].dtype == U64 and np.array_equal(r["motifs"], m[k])
    entry, extra, unpack = Engine._files_profile(STAND, n, {"want": want(n)}, gids=gids, alleles=False, file_jobs=[{}] * n, n_bins=256)
    assert entry == "entry:profile" and extra[0].value == gids.ctypes.data and type(extra[2]._obj) is _lib.ProfileArgs
    m = at(extra[1], U64, (n, 3, 98))
    m[...] = np.arange(m.size).reshape(m.shape)
    for k in range(n):
        r = unpack(k)
        assert set(r) == ({"motifs", "af_grid", "af_extra"} if want(n)[k] else {"motifs"}) and np.array_equal(r["motifs"], m[k])


MESSAGES = [
    ("profile", 3, {"want": [1], "points": [None, None]}, "profile: 1 want / 2 points entries for 3 jobs"),
    ("profile", 0, {"want": [], "points": [None]}, "profile: 0 want / 1 points entries for 0 jobs"),
    ("profile", 1, {"want": [1], "n_af_bins": 0}, "profile: 0 x 256 bins (at most 8192 cells)"),
    ("profile", 1, {"want": [1], "n_af_bins": 33}, "profile: 33 x 256 bins (at most 8192 cells)"),
    ("truthside", 3, {"fn": [None], "group": [0, 0]}, "truthside: 1 fn / 2 group entries for 3 jobs"),
    ("truthside", 0, {"fn": [None], "group": []}, "truthside: 1 fn / 1 group entries for 0 jobs"),
    ("strata", 3, {"id": 7, "want": [1]}, "strata: 1 want entries for 3 jobs"),
    ("context", 3, {"genomes": [1, 2]}, "context: 2 genomes entries for 3 jobs"),
    ("context", 1, {"genomes": [1], "n_gc": 0}, "context: 0 GC bins (1 to 15)"),
    ("normalize", 3, {"genomes": [1], "rescued": [None, None]}, "normalize: 1 genomes / 2 rescued entries for 3 jobs"),
    ("normalize", 3, {"genomes": [1]}, "normalize: 1 genomes / 3 rescued entries for 3 jobs"),
    ("atomize", 3, {"want": [1], "atoms": [None, None]}, "atomize: 1 want / 2 atoms entries for 3 jobs"),
    ("atomize", 0, {"want": [], "atoms": [None]}, "atomize: 0 want / 1 atoms entries for 0 jobs"),
    ("rescue_roc", 3, {"genomes": [1, 2, 3], "want": [1]}, "rescue_roc: 3 genomes / 1 want entries for 3 jobs"),
    ("rescue_roc", 3, {"genomes": [1, 2], "want": [1, 0, 0]}, "rescue_roc: 2 genomes / 3 want entries for 3 jobs"),
    ("vartype", 3, {"want": [1, 1]}, "vartype: 2 want entries for 3 jobs"),
    ("vartype", 1, {"want": [1], "edges": (2, 3)}, "vartype: the first size edge is 2 (it must be 1: every variant has a size of at least 1)"),
    ("haplo", 3, {"genomes": [1], "sites": [None] * 2, "seqs": [None] * 4}, "haplo: 1 genomes / 2 sites / 4 seqs entries for 3 jobs"),
    ("haplo", 1, {"genomes": [1], "gap": 33}, "haplo: the gap is an integer from 0 to 32, not 33"),
    ("hapsub", 3, {"genomes": [1], "sites": [None] * 2, "seqs": [None] * 4, "subsets": [None] * 5}, "hapsub: 1 genomes / 2 sites / 4 seqs / 5 subsets entries for 3 jobs"),
    ("hapsub", 3, {"genomes": [1, 2, 3], "subsets": [None]}, "hapsub: 3 genomes / 3 sites / 3 seqs / 1 subsets entries for 3 jobs"),
    ("hapsub", 1, {"genomes": [1], "gap": True}, "haplo: the gap is an integer from 0 to 32, not True"),
    ("boot", 3, {"want": [1]}, "boot: 1 want entries for 3 jobs"),
    ("boot", 1, {"want": [1], "window": 0}, "boot: window 0, n_win 256 (1 to 4096), n_rep 1000 (0 to 16384)"),
    ("boot", 1, {"want": [1], "n_win": 4097}, "boot: window 1024, n_win 4097 (1 to 4096), n_rep 1000 (0 to 16384)"),
    ("boot", 1, {"want": [1], "n_rep": -1}, "boot: window 1024, n_win 256 (1 to 4096), n_rep -1 (0 to 16384)"),
    ("votes", 3, {"group": [0]}, "votes: 1 group entries for 3 jobs"),
    ("votes", 3, {"group": [0, 1, 1], "k": [1], "out": [None] * 3}, "votes: 1 levels / 3 files for 2 groups"),
    ("nearmiss", 3, {"radius": 1, "want": [1], "fp_why": [None] * 2}, "nearmiss: 1 want / 2 fp_why / 3 fn_why entries for 3 jobs"),
    ("nearmiss", 1, {"radius": 65, "want": [1]}, "nearmiss: radius 65 (0 to 64)"),
    ("surface", 3, {"want": [1, 0]}, "surface: 2 want entries for 3 jobs"),
    ("surface", 1, {"want": [1], "nq": 0}, "surface: nq 0 (1 to 256)"),
]


@pytest.mark.parametrize("name,n,spec,message", MESSAGES, ids=["%s-%d" % (m[0], k) for k, m in enumerate(MESSAGES)])
def test_messages(name, n, spec, message):
    with pytest.raises(ValueError) as ei:
        getattr(Engine, "_files_" + name)(STAND, n, spec, gids=None, alleles=False, file_jobs=[{}] * n, n_bins=256)
    assert str(ei.value) == message
