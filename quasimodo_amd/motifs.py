"""Mutation-context (96-motif) spectra: the host side of the reference's rule mutationcontext (rules/mutationcontext.smk,
scripts/mutation_context_profile.R).  The counts come from the engine (qm_batch_motifs); this module names the
columns, reads the genome FASTA and writes the table.  The plot the R script draws is out of scope."""
import os

BASES = "ACGT"
SUBSTITUTIONS = ("CA", "CG", "CT", "TA", "TC", "TG")
# SomaticSignatures' motif spelling "<ref><alt> <l>.<r>", in the order of the engine's columns 0..95 (= lexicographic)
MOTIFS = tuple("%s %s.%s" % (s, l, r) for s in SUBSTITUTIONS for l in BASES for r in BASES)
N_MOTIFS = 96
MOTIF_OTHER = 96           # include/qmvt.h QM_MOTIF_OTHER
MOTIF_REF_MISMATCH = 97    # include/qmvt.h QM_MOTIF_REF_MISMATCH
MOTIF_COLS = 98


def alteration(motif):
    """'CA A.C' -> 'C>A'"""
    return "%s>%s" % (motif[0], motif[1])


def context(motif):
    """'CA A.C' -> 'A.C'"""
    return motif[3:]


def read_fasta(path, contig=None):
    """The bytes of one sequence of a FASTA file (no header, no line breaks; '\\r' of Windows line endings dropped).  contig:
    the name (first word of the header) to take; without it the file must hold exactly one sequence."""
    with open(path, "rb") as fh:
        data = fh.read()
    seqs, name, cur = [], None, None
    for ln in data.split(b"\n"):
        ln = ln.rstrip(b"\r")
        if ln.startswith(b">"):
            name = ln[1:].split(None, 1)[0].decode("utf-8", "replace") if ln[1:].split() else ""
            cur = []
            seqs.append((name, cur))
        elif ln and cur is not None:
            cur.append(ln.strip())
        elif ln.strip():
            raise ValueError("%s: sequence data before the first '>' header" % path)
    if not seqs:
        raise ValueError("%s holds no FASTA sequence" % path)
    if contig is None:
        if len(seqs) > 1:
            raise ValueError("%s holds %d sequences (%s); name one with contig=" % (path, len(seqs), ", ".join(n for n, _ in seqs[:5])))
        return b"".join(seqs[0][1])
    for n, parts in seqs:
        if n == contig:
            return b"".join(parts)
    raise ValueError("%s holds no sequence named %r" % (path, contig))


def write_mutation_context(path, columns):
    """results/final_tables/{mix}.{caller}.mutationcontext.tsv: header `motif alteration context <study>...`, one row per motif
    in MOTIFS order, integer counts.  columns: list of (study name, 96 counts).  Written atomically."""
    columns = list(columns)
    for name, counts in columns:
        if len(counts) < N_MOTIFS:
            raise ValueError("column %r has %d counts, need %d" % (name, len(counts), N_MOTIFS))
    lines = ["\t".join(["motif", "alteration", "context"] + [n for n, _ in columns])]
    for k, m in enumerate(MOTIFS):
        lines.append("\t".join([m, alteration(m), context(m)] + [str(int(c[k])) for _, c in columns]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def study_columns(sample_rows):
    """The columns of one mix's table as the R script names them: samples in sorted order, `-1-0` left out; the kept row as
    `<sample>` (`unmixed <sample>` for `-0-1`), then `<sample> (TP)` and `<sample> (FP)` for mixed samples.
    sample_rows: {sample: [3][>= 96] counts (kept, TP, FP)}."""
    cols = []
    for s in sorted(sample_rows):
        if s.endswith("-1-0"):
            continue
        rows = sample_rows[s]
        if s.endswith("-0-1"):
            cols.append(("unmixed " + s, rows[0][:N_MOTIFS]))
        else:
            cols.append((s, rows[0][:N_MOTIFS]))
            cols.append((s + " (TP)", rows[1][:N_MOTIFS]))
            cols.append((s + " (FP)", rows[2][:N_MOTIFS]))
    return cols
