"""The inputs of the tests of `-g` (abg_output_graph_seqs), `-C` / `-R` (abg_contains_seq) and abg_reset, shared by the CPU
tests (tests/test_graph_hostcheck.py: the device logic run serially through tests/hostcheck), the GPU tests
(tests/test_gpu_graph.py: the real kernels) and the generator of the reference's digests
(tests/golden/make_graph_golden.py).  TEST INFRASTRUCTURE.

Pure Python and numpy: neither tests/hostcheck nor the HIP library is loaded by importing this module."""
import functools
import hashlib
import json
import os

import numpy as np

from abyss_amd import api, synth
from util import GOLDEN, GoldenCase, mask_of

# ---- graph shapes: golden read sets whose assembly is pinned, now dumped as graphs too (cycles, tandem repeats, hairpins,
# homopolymer runs, k = 12 / 96 / 192; s_satellite_k40 has 36,180 vertices: one rehash of the vertex table)
SHAPES = ["s_plasmids_k32", "s_tandem_k32", "s_tandem_k64_t20", "s_inverted_k40", "s_lowcomplex_k25", "s_plasmids_k48_K16",
          "s_mixed_k192", "s_mixed_k12", "s_mixed_k32_H1", "s_mixed_k40_H6", "s_mixed_k32_H12_kc3", "s_satellite_k40", "k96",
          "k50_qr11"]

# ---- template widths: the device code is built per number of 64-bit words of a k-mer (1, 2, 3, 4, 6) and again for a
# spaced seed.  (k, K, read set); K None = no spaced seed.  NW 4, NW 6, masked 1, 3, 4, 6, 4 (twice)
WIDTHS = [(128, None, 0), (160, None, 0), (24, 8, 0), (96, 32, 0), (128, 40, 0), (192, 64, 0), (100, 40, 0), (100, 40, 1)]
WIDTH_N_RATE = 0.002
# ---- the sweep against the oracle (no digests): twice the N rate, two read sets each
SWEEP = [(24, 8), (33, 11), (40, 12), (48, 16), (64, 20), (64, 32), (128, 64), (100, 32), (100, 40), (128, 32), (128, 40), (160, 40)]
SWEEP_N_RATE = 0.004
SEEDED_COUNTERS_OPT = "-b2M"

# ---- growth: the smallest shape found that crosses the node buffer's first size (65,532 vertices) once and the vertex
# table's first two (32,768 and 65,536 entries).  (-b9M: the reference makes 2^23 counters of it)
GROWTH = dict(k=40, genome=80000, coverage=20.0, err=0.002, genome_seed=5, read_seed=6, opt="-b9M")
GROWTH_MIN_NODES = 70000
NODE_CAP0, TAB_LIMIT0 = 1 << 16, 1 << 15

# ---- coverage track
COV_READS = "k40_mixed"
COV_LONG = 2 * (1 << 20) + 12345
PIECE = 1 << 20  # abg_contains_seq cuts a run of k-mers into pieces of this many bases, overlapping by k - 1


def width_name(k, K, s):
    return "w_k%d%s%s" % (k, "_K%d" % K if K else "", "_b" if s else "")


def seeded_reads(k, s=0, n_rate=WIDTH_N_RATE):
    """Read set `s` of width k: 250-base pairs off a 20 kb genome at 25x, both mates one after the other, 'N' written at rate
    n_rate into two rows of three.  Returns (buf, off, generator arguments)."""
    seed = k + 1000 * s
    args = dict(genome=20000, coverage=25.0, read_len=250, err=0.004, genome_seed=seed, read_seed=seed + 1, n_seed=seed,
                n_rate=n_rate)
    m1, m2 = synth.make_read_set(args["genome"], args["coverage"], read_len=args["read_len"], err=args["err"],
                                 genome_seed=args["genome_seed"], read_seed=args["read_seed"])
    asc = synth.codes_to_ascii(np.concatenate([m1, m2])).copy()
    hit = np.random.default_rng(args["n_seed"]).random(asc.shape) < n_rate
    hit[::3] = False
    asc[hit] = ord("N")
    buf, off = api.matrix_to_seqs(asc)
    return buf, off, args


def growth_reads():
    g = GROWTH
    m1, m2 = synth.make_read_set(g["genome"], g["coverage"], err=g["err"], genome_seed=g["genome_seed"], read_seed=g["read_seed"])
    return api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))


def growth_cuts(n):
    return [0, n // 5, n // 5 + 1, n // 2, n]


def seed_of(k, K):
    return api.spaced_seed_kmer_pair(k, K) if K else None


def cov_records(k, text, seed=40, clean=False, plant_ns=False):
    """The three records of the coverage-track reference: one of 2 * 2^20 + 12,345 random bases with 6,000 characters of
    `text` planted at 2^20 - 3000 and at 2^21 - 3000 - (k - 1), 'NNN' at 500,000 and an 'n' at 2^20 + 7; a lower-case one of
    70 kb; one shorter than k.  abg_contains_seq cuts every RUN of valid k-mers into pieces, so the 'n' moves the seams: this
    record has one, at 2^21 + 8, inside the second planted stretch.  clean: without the 'NNN' and the 'n' -- one run, seams at
    2^20 and 2^21 - (k - 1), one in each planted stretch.  plant_ns (for a spaced seed, with clean): 'N' in the planted text
    behind the first seam, two of them 16 apart, which leaves a second seam in the second stretch (see cov_seams)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    long_ = acgt[rng.integers(0, 4, size=COV_LONG)].copy()
    plant = np.frombuffer(text[:12000], dtype=np.uint8).copy()
    assert len(plant) == 12000 and np.isin(plant, acgt).all()
    if plant_ns:
        plant[[3500, 4000, 4016, 5457, 6000 + 5800]] = ord("N")
    for j, at in enumerate((PIECE - 3000, 2 * PIECE - 3000 - (k - 1))):
        long_[at:at + 6000] = plant[6000 * j:6000 * (j + 1)]
    if not clean:
        long_[500000:500003] = ord("N")
        long_[PIECE + 7] = ord("n")
    low = acgt[rng.integers(0, 4, size=70000)].copy()
    low[20000:26000] = plant[3000:9000]
    return [(b"long one", long_.tobytes()), (b"low", low.tobytes().lower()), (b"tiny", b"ACGTACGTAC")]


def cov_text(name):
    """The text of a golden read set's reads that are upper-case ACGT throughout, one after the other."""
    g = GoldenCase(name)
    return b"".join(r for r in g.reads if not r.strip(b"ACGT"))


def cov_seams(k, pos):
    """Start positions of the first k-mer of every piece but a run's first, from the positions of a sequence's valid k-mers:
    a run of k-mers starting at a is the text [a, ...), cut every 2^20 bases with k - 1 bases of overlap."""
    pos = np.asarray(pos, dtype=np.int64)
    brk = np.flatnonzero(np.diff(pos) != 1) + 1
    out = []
    for a, b in zip(np.concatenate([[0], brk]), np.concatenate([brk, [len(pos)]])):
        first, last = int(pos[a]), int(pos[b - 1])
        q = first + PIECE - (k - 1)
        while q <= last:
            out.append(q)
            q += PIECE - (k - 1)
    return out


def cov_fasta(records):
    return b"".join(b">" + name + b"\n" + seq + b"\n" for name, seq in records)


def reads_fasta(buf, off):
    return b"".join(b">r%d\n%s\n" % (i, buf[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1))


@functools.lru_cache(None)
def golden():
    return json.load(open(os.path.join(GOLDEN, "graph_golden.json")))


def check_digest(name, text, nodes, edges):
    """`text` with its frame, and the visitor's counters, against what the unmodified reference wrote."""
    ref = golden()[name]
    assert (len(text), nodes, edges) == (ref["bytes"], ref["nodes"], ref["edges"]), (name, len(text), nodes, edges, ref)
    assert hashlib.sha256(text).hexdigest() == ref["sha256"], name


def same_dump(got, want):
    """(text, nodes, edges) twice; the first difference in the message, not 10 MB of text."""
    if got == want:
        return True
    a, b = got[0], want[0]
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    line = a.count(b"\n", 0, n)
    raise AssertionError("dumps differ: %d / %d bytes, counters %s / %s, first at line %d: %r / %r" % (
        len(a), len(b), got[1:], want[1:], line, a[a.rfind(b"\n", 0, n) + 1:n + 60], b[b.rfind(b"\n", 0, n) + 1:n + 60]))


def vertex_reads(text):
    """Every vertex of a dump as a read of its own (the lines "\\tKMER;\\n").  A vertex and its reverse complement are one
    vertex, so a further dump over these reads finds both of each read's start vertices seen and writes nothing -- unless
    the table of seen vertices has lost one."""
    return api.concat_seqs([ln[1:-1] for ln in text.split(b"\n") if ln.endswith(b";") and b" " not in ln])


def shape_case(name):
    """(buf, off, engine arguments) of a golden read set."""
    g = GoldenCase(name)
    kw = g.kwargs()
    return g.buf, g.off, dict(k=kw["k"], counters=g.meta["counters"], num_hashes=kw["num_hashes"], min_cov=kw["min_cov"],
                              trim=kw["trim"], mask=mask_of(g))


def width_case(k, K, s):
    buf, off, _ = seeded_reads(k, s)
    return buf, off, dict(k=k, counters=golden()[width_name(k, K, s)]["counters"], num_hashes=4, min_cov=2, trim=None,
                          mask=seed_of(k, K))


def sweep_case(k, K, s):
    buf, off, _ = seeded_reads(k, s, SWEEP_N_RATE)
    return buf, off, dict(k=k, counters=golden()[width_name(128, None, 0)]["counters"], num_hashes=4, min_cov=2, trim=None,
                          mask=seed_of(k, K))


def growth_case():
    buf, off = growth_reads()
    return buf, off, dict(k=GROWTH["k"], counters=golden()["growth_k40"]["counters"], num_hashes=4, min_cov=2, trim=None, mask=None)


def components_case(parts=6):
    """`parts` read sets off different genomes, one filter: every call of a chunked dump finds a new component, each smaller
    than the vertex table's first limit, together more than its first two -- the table grows in a LATER call, by the count
    of entries carried over from the earlier ones.  -> ([(buf, off)], (buf, off) of all, engine arguments)"""
    sets = [seeded_reads(40, s)[:2] for s in range(parts)]
    buf = b"".join(b for b, _ in sets)
    offs, base = [np.zeros(1, dtype=np.uint64)], 0
    for b, o in sets:
        offs.append(o[1:] + np.uint64(base))
        base += len(b)
    return sets, (buf, np.concatenate(offs)), dict(k=40, counters=1 << 23, num_hashes=4, min_cov=2, trim=None, mask=None)


def make_oracle(kw, buf, off):
    import oracle_binding as ob
    o = ob.Oracle(kw["k"], counters=kw["counters"], num_hashes=kw["num_hashes"], min_cov=kw["min_cov"], trim=kw["trim"],
                  mask=kw["mask"].encode() if kw["mask"] else None)
    o.load(buf, off)
    return o

