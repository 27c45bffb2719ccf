"""The inputs of the partitioned run's test cases, shared by the CPU workers (tests/dist_worker.py: the device logic run
serially through tests/hostcheck) and the GPU workers (tests/dist_gpu_worker.py: the real kernels): the same bytes, the
same knobs, the same comparison with the oracle or a golden reference run.  TEST INFRASTRUCTURE.

A case is described by a `Case` (what the engine is made with) and run by `run(name, arg, make, rank, world)`, where
`make(case)` returns an engine of the caller's kind with a communicator attached.  An engine offers (HostCheck's and
api.BloomDBG's names): load, load_chunks, keep_reads, assemble, assemble_kept -> (results, contigs), share -> (words,
offsets, lengths, total) from host arrays, load_packed, assemble_packed, counters, import_counters, visited,
counting_stats, assembly_counters, stats, comm (with .calls), close.

Pure Python and numpy: neither tests/hostcheck nor the HIP library is loaded by importing this module (the oracle's
binding is imported when a case runs)."""
import numpy as np

from abyss_amd import api, synth

# (the walkers' own work counters are per rank: each rank walks its share of the candidates)
PER_RANK_STATS = ("bulk_calls", "bulk_steps", "lin_steps", "chain_steps", "memo_hits", "memo_adds", "cls_covered_reads", "archive_bases")
ORACLE_KEYS = ("counting_filter", "results", "contigs", "visited", "assembly_counters")
GOLDEN_KEYS = ("filtered_popcount", "fasta", "readlog", "trace", "counters")


class Case:
    """What an engine of this case is made with.  insert_batch / claim_log2: abg_params.insert_batch_kmers / claim_log2;
    p2_first: PASS 2's first batch in reads (Config::p2_first_batch; 0: the engine's own)."""

    def __init__(self, k, counters, insert_batch, claim_log2, p2_first=0, num_hashes=4, min_cov=2, trim=None, mask=None):
        self.k, self.counters, self.insert_batch, self.claim_log2, self.p2_first = k, counters, insert_batch, claim_log2, p2_first
        self.num_hashes, self.min_cov, self.trim, self.mask = num_hashes, min_cov, trim, mask


def pack(codes):
    """[n, L] base codes 0..3 -> (words, woff, len) in the packed layout of include/abyss_amd.h."""
    n, L = codes.shape
    wpr = (L + 15) // 16
    pad = np.zeros((n, wpr * 16), dtype=np.uint64)
    pad[:, :L] = codes
    words = (pad.reshape(n, wpr, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint32)
    return np.ascontiguousarray(words.reshape(-1)), np.arange(n + 1, dtype=np.uint64) * np.uint64(wpr), np.full(n, L, dtype=np.uint32)


# name -> (k, genome length, counters, coverage, error rate, insert_batch, p2_first, gathered read shares)
SYNTHETIC = {
    "oracle": (33, 12000, 1 << 20, 25.0, 0.005, 20000, 64, False),
    # every read in ONE batch of PASS 2: the commit has to order thousands of candidates whose
    # contigs overlap, over several passes of its fixed point (the ranks combine their bits' verdicts)
    "bigbatch": (31, 20000, 1 << 21, 30.0, 0.01, 20000, 1 << 20, False),
    # a filter so small that counters saturate and every op conflicts with many others: long
    # reservation chains, several rounds per batch, the distributed hand-over to the drain kernel
    "tiny_filter": (25, 6000, 1 << 13, 40.0, 0.02, 5000, 64, False),
    # each rank holds a slice of the packed reads (one of them none at all) and the ranks all-gather them
    "shared": (41, 10000, 1 << 19, 25.0, 0.01, 15000, 64, True),
    # B beyond one device (ABG_SLICE_FILTER=1, set by the test): every rank holds its own range of the counters and nothing
    # else -- under tests/hostcheck the rest of the array is address space without memory, so a stray access kills the rank --
    # PASS 2 probes the gathered bit plane, coverage comes through an all-reduce
    "sliced": (41, 10000, 1 << 19, 25.0, 0.01, 15000, 64, False),
}

# PASS 1 only: (k, counters, insert_batch, claim_log2, reads)
PASS1 = {
    # 300 copies of one read saturate counters at 255 (CountingBloomFilter.hpp:146-149),
    # homopolymers give runs of identical k-mers; batches of 1000 ops
    "saturate": (21, 4096, 1000, 8, [b"ACGTTGCATGCCGATAGCTAGGATCCATGCAAATTTGGCC"] * 300 + [b"A" * 60, b"T" * 60, b"ACAC" * 20]),
    # the same through the ranks' tiles: one k-mer hundreds of times in a batch, counters driven to 255
    "saturate_tiled": (40, 1 << 22, 30000, 16,
                       [b"ACGTTGCATGCCGATAGCTAGGATCCATGCAAGCTTGGCATTCGGATACCGGTAAGCTAGCTAACGGT"] * 400 + [b"A" * 150] * 12 + [b"AC" * 75] * 8),
}

NAMES = tuple(SYNTHETIC) + tuple(PASS1) + ("kept", "sliced_checkpoint", "golden")


def keys_of(name):
    """The verdicts of a case: every one of them must be true."""
    if name == "golden":
        return GOLDEN_KEYS
    if name in PASS1:
        return ("counting_filter",)
    return ORACLE_KEYS


def synthetic_reads(k, G, cov, err):
    m1, m2 = synth.make_read_set(G, cov, err=err, genome_seed=k, read_seed=k + 3)
    codes = np.concatenate([m1, m2])
    buf, off = api.matrix_to_seqs(synth.codes_to_ascii(codes))
    return codes, buf, off


def _against_oracle(case, buf, off, cnt, results, contigs, eng):
    import oracle_binding as ob
    from util import contig_tuple
    o = ob.Oracle(case.k, counters=case.counters)
    o.load(buf, off)
    ro, co = o.assemble(buf, off)
    return {
        "counting_filter": bool(np.array_equal(o.counters(), cnt)),
        "results": bool(np.array_equal(ro, results)),
        "contigs": [contig_tuple(c) for c in co] == [contig_tuple(c) for c in contigs],
        "visited": bool(np.array_equal(o.visited(), eng.visited())),
        "assembly_counters": o.assembly_counters() == eng.assembly_counters(),
        "n_contigs": len(co),
    }


def run_golden(name, make, rank, world):
    from util import GoldenCase, mask_of
    g = GoldenCase(name)
    kw = g.kwargs()
    case = Case(kw["k"], g.meta["counters"], 50000, 16, p2_first=128, num_hashes=kw["num_hashes"], min_cov=kw["min_cov"], trim=kw["trim"],
                mask=mask_of(g))
    eng = make(case)
    eng.load(g.buf, g.off)
    pass1 = dict(eng.comm.calls)  # what PASS 1 sent through the communicator (buffer sizes handed to the collectives)
    fp = eng.counting_stats()[1]
    results, contigs = eng.assemble(g.buf, g.off)
    c = eng.assembly_counters()
    ok = {
        "comm_pass1": pass1, "kmer_ops": int(sum(max(0, len(r) - kw["k"] + 1) for r in g.reads)),
        "filtered_popcount": fp == g.meta["filtered_popcount"],
        "fasta": api.format_fasta(contigs, g.ids) == g.fasta,
        "readlog": api.format_read_log(results, g.ids) == g.readlog,
        "trace": api.format_trace(contigs, g.ids, g.reads, g.opts["k"], with_length=False) == g.trace,
        "counters": (c["reads_processed"], c["solid_reads"], c["visited_reads"]) == (g.meta["reads"], g.meta["solid_reads"], g.meta["visited_reads"]),
    }
    return ok, eng, case


def run_synthetic(name, shared, make, rank, world):
    """Synthetic reads against the oracle.  shared: each rank holds a slice of the packed reads and
    the ranks all-gather them (abg_share_reads) instead of every rank passing the whole set."""
    k, G, counters, cov, err, insert_batch, p2_first, _ = SYNTHETIC[name]
    case = Case(k, counters, insert_batch, 12, p2_first=p2_first)
    codes, buf, off = synthetic_reads(k, G, cov, err)
    eng = make(case)
    if shared:
        n = codes.shape[0]
        a, b = n * rank // world, n * (rank + 1) // world
        if rank == world - 1 and world > 2:
            a = b  # a rank without reads of its own
        elif rank == world - 2 and world > 2:
            b = n
        gw, go, gl, nt = eng.share(*pack(codes[a:b]))
        assert nt == n
        eng.load_packed(gw, go, gl, nt)
        cnt = eng.counters()
        rh, ch = eng.assemble_packed(gw, go, gl, nt)
    else:
        eng.load(buf, off)
        cnt = eng.counters()
        rh, ch = eng.assemble(buf, off)
    ok = _against_oracle(case, buf, off, cnt, rh, ch, eng)
    ok["saturated"] = int(cnt.max())
    return ok, eng, case


def run_pass1(name, make, rank, world):
    import oracle_binding as ob
    k, counters, insert_batch, claim_log2, reads = PASS1[name]
    case = Case(k, counters, insert_batch, claim_log2)
    buf, off = api.concat_seqs(reads)
    o = ob.Oracle(k, counters=counters)
    eng = make(case)
    o.load(buf, off)
    eng.load(buf, off)
    a, b = o.counters(), eng.counters()
    return {"counting_filter": bool(np.array_equal(a, b)), "saturated": int(b.max())}, eng, case


def run_kept(make, rank, world):
    """Reads kept in every rank's store between the passes (abg_keep_reads / abg_load_seqs_v /
    abg_assemble_kept) in a partitioned run: every rank loads every read (several buffers, two calls,
    reads with N and short ones among them) and assembles from its store."""
    k = 37
    case = Case(k, 1 << 20, 15000, 12, p2_first=64)
    m1, m2 = synth.make_read_set(11000, 25.0, err=0.005, genome_seed=k, read_seed=k + 3)
    reads = [bytes(r) for r in synth.codes_to_ascii(np.concatenate([m1, m2]))]
    reads[5] = reads[5][:40] + b"N" + reads[5][41:]
    reads[77] = reads[77][:20]
    reads[300] = reads[300].lower()
    buf, off = api.concat_seqs(reads)
    cuts = [0, 1, 400, 401, 1500, len(reads)]
    chunks = [api.concat_seqs(reads[a:b]) for a, b in zip(cuts, cuts[1:])]
    eng = make(case)
    eng.keep_reads(True, len(buf))
    eng.load_chunks(chunks[:3])
    eng.load_chunks(chunks[3:])
    cnt = eng.counters()
    rh, ch = eng.assemble_kept(len(reads))
    return _against_oracle(case, buf, off, cnt, rh, ch, eng), eng, case


def run_sliced_checkpoint(make, rank, world):
    """A sliced filter written out rank by rank (abg_counters_export) and read back into a fresh sliced context
    (abg_counters_import: each rank takes its own range of the host copy), which then runs PASS 2."""
    k, counters = 41, 1 << 19
    case = Case(k, counters, 15000, 12, p2_first=64)
    _, buf, off = synthetic_reads(k, 10000, 25.0, 0.01)
    a = make(case)
    a.load(buf, off)
    saved = a.counters()
    eng = make(case)
    eng.import_counters(saved)
    cnt = eng.counters()
    rh, ch = eng.assemble(buf, off)
    ok = _against_oracle(case, buf, off, cnt, rh, ch, eng)
    ok["counting_filter"] = ok["counting_filter"] and bool(np.array_equal(saved, cnt))
    ok["held_fraction"] = eng.stats()["counter_bytes_held"] / float(counters)
    a.close()
    return ok, eng, case


def run(name, arg, make, rank, world):
    """Run case `name` (`arg`: the golden's name; "shared" for `sliced` on gathered read shares) on engines from
    make(case).  Returns (verdicts, the engine that ran it, its Case); the caller closes the engine."""
    if name == "golden":
        return run_golden(arg, make, rank, world)
    if name in SYNTHETIC:
        ok, eng, case = run_synthetic(name, SYNTHETIC[name][7] or (name == "sliced" and arg == "shared"), make, rank, world)
        if name == "sliced":
            ok["held_fraction"] = eng.stats()["counter_bytes_held"] / float(case.counters)
        return ok, eng, case
    if name in PASS1:
        return run_pass1(name, make, rank, world)
    if name == "kept":
        return run_kept(make, rank, world)
    if name == "sliced_checkpoint":
        return run_sliced_checkpoint(make, rank, world)
    raise SystemExit("unknown case")


def shared_stats(eng):
    return {k: v for k, v in eng.stats().items() if k not in PER_RANK_STATS}
