"""The parallel commit's incremental passes (Engine::commit_par): a pass after the first re-stamps and re-decides only what the
pass before moved.  Whatever form the passes take -- incremental, all full (ABG_COMMIT_INCREMENTAL=0), falling back because the
list of moved records is too short, a map of moved stamps so small that its hashed positions collide all the time, tags that run
out between passes, hashed time stamps (where incremental passes are taken only when asked for) -- the commit computes the same iterates: same FASTA bytes, contig ids and coverage, same
visited filter, same counters and the same number of passes.  Inputs that stress the commit: tandem repeats, hairpins,
satellites, homopolymer runs, a spaced seed, and a filter so small that false positives chain the decisions over many short
contigs."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from abyss_amd import api, synth
from util import GoldenCase, contig_tuple, mask_of

GOLDENS = ["s_tandem_k32", "s_inverted_k40", "s_satellite_k40", "s_lowcomplex_k25", "k48_K16", "k40_mixed"]
INPUTS = GOLDENS + ["small_filter"]
# every variant must equal the run whose passes are all full ones
VARIANTS = [
    {},                                                        # the default: incremental passes where they can be taken
    {"ABG_COMMIT_DIRTY_MAX": "1"},                             # a list of one record: nearly every pass falls back
    {"ABG_COMMIT_DIRTY_LOG2": "10"},                           # a map of 1024 hashed positions: collisions everywhere
    {"ABG_T_TAGS": "2"},                                       # the tags run out between any two passes
    {"ABG_PAR_COMMIT_MAX_GB": "0"},                            # hashed time stamps: full passes by default
    {"ABG_PAR_COMMIT_MAX_GB": "0", "ABG_COMMIT_INCREMENTAL": "2"},  # ... and with incremental passes asked for
    {"ABG_PAR_COMMIT_MAX_GB": "0", "ABG_COMMIT_INCREMENTAL": "2", "ABG_T_TAGS": "5", "ABG_COMMIT_DIRTY_LOG2": "12"},
]
OFF = {"ABG_COMMIT_INCREMENTAL": "0"}


def _input(name):
    """(k, counters, num_hashes, min_cov, trim, mask, buf, off, ids, golden case or None)"""
    if name == "small_filter":
        # (tests/test_hostcheck.py::test_parallel_commit_needs_several_passes_and_stays_exact: errors make many short contigs,
        # the small filter makes their decisions depend on each other)
        m1, m2 = synth.make_read_set(8000, 30.0, err=0.02, genome_seed=30, read_seed=34)
        buf, off = api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))
        return dict(k=25, counters=1 << 17, num_hashes=4, min_cov=2, trim=None, mask=None, buf=buf, off=off,
                    ids=[b"r%d" % i for i in range(len(off) - 1)], golden=None)
    g = GoldenCase(name)
    kw = g.kwargs()
    return dict(k=kw["k"], counters=g.meta["counters"], num_hashes=kw["num_hashes"], min_cov=kw["min_cov"], trim=kw["trim"],
                mask=mask_of(g), buf=g.buf, off=g.off, ids=g.ids, golden=g)


def _set_env(monkeypatch, env):
    for key in ("ABG_COMMIT_INCREMENTAL", "ABG_COMMIT_DIRTY_MAX", "ABG_COMMIT_DIRTY_LOG2", "ABG_T_TAGS", "ABG_PAR_COMMIT_MAX_GB"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)


def _digest(inp, results, contigs, visited, counters, stats, extra):
    return dict(fasta=hashlib.sha256(api.format_fasta(contigs, inp["ids"])).hexdigest(),
                contigs=[contig_tuple(c) for c in contigs], results=bytes(results),
                visited=hashlib.sha256(visited.tobytes()).hexdigest(), counters=counters,
                commit_rounds=stats["commit_rounds"], walk_rounds=stats["walk_rounds"], **extra)


def _run_host(inp, env, monkeypatch):
    from test_hostcheck import HostCheck
    _set_env(monkeypatch, env)  # (the engine reads its knobs when the session is created)
    hc = HostCheck(inp["k"], inp["counters"], inp["num_hashes"], inp["min_cov"], inp["trim"], insert_batch=50000, claim_log2=16,
                   p2_first=64, mask=inp["mask"])
    hc.load(inp["buf"], inp["off"])
    results, contigs = hc.assemble(inp["buf"], inp["off"])
    hc.l.hc_get_commit_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    more = (C.c_uint64 * 3)()
    hc.l.hc_get_commit_stats(hc.h, more)
    return _digest(inp, results, contigs, hc.visited(), hc.assembly_counters(), hc.stats(),
                   dict(incremental=int(more[0]), dirty=int(more[1]), first_chunk=int(more[2])))


def _run_gpu(inp, env, monkeypatch):
    _set_env(monkeypatch, dict(env, ABG_P2_FIRST_BATCH="256"))
    g = api.BloomDBG(inp["k"], counters=inp["counters"], num_hashes=inp["num_hashes"], min_cov=inp["min_cov"], trim=inp["trim"],
                     spaced_seed=inp["mask"], insert_batch_kmers=1 << 17)
    g.load(inp["buf"], inp["off"])
    results, contigs = g.assemble(inp["buf"], inp["off"])
    st = g.stats()
    d = _digest(inp, results, contigs, g.visited(), g.assembly_counters(), st,
                dict(incremental=st["commit_rounds_incremental"], dirty=st["commit_dirty_records"],
                     first_chunk=st["commit_first_chunk_decided"]))
    g.close()
    return d


def _check(run, name, monkeypatch):
    inp = _input(name)
    full = run(inp, OFF, monkeypatch)
    assert full["incremental"] == 0, full["incremental"]
    assert full["commit_rounds"] > 0
    if inp["golden"] is not None:
        assert full["fasta"] == hashlib.sha256(inp["golden"].fasta).hexdigest()
    taken = {}
    for env in VARIANTS:
        got = run(inp, env, monkeypatch)
        for key in ("fasta", "contigs", "results", "visited", "counters", "commit_rounds", "walk_rounds", "dirty"):
            assert got[key] == full[key], (name, env, key)
        # (the early exits of the scans do not depend on the form of the passes)
        taken[tuple(sorted(env.items()))] = got["incremental"]
        if env.get("ABG_T_TAGS") == "2" or (env.get("ABG_PAR_COMMIT_MAX_GB") == "0" and "ABG_COMMIT_INCREMENTAL" not in env):
            assert got["incremental"] == 0, (name, env)
    return full, taken


@pytest.mark.parametrize("name", INPUTS)
def test_incremental_passes_compute_what_full_passes_compute(name, monkeypatch):
    full, taken = _check(_run_host, name, monkeypatch)
    print(name, "commit_rounds", full["commit_rounds"], "dirty", full["dirty"], "first_chunk", full["first_chunk"], "incremental", taken)
    if name == "small_filter":
        # commits that need more than one pass: the new path cannot be silently dead, nor can its variants
        assert full["commit_rounds"] > full["walk_rounds"] and full["dirty"] > 0
        assert taken[()] > 0
        assert taken[(("ABG_COMMIT_DIRTY_LOG2", "10"),)] > 0
        assert taken[(("ABG_COMMIT_INCREMENTAL", "2"), ("ABG_PAR_COMMIT_MAX_GB", "0"))] > 0
        assert taken[(("ABG_COMMIT_DIRTY_MAX", "1"),)] < taken[()]
        assert full["first_chunk"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_incremental_passes_compute_what_full_passes_compute_on_the_device(name, monkeypatch):
    full, taken = _check(_run_gpu, name, monkeypatch)
    print(name, "commit_rounds", full["commit_rounds"], "dirty", full["dirty"], "first_chunk", full["first_chunk"], "incremental", taken)
    if name == "small_filter":
        assert full["commit_rounds"] > full["walk_rounds"] and full["dirty"] > 0
        assert taken[()] > 0 and taken[(("ABG_COMMIT_INCREMENTAL", "2"), ("ABG_PAR_COMMIT_MAX_GB", "0"))] > 0
        assert full["first_chunk"] > 0
