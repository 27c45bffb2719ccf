"""The classification's reads drawn by ticket (k_foreach_wt) and its lane count sized for the wave slots: which wave handles
which read, and how many run at once, changes no verdict.  Through the C ABI on a real MI355X, against the oracle: per-read
result bytes, assembly counters and FASTA, at every lane count and at read counts around the 64 reads of a ticket."""
import numpy as np
import pytest

import oracle_binding as ob
from abyss_amd import api
from util import contig_tuple

pytestmark = pytest.mark.gpu

K, L, COUNTERS = 32, 100, 1 << 24
N_SMALL = 6000      # the reads the small cases' filter is built from
N_BIG = 220_003     # more reads in one launch than the largest lane count has lanes; no multiple of 64, so of no 64 x grid either
SLOTS_OLD = 65536
BATCH_ENV = {"ABG_P2_FIRST_BATCH": "1024", "ABG_P2_GROWTH": "16", "ABG_P2_STARVED": "0"}  # batches of 1,024, 16,384 and the other 202,595 reads


def _slots_max():
    """One lane per wave slot the kernel is compiled for on an MI355X: 256 CUs x 4 SIMDs x 3 waves x 64 lanes (what the engine
    takes unasked there; asked for by name here, so that the lane count does not hang on how much memory is free)."""
    return 256 * 4 * 3 * 64


def _read_matrix(n, seed):
    """`n` reads of L bases at random places of a genome full of tandem repeats, hairpins and self-complementary stretches
    (tests/test_stress_logic.py: reads ending in them take the generic look-ahead search), 0.3 % substitutions, every other
    read reverse-complemented."""
    from test_stress_logic import _structured_genome
    rng = np.random.default_rng(seed)
    G = 60000
    g = np.frombuffer(_structured_genome(rng, G), dtype=np.uint8)
    starts = rng.integers(0, G - L, size=n)
    m = g[starts[:, None] + np.arange(L)[None, :]].copy()
    hit = rng.random(m.shape) < 0.003
    m[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m[1::2] = comp[m[1::2, ::-1]]
    return m


@pytest.fixture(scope="module")
def big():
    """The large read set and the oracle's answer for it, computed once and left unchanged."""
    buf, off = api.matrix_to_seqs(_read_matrix(N_BIG, 9100))
    o = ob.Oracle(K, counters=COUNTERS)
    o.load(buf, off)
    res, contigs = o.assemble(buf, off)
    ids = [b"r%d" % i for i in range(N_BIG)]
    want = dict(res=res, contigs=[contig_tuple(c) for c in contigs], fasta=api.format_fasta(contigs, ids), counters=o.assembly_counters(),
                visited=o.visited())
    o.close()
    return buf, off, ids, want


@pytest.fixture(scope="module")
def small(big):
    buf, off, _, _ = big
    return buf[:int(off[N_SMALL])], off[:N_SMALL + 1]


def _gpu_run(load, reads, slots, monkeypatch, env=()):
    for key in ("ABG_CLS_SLOTS", "ABG_PREFETCH", "ABG_MEM_LIMIT_MB", *BATCH_ENV):
        monkeypatch.delenv(key, raising=False)
    if slots is not None:
        monkeypatch.setenv("ABG_CLS_SLOTS", str(slots))
    for key, val in dict(env).items():
        monkeypatch.setenv(key, val)
    g = api.BloomDBG(K, counters=COUNTERS)
    g.load(*load)
    res, contigs = g.assemble(*reads)
    out = dict(res=res, contigs=[contig_tuple(c) for c in contigs], counters=g.assembly_counters(), visited=g.visited(), stats=g.stats(),
               fasta=api.format_fasta(contigs, [b"r%d" % i for i in range(len(reads[1]) - 1)]))
    g.close()
    return out


def _same(got, want, what):
    assert np.array_equal(got["res"], want["res"]), (what, int(np.sum(got["res"] != want["res"])))
    assert got["contigs"] == want["contigs"], what
    assert got["fasta"] == want["fasta"], what
    assert got["counters"] == want["counters"], what
    assert np.array_equal(got["visited"], want["visited"]), what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_read_counts_around_a_ticket_at_every_lane_count(n, small, monkeypatch):
    """1, 63, 64, 65 and 4,097 reads (a ticket is 64 reads) with 64 lanes -- one wave draws every ticket --, 128, the old 65,536
    and one per wave slot: the oracle's verdicts, counters and FASTA, at every lane count."""
    reads = (small[0][:int(small[1][n])], small[1][:n + 1])
    o = ob.Oracle(K, counters=COUNTERS)
    o.load(*small)
    res, contigs = o.assemble(*reads)
    want = dict(res=res, contigs=[contig_tuple(c) for c in contigs], fasta=api.format_fasta(contigs, [b"r%d" % i for i in range(n)]),
                counters=o.assembly_counters(), visited=o.visited())
    o.close()
    for slots in (64, 128, SLOTS_OLD, _slots_max()):
        _same(_gpu_run(small, reads, slots, monkeypatch), want, (n, slots))


@pytest.mark.parametrize("slots", [64, 128, SLOTS_OLD, "max"])
def test_more_reads_in_a_launch_than_lanes(slots, big, monkeypatch):
    """220,003 reads, the last 202,595 of them one batch: more than the 196,608 lanes of the largest count (3,166 tickets for its
    3,072 waves, the last ticket holds 35 reads), no multiple of 64 times any grid.  Each lane count gives the oracle's
    bytes, so all of them the same."""
    buf, off, _, want = big
    got = _gpu_run((buf, off), (buf, off), _slots_max() if slots == "max" else slots, monkeypatch, BATCH_ENV)
    assert got["stats"]["walk_rounds"] >= 3, got["stats"]
    _same(got, want, slots)


def test_reads_that_search_beside_reads_the_archive_decides(big, monkeypatch):
    """At one lane per wave slot, a batch larger than the grid, so that lanes all over it meet both kinds of read: those whose ends lie
    in repeats and hairpins -- look_ahead_reg gives up and the generic search fills the lane's scratch, which is found from the
    lane's place in the grid -- and those the archive of the first two batches' contigs decides without a probe."""
    buf, off, _, want = big
    got = _gpu_run((buf, off), (buf, off), _slots_max(), monkeypatch, BATCH_ENV)
    st = got["stats"]
    assert st["cls_decided_reads"] > 1000 and st["cls_covered_reads"] > st["cls_decided_reads"], st
    assert 0 < int(np.sum(want["res"] == 3)) and 0 < int(np.sum(want["res"] == 4)), np.bincount(want["res"])  # blunt ends, unsolid reads
    _same(got, want, "max")


@pytest.mark.parametrize("slots", [None, 64])
def test_side_and_main_launches_follow_each_other(slots, small, monkeypatch):
    """Many small batches: the first is classified on the main stream, every later one ahead on the side stream, each launch
    clearing its stream's ticket counter again."""
    o = ob.Oracle(K, counters=COUNTERS)
    o.load(*small)
    res, contigs = o.assemble(*small)
    want = dict(res=res, contigs=[contig_tuple(c) for c in contigs], fasta=api.format_fasta(contigs, [b"r%d" % i for i in range(N_SMALL)]),
                counters=o.assembly_counters(), visited=o.visited())
    o.close()
    got = _gpu_run(small, small, slots, monkeypatch, {"ABG_P2_FIRST_BATCH": "64"})
    assert got["stats"]["walk_rounds"] > 4, got["stats"]
    _same(got, want, slots)
    # ... and a second pass over the same reads on the same context's counters finds them all visited: main-stream launch after side-stream launches
    monkeypatch.setenv("ABG_P2_FIRST_BATCH", "64")
    g = api.BloomDBG(K, counters=COUNTERS)
    g.load(*small)
    r1, _ = g.assemble(*small)
    r2, c2 = g.assemble(*small)
    g.close()
    assert np.array_equal(r1, want["res"])
    solid = np.isin(r1, [5, 7])
    assert np.all(np.isin(r2[solid], [5, 7])) and np.array_equal(r1[~solid], r2[~solid]) and all(c.redundant for c in c2)


def test_lane_count_follows_the_free_memory(small, monkeypatch):
    """Unasked, the classification takes a lane per wave slot where its two scratch pools (2 x 4.3 GB on 256 CUs) fit an eighth of the
    free memory, else the old 65,536 -- a 24 GB budget leaves no such room, and the run goes through all the same; ABG_CLS_SLOTS is
    taken at its word."""
    o = ob.Oracle(K, counters=COUNTERS)
    o.load(*small)
    res, contigs = o.assemble(*small)
    want = dict(res=res, contigs=[contig_tuple(c) for c in contigs], fasta=api.format_fasta(contigs, [b"r%d" % i for i in range(N_SMALL)]),
                counters=o.assembly_counters(), visited=o.visited())
    o.close()
    free = _gpu_run(small, small, None, monkeypatch)
    assert free["stats"]["cls_lanes"] in (SLOTS_OLD, _slots_max()), free["stats"]
    _same(free, want, "unasked")
    tight = _gpu_run(small, small, None, monkeypatch, {"ABG_MEM_LIMIT_MB": "24576"})
    assert tight["stats"]["cls_lanes"] == SLOTS_OLD, tight["stats"]
    _same(tight, want, "24 GB")
    asked = _gpu_run(small, small, 128, monkeypatch)
    assert asked["stats"]["cls_lanes"] == 128, asked["stats"]


def test_the_wait_for_the_classification_is_reported(small, monkeypatch):
    """cls_wait_ms: there, never negative, and 0 where nothing is classified ahead."""
    on = _gpu_run(small, small, None, monkeypatch, {"ABG_P2_FIRST_BATCH": "64"})["stats"]
    assert "cls_wait_ms" in on and on["cls_wait_ms"] >= 0.0 and on["walk_rounds"] > 4, on
    off = _gpu_run(small, small, None, monkeypatch, {"ABG_P2_FIRST_BATCH": "64", "ABG_PREFETCH": "0"})["stats"]
    assert off["cls_wait_ms"] == 0.0 and off["walk_rounds"] > 4, off
