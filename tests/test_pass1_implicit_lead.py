"""PASS 1's implicit `lead` (TileEnv::lead_implicit, lead_of in abg_engine.h): a pair that is alone on a pure counter stores
nothing, and op_verdict reads the `lead` word nobody wrote as "one op, its own leader" unless the op's first two counters are both
shared.  And TileEnv::amask: tile_purity leaves a bit per pair, tile_apply gathers no target for a pair that cannot belong to a
leader.  The device logic run serially through tests/hostcheck, with either rule on and off (ABG_LEAD_IMPLICIT, ABG_APPLY_MASK):
the counter array is the oracle's sequential incrementMin under all four settings, and the verdicts are the same op for op -- as
many ops left to the reservation rounds, as many rounds."""
import numpy as np
import pytest

import oracle_binding as ob
from abyss_amd import api, synth
from test_hostcheck import HostCheck
from util import GoldenCase, mask_of

SETTINGS = (("implicit", {}), ("explicit", {"ABG_LEAD_IMPLICIT": "0"}), ("nomask", {"ABG_APPLY_MASK": "0"}),
            ("neither", {"ABG_LEAD_IMPLICIT": "0", "ABG_APPLY_MASK": "0"}))
KEYS = ("ABG_LEAD_IMPLICIT", "ABG_APPLY_MASK", "ABG_TILE_CAP")


def run_settings(monkeypatch, buf, off, k, counters, num_hashes=4, insert_batch=30000, env=None):
    """Loads the reads under every setting; the counters against the oracle's, the verdicts against each other.  Returns the
    statistics of the default setting."""
    o = ob.Oracle(k, counters=counters, num_hashes=num_hashes)
    o.load(buf, off)
    want = o.counters()
    seen = {}
    for name, knobs in SETTINGS:
        for key in KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in {**(env or {}), **knobs}.items():
            monkeypatch.setenv(key, val)
        hc = HostCheck(k, counters, num_hashes=num_hashes, insert_batch=insert_batch, claim_log2=16)
        hc.load(buf, off)
        assert np.array_equal(want, hc.counters()), (name, counters, num_hashes)
        seen[name] = hc.stats()
    for key in ("tiled_ops", "tiled_pending", "insert_rounds", "tile_overflows"):
        assert len({st[key] for st in seen.values()}) == 1, (key, seen)
    return seen["implicit"]


@pytest.fixture(scope="module")
def reads30k():
    m1, m2 = synth.make_read_set(30000, 30.0)
    return api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))


@pytest.mark.parametrize("counters", [1 << 21, 1 << 19, 1 << 18])
def test_sparse_medium_and_dense_filters(counters, reads30k, monkeypatch):
    """At 2^21 counters nearly every counter is pure, at 2^18 both first counters of an op are often shared (nothing known: the
    rounds)."""
    st = run_settings(monkeypatch, *reads30k, 40, counters)
    assert st["tiled_ops"] > 0 and st["tile_overflows"] == 0 and 0 < st["tiled_pending"] < st["tiled_ops"], st


@pytest.mark.parametrize("nh", [1, 2, 3, 8, 9])
def test_few_and_many_hash_functions(nh, monkeypatch):
    """One hash function (the mask is one bit: no second counter to learn from), two, three, a full flag byte, and nine (a flagged op
    has 0xFF and takes the rounds before `lead` is looked at)."""
    m1, m2 = synth.make_read_set(20000, 30.0)
    buf, off = api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))
    st = run_settings(monkeypatch, buf, off, 33, 1 << 19, num_hashes=nh)
    assert st["tiled_ops"] > 0, st


@pytest.mark.parametrize("copies", [2, 3])
@pytest.mark.parametrize("layout", ["adjacent", "apart"])
def test_every_read_twice_and_three_times(copies, layout, monkeypatch):
    """k-mers with n = 2 and n = 3 ops in a batch (explicit values) beside the singletons that sequencing errors make, the copies of a
    read back to back or a whole read set apart."""
    m1, m2 = synth.make_read_set(6000, 30.0)
    reads = synth.codes_to_ascii(np.concatenate([m1, m2]))
    rep = np.repeat(reads, copies, axis=0) if layout == "adjacent" else np.tile(reads, (copies, 1))
    buf, off = api.matrix_to_seqs(rep)
    st = run_settings(monkeypatch, buf, off, 40, 1 << 19, insert_batch=1 << 20)
    assert st["tiled_ops"] > 0 and st["tile_overflows"] == 0, st


def test_a_repeat_that_saturates_and_homopolymer_runs(monkeypatch):
    rep = np.tile(np.frombuffer(b"ACGTTGCATGCCGATAGCTAGGATCCATGCAAGCTTGGCATTCGGATACCGGTAAGCTAGCTAACGGT", dtype=np.uint8), (400, 1))
    buf, off = api.matrix_to_seqs(rep)
    run_settings(monkeypatch, buf, off, 40, 1 << 18)
    o = ob.Oracle(40, counters=1 << 18)
    o.load(buf, off)
    assert o.counters().max() == 255
    # 1,665 ops of one k-mer in a bin, beside k-mers of 50 and of 20 ops
    buf, off = api.concat_seqs([b"A" * 150] * 15 + [bytes(r) for r in rep[:50]] + [b"AC" * 75] * 20)
    st = run_settings(monkeypatch, buf, off, 40, 1 << 20)
    assert st["tiled_ops"] > 0 and st["tiled_pending"] == 0 and st["tile_overflows"] == 0 and st["insert_rounds"] == 0, st


def test_bins_that_overflow(reads30k, monkeypatch):
    """Bins too small for the batch (the sorted judge applies the same rule; both arrays are cleared before it), and k-mers that recur
    thousands of times among ordinary reads, whose pairs run real bins over."""
    st = run_settings(monkeypatch, *reads30k, 40, 1 << 21, env={"ABG_TILE_CAP": "600"})
    assert st["tile_overflows"] > 0, st
    m1, m2 = synth.make_read_set(30000, 30.0)
    plain = [bytes(r) for r in synth.codes_to_ascii(np.concatenate([m1, m2]))]
    hot = [b"A" * 150] * 400 + [b"AC" * 75] * 300 + [b"CA" * 75] * 100 + [(b"GATTA" * 30)[i % 5:][:140] for i in range(300)]
    hot += [b"T" * 150] * 100
    mixed = plain + hot
    order = np.random.default_rng(4).permutation(len(mixed))
    buf, off = api.concat_seqs([mixed[i] for i in order])
    st = run_settings(monkeypatch, buf, off, 40, 1 << 21, insert_batch=1 << 20)
    assert st["tile_overflows"] > 0 and st["tiled_ops"] > 0, st


_DEFAULT_PASS1 = {}


@pytest.mark.parametrize("tag", [t for t, _ in SETTINGS])
@pytest.mark.parametrize("name", ["k64", "k40_mixed", "s_tandem_k32", "s_inverted_k40", "s_lowcomplex_k25", "s_satellite_k40", "k48_K16"])
def test_reference_runs(name, tag, monkeypatch):
    """The reference's FASTA and read log (k48_K16: under a spaced seed) under each setting; the other three against PASS 1 of the
    default setting: the same counters, ops left to the rounds and rounds."""
    g = GoldenCase(name)
    kw = g.kwargs()

    def loaded(knobs):
        for key in KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in knobs.items():
            monkeypatch.setenv(key, val)
        hc = HostCheck(kw["k"], g.meta["counters"], kw["num_hashes"], kw["min_cov"], kw["trim"], insert_batch=50000, claim_log2=16,
                       p2_first=128, mask=mask_of(g))
        hc.load(g.buf, g.off)
        st = hc.stats()
        return hc, (st["tiled_pending"], st["insert_rounds"], st["tile_overflows"]), hc.counters()

    hc, verdicts, counters = loaded(dict(SETTINGS)[tag])
    assert hc.counting_stats()[1] == g.meta["filtered_popcount"]
    results, contigs = hc.assemble(g.buf, g.off)
    assert api.format_fasta(contigs, g.ids) == g.fasta
    assert api.format_read_log(results, g.ids) == g.readlog
    if tag == SETTINGS[0][0]:
        _DEFAULT_PASS1[name] = (verdicts, counters)
    else:
        if name not in _DEFAULT_PASS1:  # (computed once per golden, whichever case comes first)
            _DEFAULT_PASS1[name] = loaded(SETTINGS[0][1])[1:]
        want_verdicts, want_counters = _DEFAULT_PASS1[name]
        assert verdicts == want_verdicts
        assert np.array_equal(counters, want_counters)
