"""PASS 1's implicit `lead` on the device (TileEnv::lead_implicit, lead_of in abg_engine.h): tile_purity and the sorted judge store
nothing for a pair that is alone on a pure counter, op_verdict reads the word nobody wrote; and TileEnv::amask: a bit per pair from
a ballot in tile_purity, by which tile_apply picks the address of its target gather.  With either rule on and off
(ABG_LEAD_IMPLICIT, ABG_APPLY_MASK) the counter array is the oracle's sequential incrementMin, and as many ops take as many reservation rounds."""
import numpy as np
import pytest

import oracle_binding as ob
from abyss_amd import api, synth
from util import contig_tuple

pytestmark = pytest.mark.gpu

SETTINGS = (("implicit", {}), ("explicit", {"ABG_LEAD_IMPLICIT": "0"}), ("nomask", {"ABG_APPLY_MASK": "0"}),
            ("neither", {"ABG_LEAD_IMPLICIT": "0", "ABG_APPLY_MASK": "0"}))
KEYS = ("ABG_LEAD_IMPLICIT", "ABG_APPLY_MASK", "ABG_TILE_CAP", "ABG_OVERLAP_PURITY")


def run_settings(monkeypatch, buf, off, k, counters, insert_batch_kmers=1 << 17, env=None, contigs=False):
    o = ob.Oracle(k, counters=counters)
    o.load(buf, off)
    want = o.counters()
    want_asm = o.assemble(buf, off) if contigs else None
    seen = {}
    for name, knobs in SETTINGS:
        for key in KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in {**(env or {}), **knobs}.items():
            monkeypatch.setenv(key, val)
        g = api.BloomDBG(k, counters=counters, insert_batch_kmers=insert_batch_kmers)
        g.load(buf, off)
        assert np.array_equal(want, g.counters()), (name, counters)
        seen[name] = g.stats()
        if contigs:
            res, cs = g.assemble(buf, off)
            assert np.array_equal(want_asm[0], res), name
            assert [contig_tuple(c) for c in want_asm[1]] == [contig_tuple(c) for c in cs], name
        g.close()
    for key in ("tiled_ops", "tiled_pending", "insert_rounds", "tile_overflows"):
        assert len({st[key] for st in seen.values()}) == 1, (key, seen)
    return seen["implicit"]


@pytest.fixture(scope="module")
def reads60k():
    m1, m2 = synth.make_read_set(60000, 40.0, err=0.006, genome_seed=11, read_seed=12)
    return api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))


@pytest.mark.parametrize("counters", [1 << 22, 1 << 20, 1 << 19])
def test_several_staged_batches_at_three_occupancies(counters, reads60k, monkeypatch):
    """Several batches: all but the first are judged while they are staged, into the second set of `lead` and flags."""
    st = run_settings(monkeypatch, *reads60k, 48, counters, contigs=counters == 1 << 22)
    assert st["tiled_ops"] > 0 and st["tile_overflows"] == 0 and 0 < st["tiled_pending"] < st["tiled_ops"], st


def test_every_read_twice(monkeypatch):
    m1, m2 = synth.make_read_set(12000, 40.0, err=0.006, genome_seed=11, read_seed=12)
    reads = synth.codes_to_ascii(np.concatenate([m1, m2]))
    buf, off = api.matrix_to_seqs(np.concatenate([np.repeat(reads[:6000], 2, axis=0), np.tile(reads[6000:], (2, 1))]))
    st = run_settings(monkeypatch, buf, off, 48, 1 << 20)
    assert st["tiled_ops"] > 0 and st["tile_overflows"] == 0, st


def test_kmers_that_recur_thousands_of_times(monkeypatch):
    """Real bins run over: the sorted judge leaves the same `lead` as the tiles would."""
    m1, m2 = synth.make_read_set(30000, 30.0)
    plain = [bytes(r) for r in synth.codes_to_ascii(np.concatenate([m1, m2]))]
    hot = [b"A" * 150] * 400 + [b"AC" * 75] * 300 + [b"CA" * 75] * 100 + [(b"GATTA" * 30)[i % 5:][:140] for i in range(300)] + [b"T" * 150] * 100
    mixed = plain + hot
    order = np.random.default_rng(4).permutation(len(mixed))
    buf, off = api.concat_seqs([mixed[i] for i in order])
    st = run_settings(monkeypatch, buf, off, 40, 1 << 21, insert_batch_kmers=0)
    assert st["tile_overflows"] > 0 and st["tiled_ops"] > 0, st


@pytest.mark.parametrize("env", [{"ABG_OVERLAP_PURITY": "0"}, {"ABG_TILE_CAP": "300"}])
def test_purity_on_the_main_stream_and_bins_too_small(env, reads60k, monkeypatch):
    st = run_settings(monkeypatch, *reads60k, 48, 1 << 20, env=env)
    if "ABG_TILE_CAP" in env:
        assert st["tile_overflows"] > 0, st
    else:
        assert st["tiled_ops"] > 0 and st["tile_overflows"] == 0, st
