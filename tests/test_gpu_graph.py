"""-g (abg_output_graph_seqs), -C / -R (abg_contains_seq) and abg_reset on a real MI355X, past the points where their buffers
grow and their pieces meet: the cases of tests/graph_cases.py with the real kernels (FTrimRun, FGraphBfs, FRehash, FHash,
FContainsSolid), against the digests of the files the unmodified reference wrote (tests/golden/make_graph_golden.py) and
against the oracle.  tests/test_graph_hostcheck.py runs the same cases through the serial CPU build."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import graph_cases as gc
from abyss_amd import api, build
from util import GoldenCase, contig_tuple

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120  # five times the measured time of either run of the binary below (notes/README.md), not under 120 s


def device(kw, **tuning):
    return api.BloomDBG(kw["k"], counters=kw["counters"], num_hashes=kw["num_hashes"], min_cov=kw["min_cov"], trim=kw["trim"],
                        spaced_seed=kw["mask"], **tuning)


def both(case):
    """The oracle and a device context holding its counting filter (PASS 1 is not what these tests are about)."""
    buf, off, kw = case
    o = gc.make_oracle(kw, buf, off)
    g = device(kw)
    g.set_counters_array(o.counters())
    return buf, off, o, g


@pytest.mark.parametrize("name", gc.SHAPES)
def test_graph_shapes_match_reference_and_oracle(name):
    buf, off, o, g = both(gc.shape_case(name))
    got = g.output_graph(buf, off)
    gc.check_digest(name, *got)
    assert gc.same_dump(got, o.output_graph(buf, off))
    g.close()


@pytest.mark.parametrize("k,K,s", gc.WIDTHS)
def test_every_template_width_matches_reference_and_oracle(k, K, s):
    """FTrimRun / FGraphBfs for 4 and 6 words, and the spaced-seed builds for 1, 3, 4 and 6."""
    buf, off, o, g = both(gc.width_case(k, K, s))
    got = g.output_graph(buf, off)
    gc.check_digest(gc.width_name(k, K, s), *got)
    assert gc.same_dump(got, o.output_graph(buf, off))
    g.close()


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("k,K", gc.SWEEP)
def test_spaced_seed_sweep_matches_oracle(k, K, s):
    buf, off, o, g = both(gc.sweep_case(k, K, s))
    assert gc.same_dump(g.output_graph(buf, off), o.output_graph(buf, off))
    g.close()


@pytest.fixture(scope="module")
def growth():
    buf, off, kw = gc.growth_case()
    o = gc.make_oracle(kw, buf, off)
    return buf, off, kw, o.counters(), o.output_graph(buf, off)


def test_growth_case_grows_node_buffer_and_vertex_table(growth):
    """One launch, a stop for the node buffer and one each for the table at 32,768 and at 65,536 entries: four launches of
    the search at the least, two of the rehash."""
    buf, off, kw, cnt, want = growth
    g = device(kw)
    g.set_counters_array(cnt)
    g.profile_enable()
    g.profile_reset()
    got = g.output_graph(buf, off)
    bfs, rehash = g.profile_get("graph_bfs"), g.profile_get("rehash")
    print("graph_bfs: %.1f ms in %d launches; rehash: %.2f ms in %d" % (bfs + rehash))
    assert bfs[1] >= 4 and rehash[1] >= 2
    gc.check_digest("growth_k40", *got)
    assert gc.same_dump(got, want)
    vbuf, voff = gc.vertex_reads(got[0])  # both rehashes kept every entry
    assert len(voff) - 1 == got[1] and g.output_graph(vbuf, voff, frame=False) == (b"", 0, 0)
    g.close()


def test_growth_case_in_chunks(growth):
    buf, off, kw, cnt, want = growth
    g = device(kw)
    g.set_counters_array(cnt)
    parts, nn, ee = [b"digraph g {\n"], [], []
    cuts = gc.growth_cuts(len(off) - 1)
    for a, b in zip(cuts, cuts[1:]):
        t, x, y = g.output_graph(buf[int(off[a]):int(off[b])], off[a:b + 1] - off[a], frame=False)
        parts.append(t); nn.append(x); ee.append(y)
    assert nn[0] > gc.NODE_CAP0 and sum(nn) > nn[0]
    assert gc.same_dump((b"".join(parts) + b"}\n", sum(nn), sum(ee)), want)
    assert g.output_graph(buf, off, frame=False) == (b"", 0, 0)
    g.close()


def test_components_grow_the_table_in_a_later_call():
    """A call per component, none reaching the table's first limit: later calls rehash a table that holds earlier calls'
    entries (tests/test_graph_hostcheck.py has the reasoning)."""
    sets, (buf, off), kw = gc.components_case()
    o = gc.make_oracle(kw, buf, off)
    want = o.output_graph(buf, off)
    g = device(kw)
    g.set_counters_array(o.counters())
    g.profile_enable()
    g.profile_reset()
    parts, nn, ee = [b"digraph g {\n"], [], []
    for b, f in sets:
        t, x, y = g.output_graph(b, f, frame=False)
        parts.append(t); nn.append(x); ee.append(y)
    assert all(0 < x < gc.TAB_LIMIT0 for x in nn) and sum(nn) > 2 * gc.TAB_LIMIT0, nn
    assert g.profile_get("rehash")[1] == 2
    assert gc.same_dump((b"".join(parts) + b"}\n", sum(nn), sum(ee)), want)
    assert g.output_graph(buf, off, frame=False) == (b"", 0, 0)
    g.close()


def contains(g, seq, cap):
    pos = np.full(max(len(seq), 1), 0xEEEEEEEE, dtype=np.uint32)
    val = np.full(max(len(seq), 1), 0xEE, dtype=np.uint8)
    n = C.c_uint64()
    g._check(g._lib.abg_contains_seq(g._ctx, seq, len(seq), pos.ctypes.data, val.ctypes.data, cap, C.byref(n)), "abg_contains_seq")
    return pos, val, n.value


@pytest.mark.parametrize("name,clean,plant_ns,seams", [(gc.COV_READS, False, False, 1), (gc.COV_READS, True, False, 2),
                                                         ("k48_K16", True, True, 2)])
def test_contains_seq_across_piece_seams(name, clean, plant_ns, seams):
    buf, off, o, g = both(gc.shape_case(name))
    k, min_cov = g.k, 2
    for rname, seq in gc.cov_records(k, gc.cov_text(name), clean=clean, plant_ns=plant_ns):
        po, ho = o.hash_seq(seq)
        want = o.min_count(ho) >= min_cov
        pos, val = g.contains_seq(seq)
        assert np.array_equal(pos, po) and np.array_equal(val.astype(bool), want), rname
        if len(seq) == gc.COV_LONG:
            assert len(gc.cov_seams(k, po)) == seams and 5000 < want.sum() < 2 * 6000 + 4000
            pos2, val2, n2 = contains(g, seq, 1000)
            assert n2 == len(po) and np.array_equal(pos2[:1000], po[:1000]) and np.array_equal(val2[:1000], val[:1000])
            assert (val2[1000:] == 0xEE).all() and (pos2[1000:] == 0xEEEEEEEE).all()
    for seq in (b"", b"N" * 5000, b"ACGT"):
        pos, val = g.contains_seq(seq)
        assert len(pos) == 0 and len(val) == 0
    g.close()


def test_probe_and_graph_are_refused_on_a_cascade():
    g = api.BloomDBG(32, counters=1 << 20, min_cov=0, cascade_levels=2)
    buf, off = api.concat_seqs([b"ACGT" * 20])
    for call in (lambda: g.contains_seq(buf), lambda: g.output_graph(buf, off)):
        with pytest.raises(api.AbyssAmdError) as e:
            call()
        assert "cascading" in str(e.value), str(e.value)
    g.close()


def cli():
    path = build.build_cli()
    assert path and os.path.exists(path)
    return path


def test_cli_coverage_track_across_piece_seams(tmp_path):
    """-C / -R on the three-record reference: the WIG file the unmodified reference wrote."""
    ref = gc.golden()["cov_track_k40"]
    g = GoldenCase(ref["reads"])
    (tmp_path / "reads.fa").write_bytes(gc.reads_fasta(g.buf, g.off))
    (tmp_path / "ref.fa").write_bytes(gc.cov_fasta(gc.cov_records(g.opts["k"], gc.cov_text(ref["reads"]))))
    r = subprocess.run([cli()] + ref["options"] + ["-j1", "-C", "cov.wig", "-R", "ref.fa", "reads.fa"], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CLI_TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == g.fasta
    wig = (tmp_path / "cov.wig").read_bytes()
    assert (len(wig), wig.count(b"variableStep")) == (ref["bytes"], ref["steps"])
    assert hashlib.sha256(wig).hexdigest() == ref["sha256"]


def test_cli_graphviz_dump_of_the_growth_case(tmp_path):
    ref = gc.golden()["growth_k40"]
    buf, off = gc.growth_reads()
    (tmp_path / "reads.fa").write_bytes(gc.reads_fasta(buf, off))
    r = subprocess.run([cli()] + ref["options"] + ["-j1", "-v", "-g", "g.dot", "reads.fa"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=CLI_TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()
    dot = (tmp_path / "g.dot").read_bytes()
    assert len(dot) == ref["bytes"] and hashlib.sha256(dot).hexdigest() == ref["sha256"]
    assert ("(k-mers visited: %d, edges visited: %d)" % (ref["nodes"], ref["edges"])).encode() in r.stderr


def cycle(g, gold):
    g.load(gold.buf, gold.off)
    results, contigs = g.assemble(gold.buf, gold.off)
    return (api.format_fasta(contigs, gold.ids), api.format_read_log(results, gold.ids), [contig_tuple(c) for c in contigs],
            g.visited().tobytes(), g.counters().tobytes(), g.assembly_counters(), g.output_graph(gold.buf, gold.off))


def test_reset_gives_a_fresh_context_on_the_device():
    """abg_reset: the second cycle on one context equals a fresh context's -- FASTA, read log, visited filter, counters
    and the graph text in full (the set of seen vertices is forgotten)."""
    gold = GoldenCase("k40_mixed")
    fresh = api.BloomDBG(**gold.kwargs())
    want = cycle(fresh, gold)
    fresh.close()
    assert (want[0], want[1]) == (gold.fasta, gold.readlog)
    gc.check_digest("k40_mixed", *want[6])
    g = api.BloomDBG(**gold.kwargs())
    assert cycle(g, gold) == want
    g.reset()
    assert not g.counters().any() and not g.visited().any() and g.assembly_counters()["next_contig_id"] == 0
    assert cycle(g, gold) == want
    g.close()


def test_reset_drops_the_kept_reads():
    """keep_reads, load, reset: nothing is kept and keeping is off, as after abg_create."""
    gold = GoldenCase("k40_mixed")
    g = api.BloomDBG(**gold.kwargs())
    g.keep_reads(True, len(gold.buf))
    g.load(gold.buf, gold.off)
    g.reset()
    with pytest.raises(api.AbyssAmdError) as e:
        g.assemble_kept(gold.n)
    assert "no reads are kept" in str(e.value), str(e.value)
    g.load(gold.buf, gold.off)
    results, contigs = g.assemble(gold.buf, gold.off)
    assert api.format_fasta(contigs, gold.ids) == gold.fasta
    assert api.format_read_log(results, gold.ids) == gold.readlog
    with pytest.raises(api.AbyssAmdError):
        g.assemble_kept(gold.n)
    g.close()
