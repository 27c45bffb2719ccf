"""MergeContigs on the GPU.  api.PathMerge.merge (the two kernels of abg_mc.hip) must equal the plain-Python restatement of
tests/mergecontigs_golden.py on generated sets that reach the seams of the kernels -- a wave of paths, a wave of overlap window, a
contig longer than a tile, segments that end around a tile's edge, batches of a few paths -- and must not hand a path to the host
unless a junction of it has no consensus.  The binary must write every golden case (tests/golden/mergecontigs, from the unmodified
reference) byte for byte, at the default tile and batch, at a tile of 64 and at the smallest tile, 16, each a path a batch.

The sets of mergecontigs_golden.dirty_sets() carry what chains() does not: lower case, N and codes in windows wider than a wave
(a marked character at lanes 0, 62, 63, 64 and the last), overlaps that differ within a path, nodes that are all window, gaps of
1 to 2k across chunks of sixteen bytes and a gap's N and n runs side by side, planned conflicts at chosen positions, junctions and
indices of a call, windows of 1023 and 1024 characters, a path of 1025 that is the host's from the start beside device paths, and
eight nodes of a few characters with many seams a chunk.  Every one of them asserts `redone` path by path and the rise of
`mc_redone` exactly, so a path the host took cannot pass for a device result."""
import os

import pytest

from abyss_amd import api, build
import mergecontigs_golden as mcg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def merger():
    m = api.PathMerge()
    yield m
    m.close()


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "MergeContigs")


def acgt(s):
    return sum(s.count(c) for c in b"ACGTacgt")


def check(m, k, contigs, paths, tile=16384, batch=1 << 20, want=None, host=()):
    """want: py_merge_path of every path, where it is at hand; host: the paths the ring cannot hold, the host's from the start"""
    m.tune(tile=tile, batch=batch)
    m.set_contigs(contigs)
    before = m.profile_get("mc_redone")[1]
    seqs, counts, redone, logs = m.merge(k, paths)
    want = want or [mcg.py_merge_path(contigs, k, nodes, ov) for nodes, ov in paths]
    assert len(seqs) == len(want) == len(paths)
    for i, (seq, flagged, log) in enumerate(want):
        assert seqs[i] == seq, i
        assert int(counts[i]) == acgt(seq), i
        assert bool(redone[i]) == (flagged or i in host), i
    assert m.profile_get("mc_redone")[1] - before == sum(f or i in host for i, (_, f, _) in enumerate(want))
    return seqs


def check_set(m, name, tile=16384, batch=1 << 20):
    """a set of mergecontigs_golden.dirty_sets(), against its restatement (computed once)"""
    s = mcg.dirty_sets()[name]
    return check(m, s["k"], s["contigs"], s["paths"], tile, batch, want=mcg.expected(name), host=s["host"])


@pytest.mark.parametrize("npaths", [1, 63, 64, 65, 257])
def test_numbers_of_paths_around_a_wave(merger, npaths):
    contigs, paths = mcg.chains(npaths, 25, npaths, lambda p: [40 + p % 9, 25 + p % 3, 33 + p % 7])
    check(merger, 25, contigs, paths)


@pytest.mark.parametrize("overlap", [1, 63, 64, 65, 95])
def test_overlaps_around_a_wave(merger, overlap):
    """lengths from the overlap itself (a contig that is all window) to twice it and more"""
    contigs, paths = mcg.chains(100 + overlap, overlap + 1, 9, lambda p: [overlap + p, overlap + (p % 3), 2 * overlap + p, overlap + 1], overlap=overlap, senses="+--+-")
    check(merger, overlap + 1, contigs, paths)


def test_a_contig_longer_than_a_tile(merger):
    contigs, paths = mcg.chains(7, 32, 2, [70001, 200, 70001], senses="-+")
    seqs = check(merger, 32, contigs, paths)
    assert len(seqs[0]) == 70001 + 200 + 70001 - 2 * 31


@pytest.mark.parametrize("edge", [63, 64, 65])
def test_segments_that_end_around_a_tile_edge(merger, edge):
    """with tiles of 64 bytes: the first contig's own bytes end at `edge`, where the consensus begins, in a path read forwards and one
    read backwards; then every length of the second contig moves the later seams across the next edges"""
    k = 25
    for second in range(k, k + 18):
        contigs, paths = mcg.chains(edge * 100 + second, k, 2, [edge + k - 1, second, 90], senses="+-+-")
        check(merger, k, contigs, paths, tile=64)


@pytest.mark.parametrize("batch", [1, 2, 7])
def test_batches_of_a_few_paths(merger, batch):
    contigs, paths = mcg.chains(batch, 25, 15, lambda p: [30 + p, 26, 40])
    check(merger, 25, contigs, paths, tile=64, batch=batch)


def test_the_same_call_twice_on_one_handle():
    m = api.PathMerge()
    try:
        contigs, paths = mcg.chains(3, 25, 20, [50, 31, 44])
        first = check(m, 25, contigs, paths)
        assert check(m, 25, contigs, paths) == first
    finally:
        m.close()


@pytest.mark.parametrize("tile,batch", [(16, 1 << 20), (64, 3), (16384, 1 << 20)])
def test_dirty_paths_equal_the_restatement(merger, tile, batch):
    """257 paths of 2 to 8 nodes in either sense: overlaps of 1 to 90 that differ within a path, nodes that are all window, lower
    case, N and codes in heads and bodies, gaps around k - 1.  Every junction has a consensus, so none goes to the host."""
    assert not mcg.dirty_sets()["dirty"]["flagged"]
    check_set(merger, "dirty", tile, batch)


@pytest.mark.parametrize("batch", [1 << 20, 7])
def test_dirty_paths_with_planned_conflicts(merger, batch):
    """the same kind of path, four of forty with one pair that has no consensus: in the first junction's first position, and in later
    junctions of longer paths"""
    assert mcg.dirty_sets()["dirty.breaks"]["flagged"] == [0, 5, 11, 39]
    check_set(merger, "dirty.breaks", 64, batch)


def test_where_in_the_window_a_character_sits(merger):
    """two nodes, ACGT but for one character -- a lower-case base or an N in the tail, a superset code in the head -- at the ends of
    windows of 63, 64, 65, 128 and 129 and at positions 62, 63 and 64, where a wave's lanes start over"""
    s, want = mcg.dirty_sets()["window"], mcg.expected("window")
    seqs = check_set(merger, "window")
    assert not any(flagged for _, flagged, _ in want)
    for p, at, kind in s["marks"]:
        assert seqs[p][at] == want[p][0][at] and (chr(seqs[p][at]) in "ACGT") == (kind == "N"), (p, at, kind)


@pytest.mark.parametrize("batch", [1 << 20, 7])
@pytest.mark.parametrize("which", range(mcg.CONFLICT_SETS))
def test_a_conflict_flags_its_path_only(merger, which, batch):
    """130 paths of four nodes; those at 0, 31, 63, 64 and 129 have one pair without a consensus, at the window positions above, in
    the first, middle or last junction (mergecontigs_golden.CONFLICTS, five a set).  Those five are redone, the others come from the
    device as the restatement has them."""
    s = mcg.dirty_sets()["conflict.%d" % which]
    assert s["flagged"] == list(mcg.CONFLICT_AT)
    check_set(merger, "conflict.%d" % which, batch=batch)


@pytest.mark.parametrize("order,batch", [("mid", 1 << 20), ("first", 1 << 20), ("last", 1 << 20), ("mid", 1)])
def test_overlaps_at_the_ring(merger, order, batch):
    """paths [3000, ov, ov + 3, 2 ov + 7, 37] with ov = 1023, 1024 and 1025 among 20 small ones: a window that fills the ring, a
    last junction of 7 under a path's window of 1024, and a path the ring cannot hold, which alone is the host's, in the middle of
    the call, first and last"""
    s = mcg.dirty_sets()["ring." + order]
    assert len(s["host"]) == 1 and max(s["paths"][s["host"][0]][1]) == 1025 and not s["flagged"]
    assert sorted(max(ov) for _, ov in s["paths"])[-3:] == [1023, 1024, 1025]
    check_set(merger, "ring." + order, batch=batch)


def test_gaps_across_chunks_of_sixteen_bytes(merger):
    """[contig, gap n, contig] for n around 16 and around k = 25, the gap's first own byte at offsets 0, 1 and 15 of a chunk, with the
    smallest tile; and gaps joined by less than k - 1, which alone lay out an N run and an n run side by side"""
    seqs = check_set(merger, "gaps", tile=16)
    assert any(b"N" in seq for seq in seqs) and any(acgt(seq) < len(seq) for seq in seqs)
    seqs = check_set(merger, "gaps.short", tile=16)
    assert any(b"Nn" in seq for seq in seqs)
    check_set(merger, "gaps.short", tile=16384)


@pytest.mark.parametrize("tile", [16, 64])
def test_many_seams_in_one_chunk(merger, tile):
    """64 paths of 8 nodes of 1 to 5 characters joined by 1 to 3: several segments begin inside most chunks of sixteen bytes"""
    check_set(merger, "seams", tile=tile)


ADJ_CASES = [c for c in mcg.cases() if mcg.needs_device(c) and c["out"] and "-" not in c["argv"] and not any(a.endswith(".dot") for a in c["argv"])]


@pytest.mark.parametrize("case", [c for c in ADJ_CASES if c["family"] <= 4 and c["name"] != "consensus.nonsubset"], ids=lambda c: c["name"])
def test_no_path_of_the_first_four_families_goes_to_the_host(merger, case):
    """a condition: those families hold no junction without a consensus (test_mergecontigs_host.py shows the restatement flags none)"""
    k, contigs, paths = mcg.case_paths(case)
    merger.tune(tile=16384, batch=1 << 20)
    merger.set_contigs(contigs)
    before = merger.profile_get("mc_redone")[1]
    seqs, counts, redone, logs = merger.merge(k, [(nodes, ov) for _, nodes, ov in paths])
    assert merger.profile_get("mc_redone")[1] - before == 0 and not redone.any()
    fasta = dict(mcg.read_fasta(mcg.golden(case["out"])))
    assert [fasta[pid] for pid, _, _ in paths] == seqs


@pytest.mark.parametrize("case", [c for c in ADJ_CASES if c["family"] == 5 or c["name"] == "consensus.nonsubset"], ids=lambda c: c["name"])
def test_the_redo_family_goes_to_the_host_path_by_path(merger, case):
    k, contigs, paths = mcg.case_paths(case)
    verbose = sum(a.count("v") if a.startswith("-v") else a == "--verbose" for a in case["argv"])
    merger.tune(tile=64, batch=2)
    merger.set_contigs(contigs)
    before = merger.profile_get("mc_redone")[1]
    seqs, counts, redone, logs = merger.merge(k, [(nodes, ov) for _, nodes, ov in paths], verbose=verbose)
    flagged = 0
    for i, (pid, nodes, ov) in enumerate(paths):
        seq, f, log = mcg.py_merge_path(contigs, k, nodes, ov, verbose, names=lambda u: "<%d>" % u)
        assert seqs[i] == seq and bool(redone[i]) == f, pid
        got = logs[i].replace("\x03", " ".join("<%d>" % u for u in nodes))
        for j, u in enumerate(nodes):
            got = got.replace("\x01%d\x02" % j, "<%d>" % u)
        assert got == log, pid
        flagged += f
    assert flagged > 0 and merger.profile_get("mc_redone")[1] - before == flagged


SMALL = {"ABG_MC_TILE": "64", "ABG_MC_BATCH": "1"}
SMALLEST = {"ABG_MC_TILE": "16", "ABG_MC_BATCH": "1"}
RUNS = [(c, {}) for c in mcg.cases() if mcg.needs_device(c) is not False] + [(c, SMALL) for c in mcg.cases() if mcg.needs_device(c)] + \
    [(c, SMALLEST) for c in mcg.cases() if mcg.needs_device(c)]


@pytest.mark.parametrize("case,env", RUNS, ids=lambda x: x["name"] if "name" in x else ("tile%s_batch%s" % (x["ABG_MC_TILE"], x["ABG_MC_BATCH"]) if x else "default"))
def test_binary_writes_what_the_reference_wrote(case, env, binary, tmp_path):
    mcg.check_case(case, mcg.run_case([binary], case, tmp_path, env=env))


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in mcg.cases() if c["name"] == "exact.k25")
    status, out, err, fa, graph = mcg.run_case([binary], case, tmp_path, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert status == 1 and out == b""
    assert err.splitlines()[-1] == "MergeContigs: error: no HIP device available (abyss_amd has no CPU fallback)"
