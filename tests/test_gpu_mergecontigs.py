"""MergeContigs on the GPU.  api.PathMerge.merge (the two kernels of abg_mc.hip) must equal the plain-Python restatement of
tests/mergecontigs_golden.py on generated sets that reach the seams of the kernels -- a wave of paths, a wave of overlap window, a
contig longer than a tile, segments that end around a tile's edge, batches of a few paths -- and must not hand a path to the host
unless a junction of it has no consensus.  The binary must write every golden case (tests/golden/mergecontigs, from the unmodified
reference) byte for byte, at the default tile and batch and at the smallest."""
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


def check(m, k, contigs, paths, tile=16384, batch=1 << 20):
    m.tune(tile=tile, batch=batch)
    m.set_contigs(contigs)
    before = m.profile_get("mc_redone")[1]
    seqs, counts, redone, logs = m.merge(k, paths)
    want = [mcg.py_merge_path(contigs, k, nodes, ov) for nodes, ov in paths]
    for i, (seq, flagged, log) in enumerate(want):
        assert seqs[i] == seq, i
        assert int(counts[i]) == acgt(seq), i
        assert bool(redone[i]) == flagged, i
    assert m.profile_get("mc_redone")[1] - before == sum(f for _, f, _ in want)
    return seqs


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
RUNS = [(c, {}) for c in mcg.cases() if mcg.needs_device(c) is not False] + [(c, SMALL) for c in mcg.cases() if mcg.needs_device(c)]


@pytest.mark.parametrize("case,env", RUNS, ids=lambda x: x["name"] if "name" in x else ("tile64_batch1" if x else "default"))
def test_binary_writes_what_the_reference_wrote(case, env, binary, tmp_path):
    mcg.check_case(case, mcg.run_case([binary], case, tmp_path, env=env))


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in mcg.cases() if c["name"] == "exact.k25")
    status, out, err, fa, graph = mcg.run_case([binary], case, tmp_path, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert status == 1 and out == b""
    assert err.splitlines()[-1] == "MergeContigs: error: no HIP device available (abyss_amd has no CPU fallback)"
