"""PopBubbles on the GPU.  api.BubbleAlign (the two kernels of abg_pb.hip) must give the matches, consensus length and consensus of the
plain-Python restatement of tests/popbubbles_golden.py -- alignGlobal with its full matrices and the reference's own backtrack -- on
pairs that put the seams of the wave kernel's stripes on both axes, on ties and long gap runs, on mixed case and IUPAC codes, on
numbers of pairs around a wave, on both sides of the limit between the two kernels, and with an arena so small that a call takes
many launches.  No pair goes to the host unless its flags fit no arena.  The binary must write every golden case
(tests/golden/popbubbles, from the unmodified reference) byte for byte at the default tuning and at the smallest arena."""
import functools
import os
import random

import pytest

from abyss_amd import api, build
import popbubbles_golden as pbg

pytestmark = pytest.mark.gpu

SIDES = (1, 2, 63, 64, 65, 127, 128, 129)
DEFAULT_ARENA = 4 << 30


@pytest.fixture(scope="module")
def aligner():
    a = api.BubbleAlign()
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def want(pairs):
    """the restatement's answer for a tuple of pairs, computed once"""
    out = []
    for a, b in pairs:
        m, c = pbg.align(a, b)
        out.append((m, len(c), c))
    return out


def check(al, pairs, arena=DEFAULT_ARENA, small_limit=16, batch=1 << 20, redone=()):
    """align with and without the consensus; `redone`: the pairs the host must take, none by default"""
    al.tune(arena_bytes=arena, small_limit=small_limit, batch=batch)
    before = al.profile_get("pb_redone")[1]
    matches, size, rd, cons = al.align(pairs, consensus=True)
    expect = want(tuple(pairs))
    for i, (m, n, c) in enumerate(expect):
        assert (int(matches[i]), int(size[i]), cons[i]) == (m, n, c), (i, len(pairs[i][0]), len(pairs[i][1]))
        assert bool(rd[i]) == (i in redone), i
    assert al.profile_get("pb_redone")[1] - before == len(redone)
    m2, s2, r2 = al.align(pairs)
    assert m2.tolist() == [e[0] for e in expect] and s2.tolist() == [e[1] for e in expect] and r2.tolist() == rd.tolist()


@functools.lru_cache(maxsize=None)
def side_pairs():
    rng = random.Random(11)
    pairs = []
    for la in SIDES:
        for lb in SIDES:
            a = pbg.random_seq(rng, la)
            # related where the lengths allow, so that the walk crosses the seams on a long diagonal with gaps, unrelated otherwise
            b = (pbg.mutate(rng, a) + pbg.random_seq(rng, lb))[:lb] if (la + lb) % 2 else pbg.random_seq(rng, lb)
            pairs.append((a, b))
    return tuple(pairs)


def test_side_lengths_around_the_stripes(aligner):
    check(aligner, list(side_pairs()))


def test_side_lengths_with_every_pair_on_a_wave(aligner):
    """small_limit 1: a 2 x 1 pair is the wave kernel's too"""
    check(aligner, list(side_pairs()), small_limit=1)


def test_ties_runs_case_and_codes(aligner):
    check(aligner, pbg.host_cases())
    check(aligner, pbg.host_cases(), small_limit=32)
    check(aligner, pbg.host_cases(), small_limit=1)


@functools.lru_cache(maxsize=None)
def tiny_pairs(n, seed):
    rng = random.Random(seed)
    return tuple((pbg.random_seq(rng, 1 + i % 3, "ACGTRYn"), pbg.random_seq(rng, 1 + (i // 3) % 3, "ACGTRYn")) for i in range(n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_numbers_of_tiny_pairs(aligner, n):
    check(aligner, list(tiny_pairs(n, n)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_numbers_of_pairs_with_long_ones_among_them(aligner, n):
    """sides of small_limit - 1, small_limit and small_limit + 1 and a few of some hundred between the tiny ones"""
    rng = random.Random(1000 + n)
    pairs = list(tiny_pairs(n, n))
    for at, (la, lb) in enumerate(((15, 15), (16, 16), (17, 17), (16, 17), (17, 1), (1, 17), (200, 190), (70, 300))):
        a = pbg.random_seq(rng, la)
        pairs[(at * 37) % n] = (a, (pbg.mutate(rng, a) + pbg.random_seq(rng, lb))[:lb])
    check(aligner, pairs)


def test_an_arena_of_a_few_thousand_bytes_takes_several_launches(aligner):
    pairs = list(side_pairs()) + list(tiny_pairs(65, 3))
    aligner.profile_reset()
    check(aligner, pairs, arena=129 * 132)   # the largest of them alone: 129 rows of 132 bytes
    assert aligner.profile_get("pb_launches")[1] >= 8
    check(aligner, pairs, batch=7)


def test_a_pair_larger_than_the_arena_is_the_hosts(aligner):
    pairs = list(tiny_pairs(65, 4))
    rng = random.Random(5)
    a = pbg.random_seq(rng, 40)
    pairs[33] = (a, pbg.mutate(rng, a))
    check(aligner, pairs, arena=64, redone=(33,))


@functools.lru_cache(maxsize=None)
def groups():
    rng = random.Random(21)
    out = []
    for n, length in ((3, 5), (4, 9), (3, 70), (4, 130), (2, 40), (3, 1), (4, 200)):
        base = pbg.random_seq(rng, length)
        out.append(tuple([base] + [pbg.mutate(rng, base, 0.15) for _ in range(n - 1)]))
    return tuple(out)


@pytest.mark.parametrize("arena", [DEFAULT_ARENA, 64 * 64, 64])
def test_chains_of_three_and_four_branches(aligner, arena):
    aligner.tune(arena_bytes=arena, small_limit=16, batch=1 << 20)
    before = aligner.profile_get("pb_redone")[1]
    matches, size, redone, cons = aligner.align_chain([list(g) for g in groups()])
    for i, g in enumerate(groups()):
        m, n, c = pbg.align_group(list(g))
        assert (int(matches[i]), int(size[i]), cons[i]) == (m, n, c), i
        assert m == 0 or len(g) == 2
    if arena == DEFAULT_ARENA:
        assert not redone.any() and aligner.profile_get("pb_redone")[1] == before
    elif arena == 64:
        assert redone.any()


def test_bytes_that_are_no_code_are_refused(aligner):
    with pytest.raises(api.AbyssAmdError, match="IUPAC"):
        aligner.align([(b"ACGT", b"AC0T")])
    with pytest.raises(api.AbyssAmdError, match="IUPAC"):
        aligner.align([(b"ACXT", b"ACGT")])


# ---- the binary against the goldens

@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "PopBubbles")


SMALLEST = {"ABG_PB_ARENA_BYTES": "4"}      # every pair of more than one row of four cells is the host's
SEAMS = {"ABG_PB_ARENA_BYTES": "8192"}      # several launches a call, the long pairs the host's
RUNS = [(c, {}) for c in pbg.cases()] + [(c, SMALLEST) for c in pbg.cases() if c["family"] != 7] + [(c, SEAMS) for c in pbg.cases() if c["family"] in (1, 4, 8)]


@pytest.mark.parametrize("case,env", RUNS, ids=lambda x: x["name"] if "name" in x else ("arena" + x["ABG_PB_ARENA_BYTES"] if x else "default"))
def test_binary_writes_what_the_reference_wrote(case, env, binary, tmp_path):
    pbg.check_case(case, pbg.run_case([binary], case, tmp_path, env=env))


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in pbg.cases() if c["name"] == "simple.k25")
    status, out, err, graph = pbg.run_case([binary], case, tmp_path, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert status == 1 and out == b""
    assert err.splitlines()[-1] == "PopBubbles: error: no HIP device available (abyss_amd has no CPU fallback)"
