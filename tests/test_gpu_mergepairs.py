"""abyss-mergepairs on the GPU.  api.PairMerge.align (the kernel of abg_mp.hip, and the host's std::sort over the rows it spills) must
give mp_check's records -- the serial body of abg_mp.h, which the CPU suite holds to the reference's goldens and to a plain-Python
restatement -- on pairs of 0 to 200 bases a side, among them the stripes' seams, mixed case and IUPAC codes, and pairs that do not
overlap, whose answer hangs on the order of ties: at the default tuning, with ABG_MP_MAX_LEN=64 (the longer pairs are the host's),
with a spill arena of two rows (the rest go out again) and in batches of 7.  The same on long_pairs(), 201 to 512 bases a side,
which is where 2 x 250 and 2 x 300 lie: every pair of the lengths around the stripes' seams up to 512, related and unrelated pairs,
and pairs made so that the record is known (512 matches, an overlap that starts at row 507, containment, an inserted base, one
base against 512), with more than 255 matches, paths of 512 cells, starts in the last stripe and spilled rows of over 256 cells
counted so that they stay in.  The limit at the default max_len: 512 is the kernel's, 513 the host's, and so is a byte of 128 or
above in read 1.  An arena of exactly one row takes it, of one cell less leaves it to the host, and of two rows one of which fits
sends the other out again.  The binary must write every golden case (tests/golden/mergepairs, from the unmodified reference) byte
for byte, the long ones also with an arena of exactly 512 cells in batches of 7."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from abyss_amd import api, build
import mergepairs_golden as mpg

pytestmark = pytest.mark.gpu

SEAMS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 193, 200)
LONG_SEAMS = (1, 64, 255, 256, 257, 319, 320, 321, 448, 449, 511, 512)
ALPHABETS = ("ACGT", "ACGT", "ACGTacgtNn", "ACGTRYKMSWBDHVNacgtrykmswbdhvn")
M, P = 3, 0.75
HOST = api.PairMerge.HOST
DEPENDENT = api.PairMerge.ORDER_DEPENDENT
LONG_UNRELATED = range(144 + 200, 144 + 200 + 100)   # where long_pairs() holds its pairs that do not overlap


def short_pairs():
    rng = random.Random(31)
    out = []
    for la in SEAMS:
        for lb in SEAMS:
            out.append(mpg.random_pair(rng, la, lb, "ACGT", 0.02))
    for n in range(300):
        out.append(mpg.random_pair(rng, rng.randint(0, 200), rng.randint(0, 200), ALPHABETS[n % 4], 0.03))
    for n in range(200):  # no overlap: every score of the last row is negative, and ties decide
        out.append((mpg.random_read(rng, rng.randint(30, 120)), mpg.random_read(rng, rng.randint(30, 120))))
    return out


def long_pairs():
    """201 to 512 bases a side, all eight stripes and all eight lines of 64 columns, and the seams of both up to the kernel's limit"""
    rng = random.Random(32)
    out = []
    for la in LONG_SEAMS:
        for lb in LONG_SEAMS:
            out.append(mpg.random_pair(rng, la, lb, "ACGT", 0.02))
    for n in range(200):
        out.append(mpg.random_pair(rng, rng.randint(201, 512), rng.randint(201, 512), ALPHABETS[n % 4], 0.03))
    assert len(out) == LONG_UNRELATED.start
    for n in range(100):  # no overlap, and a last row of up to 512 cells for the host's sort
        out.append((mpg.random_read(rng, rng.randint(201, 512)), mpg.random_read(rng, rng.randint(201, 512))))
    out += [(a, b) for name, a, b, setting, record in mpg.constructed_long_pairs()]
    return out


PAIR_SETS = {"short": short_pairs, "long": long_pairs}


@functools.lru_cache(maxsize=None)
def pairs(name="short"):
    return tuple((a.encode(), b.encode()) for a, b in PAIR_SETS[name]())


def records_of(some, m, p):
    """mp_check's records of any pairs"""
    build.build_hostcheck()
    text = b"".join(b"%s %s\n" % (a or b"-", b or b"-") for a, b in some)
    r = subprocess.run([build.MP_CHECK, "align", str(m), repr(p)], input=text, stdout=subprocess.PIPE, check=True, timeout=120)
    return np.array([[int(x) for x in line.split()] for line in r.stdout.decode().splitlines()], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def want(m, p, name="short"):
    """mp_check's records of pairs(name), computed once a setting"""
    return records_of(pairs(name), m, p)


@pytest.fixture(scope="module")
def aligner():
    a = api.PairMerge()
    yield a
    a.close()


def compare(got, expect, some, host):
    """every field of every record; `host`: which pairs the host must have taken, by their lengths"""
    assert got.shape == expect.shape
    for k, (a, b) in enumerate(some):
        assert bool(got[k, 8] & HOST) == host(len(a), len(b)), (k, len(a), len(b))
        g = got[k].copy()
        g[8] &= ~np.uint32(HOST)
        assert g.tolist() == expect[k].tolist(), (k, len(a), len(b))


def check(al, which=None, m=M, p=P, host=lambda la, lb: False, name="short"):
    """align pairs(name)[which] and compare every field; `host`: which pairs the host must have taken"""
    idx = list(range(len(pairs(name)))) if which is None else list(which)
    some = [pairs(name)[i] for i in idx]
    got = al.align(some, min_matches=m, identity=p)
    compare(got, want(m, p, name)[idx], some, host)
    return got


def test_records_equal_the_serial_body(aligner):
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    aligner.profile_reset()
    got = check(aligner)
    dependent = int((got[:, 8] & api.PairMerge.ORDER_DEPENDENT).astype(bool).sum())
    assert dependent >= 5                                   # the pairs that do not overlap give some
    assert aligner.profile_get("mp_spilled")[1] == dependent and aligner.profile_get("mp_host")[1] == 0
    assert aligner.profile_get("mp_relaunched")[1] == 0 and aligner.profile_get("mp_launches")[1] == 1
    assert aligner.profile_get("mp_wave")[1] == 1
    assert int((got[:, 3] == 1).sum()) > 100 and int((got[:, 0] == 0).sum()) > 10


def test_records_at_the_default_options(aligner):
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    check(aligner, m=10, p=0.9)


def test_reads_past_max_len_are_the_hosts(monkeypatch):
    monkeypatch.setenv("ABG_MP_MAX_LEN", "64")
    al = api.PairMerge()
    try:
        al.profile_reset()
        check(al, host=lambda la, lb: la > 64 or lb > 64)
        assert al.profile_get("mp_host")[1] == sum(1 for a, b in pairs() if len(a) > 64 or len(b) > 64)
    finally:
        al.close()


def test_a_spill_arena_of_two_rows_sends_the_rest_out_again(aligner):
    aligner.tune(max_len=512, spill_bytes=2 * 120 * 16, batch=1 << 16)
    aligner.profile_reset()
    got = check(aligner)
    dependent = int((got[:, 8] & api.PairMerge.ORDER_DEPENDENT).astype(bool).sum())
    assert aligner.profile_get("mp_relaunched")[1] > 0 and aligner.profile_get("mp_launches")[1] >= 3
    assert aligner.profile_get("mp_spilled")[1] == dependent and aligner.profile_get("mp_host")[1] == 0   # 240 cells hold any one row
    aligner.tune(spill_bytes=64 << 20)


def test_an_arena_smaller_than_a_row_leaves_the_pair_to_the_host(aligner):
    aligner.tune(max_len=512, spill_bytes=16 * 16, batch=1 << 16)
    aligner.profile_reset()
    idx = list(range(len(pairs()) - 200, len(pairs())))
    got = aligner.align([pairs()[i] for i in idx], min_matches=M, identity=P)
    expect = want(M, P)[idx]
    dependent = (expect[:, 8] & api.PairMerge.ORDER_DEPENDENT).astype(bool)
    assert ((got[:, 8] & HOST).astype(bool) == dependent).all()   # every row there is 30 cells or more
    got[:, 8] &= ~np.uint32(HOST)
    assert got.tolist() == expect.tolist()
    assert aligner.profile_get("mp_host")[1] == int(dependent.sum()) > 0
    aligner.tune(spill_bytes=64 << 20)


def test_batches_of_seven(aligner):
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=7)
    aligner.profile_reset()
    check(aligner, which=range(300, 400))
    assert aligner.profile_get("mp_launches")[1] == 15
    aligner.tune(batch=1 << 16)


def test_a_byte_with_no_complement_is_refused(aligner):
    with pytest.raises(api.AbyssAmdError, match="complement"):
        aligner.align([(b"ACGT", b"ACXT")])


def test_no_pairs(aligner):
    assert aligner.align([]).shape == (0, 10)


# ---- 201 to 512 bases a side, and the limit

@pytest.mark.parametrize("m,p", [(M, P), (10, 0.9)])
def test_long_records_equal_the_serial_body(aligner, m, p):
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    aligner.profile_reset()
    got = check(aligner, m=m, p=p, name="long")
    assert aligner.profile_get("mp_host")[1] == 0 and aligner.profile_get("mp_relaunched")[1] == 0
    # what the long pairs are for: a count past a byte, a path or a start in the last stripe, a spilled row of more than four lines
    lb = np.array([len(b) for a, b in pairs("long")])
    dependent = (got[:, 8] & DEPENDENT).astype(bool)
    assert int((got[:, 7] > 255).sum()) >= 5
    assert int(((got[:, 6] == 512) | (got[:, 4] >= 448)).sum()) >= 5
    assert int((dependent & (lb > 256)).sum()) >= 5
    assert aligner.profile_get("mp_spilled")[1] == int(dependent.sum())


def test_the_constructed_pairs_give_the_records_they_were_made_for(aligner):
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    for name, a, b, setting, record in mpg.constructed_long_pairs():
        m, p = mpg.LONG_SETTINGS[setting]
        got = aligner.align([(a.encode(), b.encode())], min_matches=m, identity=p)
        assert tuple(got[0, :8].tolist()) == record, name


def test_long_rows_in_batches_of_seven_and_an_arena_of_two_rows(aligner):
    flags = want(M, P, "long")[:, 8]
    dependent = [i for i in range(len(flags)) if flags[i] & DEPENDENT]
    rest = [i for i in LONG_UNRELATED if not flags[i] & DEPENDENT]
    which = dependent + rest[:100 - len(dependent)]       # the first batch holds seven rows of 201 cells or more: over 1,024
    assert len(dependent) >= 7 and len(which) == 100
    aligner.tune(max_len=512, spill_bytes=2 * 512 * 16, batch=7)
    try:
        aligner.profile_reset()
        check(aligner, which=which, name="long")
        assert aligner.profile_get("mp_relaunched")[1] > 0 and aligner.profile_get("mp_host")[1] == 0
        assert aligner.profile_get("mp_spilled")[1] == len(dependent)
    finally:
        aligner.tune(spill_bytes=64 << 20, batch=1 << 16)


def test_the_limit_at_the_default_max_len(aligner):
    rng = random.Random(33)

    def overlapping(la, lb):
        """the two ends of a fragment: all but 2 bases of the shorter read overlap, and at most 300"""
        ov = min(la, lb, 302) - 2
        f = mpg.random_read(rng, la + lb - ov)
        return f[:la], mpg.reverse_complement(f[-lb:]), (1, 1, 1, 1, la - ov, ov - 1, ov, ov)

    some = [overlapping(rng.randint(20, 60), rng.randint(20, 60))]
    for la, lb in ((512, 512), (513, 10), (10, 513), (512, 513), (513, 513), (600, 600)):
        some += [overlapping(la, lb), overlapping(rng.randint(20, 60), rng.randint(20, 60))]
    made_for = [list(record) for a, b, record in some]
    some = [(a.encode(), b.encode()) for a, b, record in some]
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    aligner.profile_reset()
    got = aligner.align(some, min_matches=M, identity=P)
    compare(got, records_of(some, M, P), some, host=lambda la, lb: la > 512 or lb > 512)
    assert aligner.profile_get("mp_host")[1] == 5 == sum(1 for a, b in some if len(a) > 512 or len(b) > 512)
    assert got[:, :8].tolist() == made_for                # (8 matches pass -m3, and every overlap here is exact)


def test_a_byte_of_128_or_above_in_read_1_is_the_hosts(aligner):
    """read 1 does not go through the complement table, and a lane's four registers hold the match table's first 128 columns"""
    rng = random.Random(34)
    some = []
    for _ in range(3):  # the last 200 bases of read 1 are the first 200 of the other
        f = mpg.random_read(rng, 380)
        some.append((f[:300].encode(), mpg.reverse_complement(f[100:]).encode()))
    odd = bytearray(some[1][0])
    odd[250] = 200      # inside the overlap: it matches nothing
    with_odd = [some[0], (bytes(odd), some[1][1]), some[2]]
    aligner.tune(max_len=512, spill_bytes=64 << 20, batch=1 << 16)
    plain = aligner.align(some, min_matches=M, identity=P)
    aligner.profile_reset()
    got = aligner.align(with_odd, min_matches=M, identity=P)
    assert [bool(f & HOST) for f in got[:, 8]] == [False, True, False] and aligner.profile_get("mp_host")[1] == 1
    assert got[0].tolist() == plain[0].tolist() and got[2].tolist() == plain[2].tolist()
    got[1, 8] &= ~np.uint32(HOST)
    assert got.tolist() == records_of(with_odd, M, P).tolist()
    assert plain[1, :8].tolist() == [1, 1, 1, 1, 100, 199, 200, 200] and got[1, :8].tolist() == [1, 1, 1, 1, 100, 199, 200, 199]


def test_an_arena_that_fits_a_row_exactly(aligner):
    flags = want(M, P, "long")[:, 8]
    dependent = sorted((i for i in LONG_UNRELATED if flags[i] & DEPENDENT), key=lambda i: -len(pairs("long")[i][1]))
    assert len(dependent) >= 2
    one, two = dependent[0], dependent[1]                 # the two longest rows among them
    lb1, lb2 = len(pairs("long")[one][1]), len(pairs("long")[two][1])
    assert lb1 > 256 and lb2 > 256                        # more than four lines of 64 columns
    try:
        aligner.tune(max_len=512, spill_bytes=lb1 * 16, batch=1 << 16)
        aligner.profile_reset()
        check(aligner, which=[one], name="long")
        assert [aligner.profile_get(x)[1] for x in ("mp_spilled", "mp_relaunched", "mp_host")] == [1, 0, 0]
        aligner.tune(spill_bytes=(lb1 - 1) * 16)
        aligner.profile_reset()
        check(aligner, which=[one], name="long", host=lambda la, lb: True)
        assert [aligner.profile_get(x)[1] for x in ("mp_spilled", "mp_relaunched", "mp_host")] == [0, 0, 1]
        aligner.tune(spill_bytes=max(lb1, lb2) * 16)      # whichever wave claims its cells first, the other finds the arena full
        aligner.profile_reset()
        check(aligner, which=[one, two], name="long")
        assert [aligner.profile_get(x)[1] for x in ("mp_spilled", "mp_relaunched", "mp_host")] == [2, 1, 0]
    finally:
        aligner.tune(spill_bytes=64 << 20)


# ---- the binary against the goldens

@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-mergepairs")


SMALL = {"ABG_MP_MAX_LEN": "64", "ABG_MP_SPILL_BYTES": "3200", "ABG_MP_BATCH": "7"}   # the host's pairs, relaunches and seams at once
ROW = {"ABG_MP_SPILL_BYTES": str(512 * 16), "ABG_MP_BATCH": "7"}   # an arena of exactly the kernel's longest row, batches over both streams
RUNS = [(c, {}) for c in mpg.cases()] + [(c, SMALL) for c in mpg.cases() if c["name"].split(".")[0] in ("eq100", "seam", "apart", "codes", "bad", "unequal", "seam512")]
RUNS += [(c, ROW) for c in mpg.cases() if c["name"].split(".")[0] in ("seam512", "apart400")]


@pytest.mark.parametrize("case,env", RUNS, ids=lambda x: x["name"] if "name" in x else ("small" if x == SMALL else "row" if x else "default"))
def test_binary_writes_what_the_reference_wrote(case, env, binary, tmp_path):
    mpg.check_case(case, mpg.run_case([binary], case, tmp_path, env=env))
