"""abyss-mergepairs on the GPU.  api.PairMerge.align (the kernel of abg_mp.hip, and the host's std::sort over the rows it spills) must
give mp_check's records -- the serial body of abg_mp.h, which the CPU suite holds to the reference's goldens and to a plain-Python
restatement -- on pairs of 0 to 200 bases a side, among them the stripes' seams, mixed case and IUPAC codes, and pairs that do not
overlap, whose answer hangs on the order of ties: at the default tuning, with ABG_MP_MAX_LEN=64 (the longer pairs are the host's),
with a spill arena of two rows (the rest go out again) and in batches of 7.  The binary must write every golden case
(tests/golden/mergepairs, from the unmodified reference) byte for byte."""
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
ALPHABETS = ("ACGT", "ACGT", "ACGTacgtNn", "ACGTRYKMSWBDHVNacgtrykmswbdhvn")
M, P = 3, 0.75
HOST = api.PairMerge.HOST


@functools.lru_cache(maxsize=None)
def pairs():
    rng = random.Random(31)
    out = []
    for la in SEAMS:
        for lb in SEAMS:
            out.append(mpg.random_pair(rng, la, lb, "ACGT", 0.02))
    for n in range(300):
        out.append(mpg.random_pair(rng, rng.randint(0, 200), rng.randint(0, 200), ALPHABETS[n % 4], 0.03))
    for n in range(200):  # no overlap: every score of the last row is negative, and ties decide
        out.append((mpg.random_read(rng, rng.randint(30, 120)), mpg.random_read(rng, rng.randint(30, 120))))
    return tuple((a.encode(), b.encode()) for a, b in out)


@functools.lru_cache(maxsize=None)
def want(m, p):
    """mp_check's records of pairs(), computed once a setting"""
    build.build_hostcheck()
    text = b"".join(b"%s %s\n" % (a or b"-", b or b"-") for a, b in pairs())
    r = subprocess.run([build.MP_CHECK, "align", str(m), repr(p)], input=text, stdout=subprocess.PIPE, check=True, timeout=120)
    return np.array([[int(x) for x in line.split()] for line in r.stdout.decode().splitlines()], dtype=np.uint32)


@pytest.fixture(scope="module")
def aligner():
    a = api.PairMerge()
    yield a
    a.close()


def check(al, which=None, m=M, p=P, host=lambda la, lb: False):
    """align pairs()[which] and compare every field; `host`: which pairs the host must have taken"""
    idx = list(range(len(pairs()))) if which is None else list(which)
    got = al.align([pairs()[i] for i in idx], min_matches=m, identity=p)
    expect = want(m, p)[idx]
    assert got.shape == expect.shape
    for k, i in enumerate(idx):
        la, lb = len(pairs()[i][0]), len(pairs()[i][1])
        assert bool(got[k, 8] & HOST) == host(la, lb), (i, la, lb)
        g = got[k].copy()
        g[8] &= ~np.uint32(HOST)
        assert g.tolist() == expect[k].tolist(), (i, la, lb)
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


# ---- the binary against the goldens

@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-mergepairs")


SMALL = {"ABG_MP_MAX_LEN": "64", "ABG_MP_SPILL_BYTES": "3200", "ABG_MP_BATCH": "7"}   # the host's pairs, relaunches and seams at once
RUNS = [(c, {}) for c in mpg.cases()] + [(c, SMALL) for c in mpg.cases() if c["name"].split(".")[0] in ("eq100", "seam", "apart", "codes", "bad", "unequal")]


@pytest.mark.parametrize("case,env", RUNS, ids=lambda x: x["name"] if "name" in x else ("small" if x else "default"))
def test_binary_writes_what_the_reference_wrote(case, env, binary, tmp_path):
    mpg.check_case(case, mpg.run_case([binary], case, tmp_path, env=env))
