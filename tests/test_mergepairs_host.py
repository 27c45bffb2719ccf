"""abyss-mergepairs without a GPU.  mp_check (mergepairs_core.h over the serial body of abg_mp.h, the text the kernel compiles) must
write every golden case of tests/golden/mergepairs (from the unmodified reference) byte for byte, among them 2 x 250 and 2 x 300,
every pair of the lengths 1 to 600 around the kernel's limit of 512 (seam512) and unrelated pairs of 300 to 512 (apart400); the
serial body must equal the plain-Python restatement of alignOverlap and filterAlignments (tests/mergepairs_golden.py) on random
pairs of 0 to 14 bases and on 48 pairs of 201 to 512, seven of them constructed so that their record is known; the match table
must equal the restated isMatch on every pair of bytes, and the identity table the comparison itself up to the 1,024 entries the
device holds; and the binary, with no device to be seen, must still write every case that
aligns nothing on the device and say that it has no device where a case does."""
import functools
import os
import random
import subprocess

import pytest

from abyss_amd import build
import mergepairs_golden as mpg

NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


@pytest.fixture(scope="module")
def mp_check():
    build.build_hostcheck()
    return build.MP_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-mergepairs")


@pytest.mark.parametrize("case", mpg.cases(), ids=lambda c: c["name"])
def test_mp_check_writes_what_the_reference_wrote(case, mp_check, tmp_path):
    mpg.check_case(case, mpg.run_case([mp_check, "run"], case, tmp_path))


def test_the_cases_reach_every_statistic():
    seen = {name: 0 for name in mpg.STAT_NAMES}
    for case in mpg.cases():
        for name, value in (mpg.stats(case) or {}).items():
            seen[name] += value
    for name in ("merged", "unmerged", "unchaste", "no_alignment", "too_many_aligns", "too_few_matches", "has_indel", "low_pid"):
        assert seen[name] > 0, name
    assert any(c.get("aborts") for c in mpg.cases()) and any(c["status"] == 1 and not c.get("aborts") for c in mpg.cases())


def test_the_cases_hold_order_dependent_pairs_and_both_ends_of_the_early_break(mp_check, tmp_path):
    """the host body counts them; the golden outputs of those pairs came from the reference's std::sort"""
    total = [0, 0, 0, 0]
    for name in ("eq100.default", "lt.m0_p0", "gt.m0_p0", "apart.default", "seam.default", "codes.no_trim"):
        case = next(c for c in mpg.cases() if c["name"] == name)
        d = tmp_path / name
        d.mkdir()
        counts = d / "counts"
        mpg.check_case(case, mpg.run_case([mp_check, "run"], case, d, env={"MP_CHECK_COUNTS": str(counts)}))
        for k, v in enumerate(counts.read_text().split()):
            total[k] += int(v)
    pairs, order_dependent, taken, not_taken = total
    assert pairs > 1000 and order_dependent >= 20 and taken > 0 and not_taken > 0, total


def test_the_long_cases_hold_order_dependent_pairs_too(mp_check, tmp_path):
    """rows of 250 to 512 columns whose golden outputs came from the reference's std::sort"""
    total = [0, 0, 0, 0]
    for name in ("eq250.default", "eq300.default", "seam512.default", "apart400.default"):
        case = next(c for c in mpg.cases() if c["name"] == name)
        d = tmp_path / name
        d.mkdir()
        counts = d / "counts"
        mpg.check_case(case, mpg.run_case([mp_check, "run"], case, d, env={"MP_CHECK_COUNTS": str(counts)}))
        for k, v in enumerate(counts.read_text().split()):
            total[k] += int(v)
    pairs, order_dependent, taken, not_taken = total
    assert pairs == 301 and order_dependent >= 5 and taken > 0 and not_taken > 0, total


SETTINGS = ((10, 0.9), (0, 0.0), (1, 0.5), (3, 0.75))
ALPHABETS = ("ACGT", "AC", "ACGTacgtNn", "ACGTRYKMSWBDHVNacgtrykmswbdhvn")


@functools.lru_cache(maxsize=None)
def small_pairs(seed):
    rng = random.Random(seed)
    pairs = []
    for n in range(800):
        alphabet = ALPHABETS[n % len(ALPHABETS)]
        la, lb = rng.randint(0, 14), rng.randint(0, 14)
        if n % 3 == 0:
            pairs.append((mpg.random_read(rng, la, alphabet), mpg.random_read(rng, lb, alphabet)))
        else:
            pairs.append(mpg.random_pair(rng, la, lb, alphabet, 0.1))
    return tuple(pairs)


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_serial_body_equals_the_restatement(setting, mp_check):
    m, p = SETTINGS[setting]
    pairs = small_pairs(setting)
    text = "".join("%s %s\n" % (a or "-", b or "-") for a, b in pairs)
    r = subprocess.run([mp_check, "align", str(m), repr(p)], input=text.encode(), stdout=subprocess.PIPE, check=True, timeout=120)
    got = [tuple(map(int, line.split())) for line in r.stdout.decode().splitlines()]
    assert len(got) == len(pairs)
    compared = 0
    for (a, b), rec in zip(pairs, got):
        n1, n2, n3, n4, left, order_dependent = mpg.align(a, mpg.reverse_complement(b), m, mpg.float32(p))
        assert bool(rec[8] & 1) == order_dependent, (a, b)
        if order_dependent:
            continue
        assert rec[:4] == (n1, n2, n3, n4), (a, b, rec)
        assert rec[4:8] == (left if left else (0, 0, 0, 0)), (a, b, rec)
        compared += 1
    assert compared > 700


LONG_SEAMS = (201, 255, 256, 257, 320, 384, 385, 448, 511, 512)


@functools.lru_cache(maxsize=None)
def long_pairs():
    """(read 1, read 2, index into mpg.LONG_SETTINGS, the record expected or None): 48 pairs at the lengths the kernel takes and the
    short test does not reach, the settings dealt out in turn"""
    rng = random.Random(2)
    out = []
    for n in range(35):
        a, b = mpg.random_pair(rng, rng.choice(LONG_SEAMS), rng.choice(LONG_SEAMS), ALPHABETS[n % len(ALPHABETS)], 0.02)
        out.append((a, b, n % 2, None))
    for n in range(6):
        out.append((mpg.random_read(rng, rng.choice(LONG_SEAMS)), mpg.random_read(rng, rng.choice(LONG_SEAMS)), n % 2, None))
    out += [(a, b, s, rec) for name, a, b, s, rec in mpg.constructed_long_pairs()]
    return tuple(out)


def test_serial_body_equals_the_restatement_on_long_reads(mp_check):
    """201 to 512 bases a side: more than 255 matches, paths of 512 cells, starts in the fifth to eighth stripe.  The carried
    (matches, length, start, fail) against the walk back through the full matrix, which is what takes the time here."""
    pairs = long_pairs()
    assert len(pairs) == 48
    got = []
    for s, (m, p) in enumerate(mpg.LONG_SETTINGS):
        text = "".join("%s %s\n" % (a, b) for a, b, at, rec in pairs if at == s)
        r = subprocess.run([mp_check, "align", str(m), repr(p)], input=text.encode(), stdout=subprocess.PIPE, check=True, timeout=120)
        got.append(iter([tuple(map(int, line.split())) for line in r.stdout.decode().splitlines()]))
    compared = 0
    for a, b, s, expected in pairs:
        m, p = mpg.LONG_SETTINGS[s]
        rec = next(got[s])
        n1, n2, n3, n4, left, order_dependent = mpg.align(a, mpg.reverse_complement(b), m, mpg.float32(p))
        assert bool(rec[8] & 1) == order_dependent, (a, b)
        assert not (expected and order_dependent), (a, b)          # every constructed pair is compared
        if order_dependent:
            continue
        assert rec[:4] == (n1, n2, n3, n4), (a, b, rec)
        assert rec[4:8] == (left if left else (0, 0, 0, 0)), (a, b, rec)
        if expected:
            assert rec[:8] == expected, (a, b, rec)
        compared += 1
    assert all(next(g, None) is None for g in got)
    assert compared * 6 >= len(pairs) * 5, compared


def test_match_table_is_the_restated_is_match(mp_check):
    r = subprocess.run([mp_check, "table"], stdout=subprocess.PIPE, check=True, timeout=120)
    rows = r.stdout.decode().split()
    assert len(rows) == 256 and all(len(row) == 256 for row in rows)
    for a in range(256):
        want = "".join("1" if mpg.is_match(chr(a), chr(b)) else "0" for b in range(256))
        assert rows[a] == want, a
    # the asymmetric pairs: ambiguityAnd (Common/Sequence.h:94-99) is lower case only when both are, so the intersection 'A' of
    # ('r', 'A') is its second character, and that of ('R', 'a') is neither
    assert rows[ord("r")][ord("A")] == "1" and rows[ord("R")][ord("a")] == "0"
    assert rows[ord("A")][ord("r")] == "1" and rows[ord("a")][ord("R")] == "0"


def test_identity_table_is_the_comparison_itself(mp_check):
    for p in (0.9, 0.5, 0.75, 0.3, 0.0, 1.0):
        r = subprocess.run([mp_check, "identity", repr(p), "1024"], stdout=subprocess.PIPE, check=True, timeout=120)   # the device's table
        table = [int(x) for x in r.stdout.split()]
        assert len(table) == 1024
        f = mpg.float32(p)
        for L, least in enumerate(table, 1):
            assert all((m / L < f) == (m < least) for m in range(L + 1)), (p, L, least)


@pytest.mark.parametrize("case", [c for c in mpg.cases() if mpg.needs_no_device(c)], ids=lambda c: c["name"])
def test_binary_needs_no_device_where_nothing_is_aligned_on_it(case, binary, tmp_path):
    mpg.check_case(case, mpg.run_case([binary], case, tmp_path, env=NO_DEVICE))


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in mpg.cases() if c["name"] == "eq100.default")
    status, out, err, files = mpg.run_case([binary], case, tmp_path, env=NO_DEVICE)
    assert status == 1 and out == b""
    assert err.splitlines()[-1] == "abyss-mergepairs: error: no HIP device available (abyss_amd has no CPU fallback)"
