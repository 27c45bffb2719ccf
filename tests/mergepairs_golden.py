"""abyss-mergepairs' alignment restated in plain Python, for the tests, and the loader of tests/golden/mergepairs.

The restatement is alignOverlap with its full matrices, its own Backtrack over the parent pointers and the reference's loop over the
sorted last row (Align/smith_waterman.cpp), then filterAlignments (Align/mergepairs.cc:162-205).  Nothing here carries values
forwards: the header's carried (matches, length, start, fail) are checked against the walk back itself.  The one thing it cannot
restate is where std::sort puts equal scores; align() reports the pairs whose answer depends on that, and the tests leave them out.
"""
from __future__ import annotations

import functools
import hashlib
import json
import os
import random
import re
import struct
import subprocess

import golden_archive

MATCH, MISMATCH, GAP = 1, -2, -10000
NEG = float("-inf")

_MASK = {"A": 0x1, "B": 0xe, "C": 0x2, "D": 0xd, "G": 0x4, "H": 0xb, "K": 0xc, "M": 0x3, "N": 0xf, "R": 0x5, "S": 0x6, "T": 0x8,
         "V": 0x7, "W": 0x9, "Y": 0xa}
_UNMASK = "NACMGRSVTWYHKDBN"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", ".": ".", "M": "K", "R": "Y", "W": "W", "S": "S", "Y": "R", "K": "M", "V": "B", "H": "D",
         "D": "H", "B": "V"}
CODES = "ACGTNMRWSYKVHDB"


def _islower(c: str) -> bool:
    return "a" <= c <= "z"


def _upper(c: str) -> str:
    return c.upper() if _islower(c) else c


def ambiguity_and(a: str, b: str) -> str:
    c = _UNMASK[_MASK.get(_upper(a), 0) & _MASK.get(_upper(b), 0)]
    return c.lower() if _islower(a) and _islower(b) else c


def is_match(a: str, b: str) -> bool:
    """isMatch, smith_waterman.cpp:65-80, on any two bytes (a byte that is no code has the empty mask here; the reference asserts)"""
    if a == b:
        return True
    if _upper(a) == _upper(b):
        return True
    if a in "Nn" or b in "Nn":
        return True
    both = ambiguity_and(a, b)
    return both == a or both == b


def reverse_complement(s: str) -> str:
    return "".join(_COMP[c.upper()].lower() if c.islower() else _COMP[c] for c in reversed(s))


def align(a: str, b: str, min_matches: int, identity: float):
    """read 1 against the reverse complement b of read 2: (n_aligned, n_matches, n_identity, n_gapless, survivor, order_dependent),
    survivor (t_pos, h_pos, length, matches) when n_gapless is 1.  identity: the float the option parses to, as a Python float."""
    na, nb = len(a), len(b)
    if na == 0 or nb == 0:
        return 0, 0, 0, 0, None, False
    H = [[0.0] * (nb + 1) for _ in range(na + 1)]
    P = [[None] * (nb + 1) for _ in range(na + 1)]
    V = [[False] * (nb + 1) for _ in range(na + 1)]
    for i in range(na + 1):
        V[i][0] = True
    for i in range(1, na + 1):
        for j in range(1, nb + 1):
            s = MATCH if is_match(a[i - 1], b[j - 1]) else MISMATCH
            scores = (H[i - 1][j - 1] + s if V[i - 1][j - 1] else NEG, H[i - 1][j] + GAP if V[i - 1][j] else NEG, H[i][j - 1] + GAP if V[i][j - 1] else NEG)
            best = max(range(3), key=lambda k: (scores[k], -k))
            H[i][j] = scores[best]
            P[i][j] = ((i - 1, j - 1), (i - 1, j), (i, j - 1))[best]
            V[i][j] = scores[best] != NEG

    def backtrack(j):
        ci, cj = na, j
        ni, nj = P[ci][cj]
        matches = length = 0
        while ni != 0 and nj != 0:
            if ni != ci and nj != cj and is_match(a[ci - 1], b[cj - 1]):
                matches += 1
            length += 1
            ci, cj = ni, nj
            ni, nj = P[ci][cj]
        if cj > 1:
            return None
        matches += is_match(a[ci - 1], b[cj - 1])
        length += 1
        return (ci - 1, j - 1, length, matches) if matches else None

    last = H[na]
    groups = {}
    for j in range(1, nb + 1):
        groups.setdefault(last[j], []).append(j)
    kept, found, stop, order_dependent = [], False, False, False
    scores = sorted(groups, reverse=True)
    for at, score in enumerate(scores):
        if score == 0 or stop:
            break
        done = [backtrack(j) for j in groups[score]]
        wins = [o for o in done if o]
        if not found and wins:
            found = True
            lower = at + 1 < len(scores)
            if len(wins) == 1 and lower:
                if len(done) == 1:
                    stop = True          # the early break
                else:
                    order_dependent = True
        kept += wins
    if order_dependent:
        return None, None, None, None, None, True
    n1 = len(kept)
    kept = [o for o in kept if o[3] >= min_matches]
    n2 = len(kept)
    kept = [o for o in kept if not (o[3] / o[2] < identity)]
    n3 = len(kept)
    kept = [o for o in kept if o[2] == na - o[0] and o[2] == o[1] + 1]
    return n1, n2, n3, len(kept), kept[0] if len(kept) == 1 else None, False


def float32(x: float) -> float:
    """what `float identity` holds, widened to double as the comparison does"""
    return struct.unpack("f", struct.pack("f", x))[0]


def random_read(rng: random.Random, n: int, alphabet: str = "ACGT") -> str:
    return "".join(rng.choice(alphabet) for _ in range(n))


def random_pair(rng: random.Random, la: int, lb: int, alphabet: str = "ACGT", rate: float = 0.03):
    """reads of la and lb bases from the ends of a fragment that makes them overlap more often than not, as the files hold them"""
    frag = random_read(rng, rng.randint(1, max(1, la + lb)), alphabet)
    one = (frag + random_read(rng, la, alphabet))[:la]
    two = (random_read(rng, lb, alphabet) + frag)[-lb:] if lb else ""

    def noisy(s):
        return "".join(rng.choice(alphabet) if rng.random() < rate else c for c in s)
    return noisy(one), reverse_complement(noisy(two))


LONG_SETTINGS = ((10, 0.9), (3, 0.75))


@functools.lru_cache(maxsize=None)
def constructed_long_pairs():
    """Pairs of up to 512 bases whose answer follows from how they are made: (name, read 1, read 2 as the file holds it, index into
    LONG_SETTINGS, the record's first eight fields there).  Each is one overlap that scores above every other column of the last
    row, so the reference breaks after it and n_aligned is 1."""
    rng = random.Random(512)
    f = random_read(rng, 512)
    out = [("identical", f, reverse_complement(f), 0, (1, 1, 1, 1, 0, 511, 512, 512))]
    # the last 5 bases of read 1 are the first 5 of the other: 5 matches are under -m10, so this one is for -m3
    core = random_read(rng, 5)
    out.append(("last5", random_read(rng, 507) + core, reverse_complement(core + random_read(rng, 295)), 1, (1, 1, 1, 1, 507, 4, 5, 5)))
    # read 2 inside read 1, ending where it ends; read 1 inside read 2, starting where it starts
    g = random_read(rng, 300)
    out.append(("two_in_one", random_read(rng, 212) + g, reverse_complement(g), 1, (1, 1, 1, 1, 212, 299, 300, 300)))
    h = random_read(rng, 300)
    out.append(("one_in_two", h, reverse_complement(h + random_read(rng, 212)), 0, (1, 1, 1, 1, 0, 299, 300, 300)))
    # One base more in the middle of an overlap of 400.  A gap costs 10,000, so the cell where the overlap would end keeps its
    # diagonal, half of which is out of step, and no column scores above chance.  The ends are chosen so that chance has one answer:
    # G against G in column 1 scores 1, and AAAG against GCCC keeps every column of 2 to 8 below that.  The break is taken after
    # column 1, whose one match -m10 drops: nothing is gapless, where without the inserted base 400 matches would be.
    c = "GCCC" + random_read(rng, 392) + "AAAG"
    out.append(("inserted", random_read(rng, 112) + c, reverse_complement(c[:200] + "ACGT"[("ACGT".index(c[200]) + 1) % 4] + c[200:] + random_read(rng, 111)), 0,
                (1, 0, 0, 0, 0, 0, 0, 0)))
    # one base against 512: the one cell that starts at column 1 matches, which is fewer matches than -m3 asks for
    s = random_read(rng, 512)
    out.append(("512x1", s, reverse_complement(s[-1]), 1, (1, 0, 0, 0, 0, 0, 0, 0)))
    out.append(("1x512", s[0], reverse_complement(s), 0, (1, 0, 0, 0, 0, 0, 0, 0)))
    return tuple(out)


# ---- the goldens (tests/golden/mergepairs, written by tests/golden/make_mergepairs.py from the unmodified reference)

HERE = os.path.dirname(os.path.abspath(__file__))
SUFFIXES = ("_merged.fastq", "_reads_1.fastq", "_reads_2.fastq")
STATS = re.compile(r"total=(\d+) merged=(\d+) unmerged=(\d+) unchaste=(\d+)\nno_alignment=(\d+) too_many_aligns=(\d+) too_few_matches=(\d+) has_indel=(\d+) low_pid=(\d+)\n")
STAT_NAMES = ("total", "merged", "unmerged", "unchaste", "no_alignment", "too_many_aligns", "too_few_matches", "has_indel", "low_pid")


_files, golden, cases = golden_archive.bind("mergepairs")


def needs_no_device(case):
    """no pair of the run reaches the device: option errors, missing and empty files, -1 / -2 beyond the first read, and -vvv, whose
    alignments the host prints pair by pair"""
    name = case["name"]
    return name.startswith(("error.", "empty.", "out.vvv", "casava.long_length1")) or name.endswith("_beyond_the_read")


def stderr_of(case):
    return golden(case["stderr"]).decode() if case["stderr"] else ""


def stats(case):
    m = STATS.search(stderr_of(case))
    return dict(zip(STAT_NAMES, map(int, m.groups()))) if m else None


def run_case(cmd, case, d, env=None):
    """(status, stdout, stderr, {suffix: bytes}) of cmd + argv in a directory that holds the inputs"""
    for name in case["inputs"]:
        (d / name).write_bytes(golden(name))
    for sub in case["dirs"]:
        (d / sub).mkdir(parents=True, exist_ok=True)
    e = dict(os.environ, **(env or {}))
    r = subprocess.run(list(cmd) + case["argv"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120, input=b"")
    files = {s: (d / (case["prefix"] + s)).read_bytes() for s in SUFFIXES if (d / (case["prefix"] + s)).exists()}
    return r.returncode, r.stdout, r.stderr.decode(), files


def check_case(case, got):
    status, out, err, files = got
    want_err = stderr_of(case)
    if case.get("aborts"):  # the reference's lines up to its assert or its exception, then one line of the drop-in's own
        assert status == 1 and err.startswith(want_err), (status, err)
        rest = err[len(want_err):]
        assert rest.count("\n") == 1 and rest.startswith("abyss-mergepairs: error: "), rest
        return
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    err = "".join(re.sub(r"^\S*/(abyss-mergepairs|mp_check): ", "abyss-mergepairs: ", ln) for ln in err.splitlines(True))
    assert err == want_err, (err[-400:], want_err[-400:])
    assert status == case["status"]
    assert out == (golden(case["stdout"]) if case["stdout"] else b"")
    assert sorted(files) == sorted(case["outputs"])
    for suffix, want in case["outputs"].items():
        assert (len(files[suffix]), hashlib.sha256(files[suffix]).hexdigest()) == (want["bytes"], want["sha256"]), suffix
