"""PopBubbles' alignment restated in plain Python, for the tests: alignGlobal with its three full matrices and the reference's own
backtrack over them (Align/alignGlobal.cc), alignPair / alignMulti (Align/alignGlobal.h:47-83) and ambiguityOr
(Common/Sequence.h:102-107, Sequence.cpp:141-204).  Nothing here knows about flags: the header's five bits a cell are checked
against the matrices themselves."""
from __future__ import annotations

import random

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND = 5, -4, -12, -4
NEG = -(2 ** 30)  # INT_MIN / 2

_MASK = {"A": 0x1, "B": 0xe, "C": 0x2, "D": 0xd, "G": 0x4, "H": 0xb, "K": 0xc, "M": 0x3, "N": 0xf, "R": 0x5, "S": 0x6, "T": 0x8,
         "V": 0x7, "W": 0x9, "Y": 0xa}
_UNMASK = "NACMGRSVTWYHKDBN"
CODES = "".join(sorted(_MASK))


def ambiguity_or(a: str, b: str) -> str:
    c = _UNMASK[_MASK[a.upper()] | _MASK[b.upper()]]
    return c.lower() if a.islower() or b.islower() else c


def score(a: str, b: str):
    """(score, consensus character)"""
    if a == b:
        return MATCH, a
    c = ambiguity_or(a, b)
    return (MATCH if c == a or c == b else MISMATCH), c


def align(seq_a: bytes, seq_b: bytes):
    """alignGlobal: (matches, consensus as bytes)"""
    a, b = seq_a.decode(), seq_b.decode()
    la, lb = len(a), len(b)
    f = [[0] * (lb + 1) for _ in range(la + 1)]
    g = [[0] * (lb + 1) for _ in range(la + 1)]
    h = [[0] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        f[i][0] = g[i][0] = 0 if i == 0 else GAP_OPEN + GAP_EXTEND * (i - 1)
        h[i][0] = NEG
    for j in range(lb + 1):
        f[0][j] = h[0][j] = 0 if j == 0 else GAP_OPEN + GAP_EXTEND * (j - 1)
        g[0][j] = NEG
    for i in range(1, la + 1):
        fi, gi, hi, fu, gu, ai = f[i], g[i], h[i], f[i - 1], g[i - 1], a[i - 1]
        for j in range(1, lb + 1):
            gi[j] = max(fu[j] + GAP_OPEN, gu[j] + GAP_EXTEND)
            hi[j] = max(fi[j - 1] + GAP_OPEN, hi[j - 1] + GAP_EXTEND)
            bj = b[j - 1]
            s = MATCH if ai == bj else score(ai, bj)[0]
            fi[j] = max(fu[j - 1] + s, gi[j], hi[j])
    cons = []
    matches = 0
    i, j = la, lb
    while i > 0 and j > 0:
        fij = f[i][j]
        s, c = score(a[i - 1], b[j - 1])
        if fij == f[i - 1][j - 1] + s:
            cons.append(c)
            if s == MATCH:
                matches += 1
            i -= 1
            j -= 1
        elif fij == f[i - 1][j] + GAP_OPEN or fij == g[i - 1][j] + GAP_EXTEND:
            while g[i][j] == g[i - 1][j] + GAP_EXTEND:
                cons.append(a[i - 1].lower())
                i -= 1
                assert i > 0
            assert g[i][j] == f[i - 1][j] + GAP_OPEN
            cons.append(a[i - 1].lower())
            i -= 1
        elif fij == f[i][j - 1] + GAP_OPEN or fij == h[i][j - 1] + GAP_EXTEND:
            while h[i][j] == h[i][j - 1] + GAP_EXTEND:
                cons.append(b[j - 1].lower())
                j -= 1
                assert j > 0
            assert h[i][j] == f[i][j - 1] + GAP_OPEN
            cons.append(b[j - 1].lower())
            j -= 1
        else:
            raise AssertionError("no way back from (%d, %d)" % (i, j))
    while i > 0:
        cons.append(a[i - 1].lower())
        i -= 1
    while j > 0:
        cons.append(b[j - 1].lower())
        j -= 1
    return matches, "".join(reversed(cons)).encode()


def align_group(seqs):
    """align(seqs) of alignGlobal.h: (matches, size, consensus).  alignMulti's matches is min(0, ...): 0."""
    if len(seqs) == 2:
        m, c = align(seqs[0], seqs[1])
        return m, len(c), c
    cur, matches = seqs[0], 0
    for s in seqs[1:]:
        m, cur = align(cur, s)
        matches = min(matches, m)
    return matches, len(cur), cur


def random_seq(rng: random.Random, n: int, alphabet: str = "ACGT") -> bytes:
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def mutate(rng: random.Random, s: bytes, rate: float = 0.08) -> bytes:
    """substitutions, insertions and deletions at `rate` a base"""
    out = []
    for ch in s.decode():
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
        elif r < rate:
            out.append(ch)
            out.append(rng.choice("ACGT"))
            continue
        else:
            out.append(ch)
    return "".join(out).encode() or b"A"


def host_cases(seed: int = 7):
    """the pairs pb_check and the GPU tests share: random, related, tied, IUPAC and mixed case, sides up to about 150"""
    rng = random.Random(seed)
    iupac = CODES + CODES.lower()
    pairs = []
    for la, lb in ((1, 1), (1, 2), (2, 1), (3, 7), (17, 16), (40, 33), (64, 65), (100, 150), (150, 97), (129, 128)):
        pairs.append((random_seq(rng, la), random_seq(rng, lb)))
        a = random_seq(rng, la)
        pairs.append((a, mutate(rng, a)))
        pairs.append((random_seq(rng, la, iupac), random_seq(rng, lb, iupac)))
        a = random_seq(rng, la, "ACGTacgtNRY")
        pairs.append((a, mutate(rng, a)))
    for n, m in ((1, 5), (5, 1), (30, 41), (70, 64), (64, 70), (120, 90)):
        pairs.append((b"A" * n, b"A" * m))                       # homopolymers: diagonal and gap scores tie
        pairs.append((b"AC" * (n // 2 + 1), b"AC" * (m // 2 + 1)))  # tandem repeats
        pairs.append((b"A" * n, b"C" * m))                       # nothing matches
    a = random_seq(rng, 90)
    ins = random_seq(rng, 45)
    pairs += [(a, a), (a, ins + a), (a, a + ins), (a, a[:45] + ins + a[45:]), (ins + a, a), (a[:45] + ins + a[45:], a), (a.lower(), a), (b"", a[:9]), (a[:9], b"")]
    return pairs


# ---- the goldens (tests/golden/popbubbles, written by tests/golden/make_popbubbles.py from the unmodified reference)

import functools  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402
import subprocess  # noqa: E402

import golden_archive  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_files, golden, cases = golden_archive.bind("popbubbles")


def rules():
    return json.load(open(os.path.join(HERE, "golden", "popbubbles_rules.json")))


def run_case(cmd, case, d, env=None):
    """(status, stdout, stderr, -g file) of cmd + argv in a directory that holds the inputs"""
    for name in case["inputs"]:
        (d / name).write_bytes(golden(name))
    e = dict(os.environ, **(env or {}))
    e.pop("COLUMNS", None)
    r = subprocess.run(list(cmd) + case["argv"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120, input=b"")
    return r.returncode, r.stdout, r.stderr.decode(), (d / "out.g").read_bytes() if (d / "out.g").exists() else None


def check_case(case, got):
    status, out, err, graph = got
    if case.get("refused"):  # colour-space contigs: the reference aligns them, this build says it does not
        assert status == 1 and "PopBubbles: error: " in err and any(i in err for i in case["inputs"]), (status, err)
        return
    if case.get("aborts"):  # the reference's lines up to its assert, then one line of the drop-in's own
        assert status == 1 and err.startswith(case["stderr"]), (status, err)
        rest = err[len(case["stderr"]):]
        assert rest.count("\n") == 1 and ("error: " in rest), rest
        return
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    err = "".join(re.sub(r"^\S*/(PopBubbles|pb_check): ", "PopBubbles: ", ln) for ln in err.splitlines(True))
    assert err == case["stderr"], (err, case["stderr"])
    assert status == case["status"]
    assert out == (golden(case["stdout"]) if case["stdout"] else b"")
    if graph is not None:  # (the SAM header holds the command line, argv[0] included)
        graph = re.sub(rb"\tCL:\S*/(PopBubbles|pb_check) ", b"\tCL:PopBubbles ", graph)
    assert graph == (golden(case["graph"]) if case["graph"] else None)


def groups_aligned(pb_check, case, d):
    """how many groups of branches the run hands to the aligner (pb_check counts them into the file PB_CHECK_GROUPS names); None
    when it hands over none"""
    count = d / "groups.count"
    run_case([pb_check, "run"], case, d, env={"PB_CHECK_GROUPS": str(count)})
    return int(count.read_text()) if count.exists() else None
