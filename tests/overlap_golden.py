"""Shared by the Overlap tests: the goldens of tests/golden/overlap (made by tests/golden/make_overlap.py from the unmodified
reference), pair files of tests/hostcheck/ov_check, the small shapes of the search tests and a plain-Python restatement of the search
(Overlap/Overlap.cpp:159-166) that owes nothing to abg_ov.h."""
import functools
import json
import os
import random
import re
import struct
import subprocess

import numpy as np

import golden_archive

HERE = os.path.dirname(os.path.abspath(__file__))
COMPLEMENT = str.maketrans("ACGTN.MRWSYKVHDBacgtnmrwsykvhdb", "TGCAN.KYWSRMBDHVtgcankywsrmbdhv")  # Common/Sequence.cpp:21-45


def revcomp(s):
    return s[::-1].translate(COMPLEMENT)


def py_find(t, h):
    """every l for which the last l characters of t are the first l of h, descending"""
    return [l for l in range(min(len(t), len(h)), 0, -1) if t[-l:] == h[:l]]


# ---- the goldens

_files, golden, cases = golden_archive.bind("overlap")


def rules():
    return json.load(open(os.path.join(HERE, "golden", "overlap_rules.json")))


def needs_device(case):
    """whether a pair reaches findOverlap in this run (counted by the generator from the reference's own -v lines)"""
    return case.get("searched", 0) > 0


def run_case(prefix, case, tmp, env=None):
    """runs `prefix + argv` in tmp as the generator ran the reference: (status, stdout, stderr, -o file or None, -g file or None)"""
    tmp = str(tmp)
    for name in case["inputs"]:
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(golden(name))
    e = dict(os.environ)
    e.pop("COLUMNS", None)
    e.update(env or {})
    r = subprocess.run(list(prefix) + list(case["argv"]), cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    written = []
    for f in ("out.fa", "out.g", "x.fa"):
        p = os.path.join(tmp, f)
        written.append(open(p, "rb").read() if os.path.exists(p) else None)
        if os.path.exists(p):
            os.remove(p)
    return r.returncode, r.stdout, r.stderr.decode(), written[0], written[1]


def check_case(case, got, prefix):
    """every byte of stdout, the -o and -g files, stderr and the status against what the reference wrote; `prefix` is what was run
    in place of `Overlap` (a SAM graph names its command line)"""
    status, out, err, fa, g = got
    assert status == case["status"], err
    want_out = golden(case["stdout"]) if case["stdout"] else case["stdout_text"].encode()
    assert out == want_out
    if case["status"] == 0:
        assert fa == (golden(case["out_fa"]) if case["out_fa"] else None)
        want_g = golden(case["out_g"]) if case["out_g"] else None
        if want_g is not None and want_g.startswith(b"@HD"):
            want_g = want_g.replace(b"\tCL:Overlap ", b"\tCL:" + prefix[0].encode() + b" ", 1)
        assert g == want_g
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    assert [re.sub(r"^\S*/(Overlap|ov_check): ", "Overlap: ", ln) for ln in err.splitlines()] == case["stderr"].splitlines()


# ---- pair files (tests/hostcheck/ov_check.cc): u64 ncontigs, u64 offsets[n + 1], bytes, u64 npairs, {u32 t, h}[npairs]; the result
# file: per pair u32 top[3], u32 ntop, u32 nall, u32 all[nall]

def write_pairs(path, contigs, pairs):
    data = b"".join(contigs)
    off = np.zeros(len(contigs) + 1, dtype="<u8")
    np.cumsum([len(c) for c in contigs], out=off[1:])
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(contigs)))
        f.write(off.tobytes())
        f.write(data)
        f.write(struct.pack("<Q", len(pairs)))
        f.write(np.asarray(pairs, dtype="<u4").reshape(-1, 2).tobytes())


def read_results(path, npairs):
    b = np.fromfile(path, dtype="<u4")
    at, out = 0, []
    for _ in range(npairs):
        top, ntop, nall = b[at:at + 3].tolist(), int(b[at + 3]), int(b[at + 4])
        out.append((top, ntop, b[at + 5:at + 5 + nall].tolist()))
        at += 5 + nall
    assert at == len(b)
    return out


# ---- the small shapes

MIN_LENGTHS = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257, 4097]


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _other(c, *more):
    return [x for x in "ACGT" if x != c and x not in more][0]


class Group:
    """contigs and oriented pairs; add(T, H) stores T and H so that the pair's nodes read T and H in the senses asked for"""

    def __init__(self, name):
        self.name, self.contigs, self.pairs, self.labels, self.claims = name, [], [], [], []

    def add(self, label, t, h, st=0, sh=0, claim=None):
        self.contigs.append(revcomp(t) if st else t)
        self.contigs.append(revcomp(h) if sh else h)
        n = len(self.contigs)
        self.pairs.append((2 * (n - 2) + st, 2 * (n - 1) + sh))
        self.labels.append(label)
        self.claims.append(claim)

    def oriented(self, node):
        s = self.contigs[node >> 1].upper()
        return revcomp(s) if node & 1 else s

    def expected(self):
        return [py_find(self.oriented(t), self.oriented(h)) for t, h in self.pairs]

    def raw(self):
        return [c.encode() for c in self.contigs]

    def folded(self):
        return [c.upper().encode() for c in self.contigs]


def _periodic(rng, p, n):
    """n characters of smallest period exactly p"""
    while True:
        u = _rand(rng, p)
        w = (u * (n // p + 1))[:n]
        if py_find(w, w) == list(range(n, 0, -p)):  # (no border by chance)
            return w


@functools.lru_cache(maxsize=None)
def small_shapes():
    rng = random.Random(20261019)
    groups = []
    senses = [(0, 0), (0, 1), (1, 0), (1, 1)]

    g = Group("lengths")
    for i, m in enumerate(MIN_LENGTHS):
        st, sh = senses[i % 4]
        w = _rand(rng, m)
        g.add("whole_t_%d" % m, w, w + _rand(rng, 13), st, sh, claim=("has", m))             # |t| = m: all of t is a prefix of h
        g.add("whole_h_%d" % m, _rand(rng, 11) + w, w, sh, st, claim=("has", m))             # |h| = m: all of h is a suffix of t
        g.add("t_long_%d" % m, _rand(rng, 5000) + w, w, st, 1 - sh, claim=("min", m))        # |t| >> |h|
        g.add("h_long_%d" % m, w, w + _rand(rng, 5000), 1 - st, sh, claim=("min", m))        # |h| >> |t|
        a = _rand(rng, m)
        g.add("none_%d" % m, a, _other(a[-1]) + _rand(rng, m - 1), st, sh, claim=("min", m))  # the same lengths, (almost surely) no match
    groups.append(g)

    g = Group("sets")
    a = "ACCGTTGACA" * 5
    g.add("no_match", a[:-1] + "A", "C" + "G" * 40, 0, 0, claim=("is", []))
    g.add("single_1", _rand(rng, 50) + "GA", "ACC" + "CT" * 20, 0, 1, claim=("is", [1]))
    for i, (nt, nh) in enumerate(((130, 70), (70, 130), (64, 64), (65, 200))):
        st, sh = senses[i]
        m = min(nt, nh)
        g.add("homopolymer_%d_%d" % (nt, nh), "A" * nt, "A" * nh, st, sh, claim=("is", list(range(m, 0, -1))))           # every l matches
        g.add("homopolymer_ends_%d_%d" % (nt, nh), "G" + "A" * (nt - 1), "A" * (nh - 1) + "G", sh, st, claim=("is", list(range(m - 1, 0, -1))))
    for i, (p, n) in enumerate(((2, 90), (3, 100), (7, 150), (7, 64), (3, 4097))):
        st, sh = senses[(i + 1) % 4]
        w = _periodic(rng, p, n)
        g.add("period_%d_%d" % (p, n), _rand(rng, 20) + _other(w[p - 1]) + w, w + _other(w[n - p]) + _rand(rng, 20), st, sh, claim=("step", p, n))
    # exactly two matches; matches on both sides of a 64-candidate step
    for i, m in enumerate((64, 65)):  # l = m and l = 1: for m = 65 the second is the only candidate of the second step
        st, sh = senses[i + 1]
        while True:
            w = _rand(rng, m - 1)
            w = w + w[0]
            if py_find(w, w) == [m, 1]:
                break
        g.add("ends_%d" % m, w, w + _other(w[1]) + _rand(rng, 30), st, sh, claim=("is", [m, 1]))
    while True:
        u = _rand(rng, 63)
        u = u + u[0]
        if py_find(u + u, u + u) == [128, 64, 1]:
            break
    g.add("two_steps_128_64_1", u + u, u + u + _other(u[1]) + _rand(rng, 9), 1, 1, claim=("is", [128, 64, 1]))
    # more than three matches, the third and fourth in a later step than the first (top mode stops before the end)
    for i, (p, n) in enumerate(((40, 130), (60, 200), (64, 300))):
        st, sh = senses[i]
        w = _periodic(rng, p, n)
        g.add("four_across_steps_%d_%d" % (p, n), _other(w[p - 1]) + w, w + _other(w[n - p]) + _rand(rng, 5), st, sh, claim=("across", p, n))
    groups.append(g)

    g = Group("mismatch")
    for n in (40, 100, 129):
        for i, q in enumerate((0, 7, 8, 9, n - 1)):
            st, sh = senses[i % 4]
            w = _rand(rng, n)
            bad = w[:q] + _other(w[q]) + w[q + 1:]
            g.add("only_at_%d_of_%d" % (q, n), w, bad, st, sh, claim=("one_off", n, q))   # |t| = |h| = n: the candidate l = n differs in byte q alone
            g.add("only_at_%d_of_%d_in_t" % (q, n), _rand(rng, 3) + bad, w + _rand(rng, 5), sh, st, claim=("one_off", n, q))
    groups.append(g)

    g = Group("bytes")
    codes = "NMRWSYKVHDB."
    for i, (st, sh) in enumerate(senses):
        w = "".join(rng.choice("ACGT" + codes) for _ in range(37)) + codes
        g.add("codes_equal_themselves_%d%d" % (st, sh), _rand(rng, 9) + w, w + _rand(rng, 9), st, sh, claim=("has", len(w)))
        v = _rand(rng, 30)
        g.add("n_is_not_a_%d%d" % (st, sh), v[:10] + "N" + v[11:], v[:10] + "A" + v[11:] + "C", st, sh, claim=("lacks", 30))
        g.add("r_is_not_y_%d%d" % (st, sh), v[:29] + "R", v[:29] + "Y" + "T", st, sh, claim=("lacks", 30))
        lw = _rand(rng, 25)
        g.add("lower_case_%d%d" % (st, sh), (_rand(rng, 4) + lw).lower(), lw[:12] + lw[12:].lower() + "ACG", st, sh, claim=("has", 25))
    groups.append(g)

    # placement: h is the first contig of the store and t the last, so the byte before h and the byte after t are not theirs.
    # The store is the contigs end to end and then their reverse complements; the byte after t is the first byte of the reverse
    # complement of contig 0, the complement of h's last byte.
    for which in ("late_t", "long_l", "early_t"):
        g = Group("placement_" + which)
        y = _rand(rng, 40)
        filler = [_rand(rng, 17), _rand(rng, 8)]
        if which == "late_t":
            # reading t one byte late at l = 21 would see t[-20:] + (the byte after t) == h[:21]: a match that is not there
            t = _rand(rng, 60)
            after = revcomp(y[-1])
            h = t[-20:] + after + y
            claim = ("trap", "late_t", 21)
        elif which == "long_l":
            # a candidate l = |h| + 1 would compare h + (the first byte of the next contig) with t's last |h| + 1 bytes: equal
            h = _rand(rng, 23)
            t = _rand(rng, 30) + h + filler[0][0]
            claim = ("trap", "long_l", len(h) + 1)
        else:
            # reading t one byte early at l = 20: t[-21:-1] == h[:20], while t[-20:] != h[:20]
            t = _rand(rng, 60)
            h = t[-21:-1] + y
            claim = ("trap", "early_t", 20)
        g.contigs = [h] + filler + [t]
        g.pairs = [(2 * 3, 0)]
        g.labels = [which]
        g.claims = [claim]
        groups.append(g)
    return groups


def check_claims(group):
    """that every shape is what its label says: raises AssertionError otherwise"""
    want = group.expected()
    store = "".join(c.upper() for c in group.contigs)
    store += "".join(revcomp(c.upper()) for c in group.contigs)
    for (t, h), label, claim, found in zip(group.pairs, group.labels, group.claims, want):
        T, H = group.oriented(t), group.oriented(h)
        m = min(len(T), len(H))
        assert found == sorted(found, reverse=True)
        if claim is None:
            continue
        kind = claim[0]
        if kind == "has":
            assert claim[1] in found, label
        elif kind == "lacks":
            assert claim[1] not in found and claim[1] <= m, label
        elif kind == "min":
            assert m == claim[1], label
        elif kind == "is":
            if claim[1] is not None:
                assert found == claim[1], (label, found)
        elif kind == "step":
            p, n = claim[1], claim[2]
            assert found == list(range(n, 0, -p)), (label, found[:5])
        elif kind == "across":
            p, n = claim[1], claim[2]
            assert found[:4] == [n, n - p, n - 2 * p, n - 3 * p] and len(found) > 3, (label, found)
            step = lambda l: (m - l) // 64
            assert step(found[0]) < step(found[2]) and step(found[3]) >= step(found[2]), label
        elif kind == "one_off":
            n, q = claim[1], claim[2]
            assert [i for i in range(n) if T[len(T) - n + i] != H[i]] == [q] and n not in found, label
        elif kind == "trap":
            l = claim[2]
            assert l not in found, label
            assert (t, h) == (2 * (len(group.contigs) - 1), 0)
            tpos = sum(len(c) for c in group.contigs[:-1])
            if claim[1] == "late_t":
                assert store[tpos + len(T) - l + 1:tpos + len(T) + 1] == H[:l], label
            elif claim[1] == "early_t":
                assert store[tpos + len(T) - l - 1:tpos + len(T) - 1] == H[:l], label
            else:
                assert l == len(H) + 1 and store[tpos + len(T) - l:tpos + len(T)] == store[0:l], label
