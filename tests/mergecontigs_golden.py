"""Shared by the MergeContigs tests: the goldens of tests/golden/mergecontigs (made by tests/golden/make_mergecontigs.py from the
unmodified reference), readers of their inputs, generated inputs for the GPU tests and a plain-Python restatement of the merge
(MergePaths/MergeContigs.cpp:159-313 with Align/smith_waterman.cpp) that owes nothing to abg_mc.h: it builds the sequence as a string,
junction by junction, as the reference does.  dirty_paths() and dirty_sets() generate, over that restatement, the paths with
content (case, N, codes, gaps, overlaps that differ, planned conflicts) that the device tests and `mc_check splice` both merge."""
import functools
import json
import os
import random
import re
import subprocess

import golden_archive

HERE = os.path.dirname(os.path.abspath(__file__))
COMP = bytes.maketrans(b"ACGTacgtMRWSYKVHDBNmrwsykvhdbn", b"TGCAtgcaKYWSRMBDHVNkywsrmbdhvn")
MASK = {"A": 1, "C": 2, "G": 4, "T": 8, "M": 3, "R": 5, "S": 6, "V": 7, "W": 9, "Y": 10, "H": 11, "K": 12, "D": 13, "B": 14, "N": 15}
UNMASK = "NACMGRSVTWYHKDBN"


# ---- the restatement

def rc(s):
    return s.translate(COMP)[::-1]


def node_sequence(contigs, k, node):
    """sequence(), MergeContigs.cpp:159-171; node = 2 * contig + sense, or -n for the gap of n"""
    if node < 0:
        n = -node
        return b"N" * (k - 1) + (b"n" if n < k else b"N") * n
    s = contigs[node >> 1]
    return rc(s) if node & 1 else s


def create_consensus(a, b):
    """createConsensus, MergeContigs.cpp:176-197: '' when there is none"""
    if a == b:
        return a
    out = []
    for x, y in zip(a.decode(), b.decode()):
        mask = x.islower() or y.islower()
        ca, cb = x.upper(), y.upper()
        if ca == cb:
            c = ca
        elif ca == "N":
            c = cb
        elif cb == "N":
            c = ca
        else:
            both = MASK[ca] & MASK[cb]
            if both != MASK[ca] and both != MASK[cb]:
                return b""
            c = UNMASK[MASK[ca] | MASK[cb]]
        out.append(c.lower() if mask else c)
    return "".join(out).encode()


def _ambiguity(a, b, isor):
    m = MASK[a.upper()] | MASK[b.upper()] if isor else MASK[a.upper()] & MASK[b.upper()]
    c = UNMASK[m]
    lower = (a.islower() or b.islower()) if isor else (a.islower() and b.islower())
    return c.lower() if lower else c


def _is_match(a, b):
    """isMatch, smith_waterman.cpp:65-80: (matches, consensus character)"""
    if a == b:
        return True, a
    if a.upper() == b.upper():
        return True, (a.lower() if a.islower() or b.islower() else a)
    if a in "Nn":
        return True, b
    if b in "Nn":
        return True, a
    both = _ambiguity(a, b, False)
    return both == a or both == b, _ambiguity(a, b, True)


@functools.lru_cache(maxsize=None)  # (a generated path is merged again after every node it gains, and once more by the test)
def align_overlap(a, b, verbose):
    """alignOverlap(a, b, 0, overlaps, false, verbose), smith_waterman.cpp:179-292: None, or (t_pos, h_pos, consensus, matches, print)"""
    a, b = a.decode(), b.decode()
    na, nb = len(a), len(b)
    NEG = float("-inf")
    H = [[0.0] * (nb + 1) for _ in range(na + 1)]
    Ii = [[0] * (nb + 1) for _ in range(na + 1)]
    Ij = [[0] * (nb + 1) for _ in range(na + 1)]
    V = [[False] * (nb + 1) for _ in range(na + 1)]
    for i in range(na + 1):
        Ii[i][0], V[i][0] = i - 1, True
    for j in range(nb + 1):
        Ij[0][j], V[0][j] = j - 1, False
    V[0][0] = True
    for i in range(1, na + 1):
        for j in range(1, nb + 1):
            scores = [H[i - 1][j - 1] + (5 if _is_match(a[i - 1], b[j - 1])[0] else -4) if V[i - 1][j - 1] else NEG,
                      H[i - 1][j] + (-4 if Ij[i - 1][j] == j else -12) if V[i - 1][j] else NEG,
                      H[i][j - 1] + (-4 if Ii[i][j - 1] == i else -12) if V[i][j - 1] else NEG]
            best = scores.index(max(scores))
            H[i][j] = scores[best]
            Ii[i][j], Ij[i][j] = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][best]
            V[i][j] = H[i][j] != NEG
    last = H[na]
    # (std::sort leaves equal scores in an order of its own; a tie between two columns that both backtrack to the first column would
    # show here as a difference from the golden, and none does)
    for jmax in sorted(range(1, nb + 1), key=lambda j: -last[j]):
        if last[jmax] == 0:
            break
        ci, cj = na, jmax
        ni, nj = Ii[ci][cj], Ij[ci][cj]
        qa, ta, match, matches = [], [], [], 0
        while (ci != ni or cj != nj) and nj != 0 and ni != 0:
            if ni == ci:
                qa.append("-"), match.append(b[cj - 1].lower()), ta.append(b[cj - 1])
            else:
                qa.append(a[ci - 1])
                if nj == cj:
                    ta.append("-"), match.append(a[ci - 1].lower())
                else:
                    ta.append(b[cj - 1])
                    ok, c = _is_match(a[ci - 1], b[cj - 1])
                    match.append(c)
                    matches += ok
            ci, cj = ni, nj
            ni, nj = Ii[ci][cj], Ij[ci][cj]
        if cj > 1:
            continue
        qa.append(a[ci - 1]), ta.append(b[cj - 1])
        ok, c = _is_match(a[ci - 1], b[cj - 1])
        match.append(c)
        matches += ok
        if not matches:
            continue
        qa, ta, match = "".join(reversed(qa)), "".join(reversed(ta)), "".join(reversed(match))
        t_pos, h_pos = ci - 1, jmax - 1
        text = ""
        if verbose:
            text = a[:t_pos] + qa + "\n" + " " * t_pos + "".join("." if m == x or m == y else m for m, x, y in zip(match, qa, ta)) + "\n" + " " * t_pos + ta + b[h_pos + 1:] + "\n"
        return t_pos, h_pos, match, matches, text
    return None


def py_merge_path(contigs, k, nodes, overlaps, verbose=0, names=None):
    """mergePath's sequence: (sequence, flagged, stderr text).  overlaps[j]: of nodes[j] with what precedes it (overlaps[0] unused).
    flagged: a junction's first consensus failed, which is when abg_mc hands the path to the host.  names: node -> str for the warning."""
    import numpy as np
    names = names or (lambda u: "%dN" % -u if u < 0 else "%d%s" % (u >> 1, "+-"[u & 1]))
    seq, flagged, log = b"", False, ""
    for j, node in enumerate(nodes):
        if not seq:
            seq = node_sequence(contigs, k, node)
            continue
        ov = overlaps[j]
        s = node_sequence(contigs, k, node)
        assert len(s) >= ov
        bo = s[:ov]
        merged = False
        while True:
            assert len(seq) >= ov
            ao = seq[len(seq) - ov:]
            o = create_consensus(ao, bo)
            if o:
                seq = seq[:len(seq) - ov] + o + s[ov:]
                merged = True
                break
            flagged = True
            if seq.endswith(b"n"):
                seq = seq[:-1]
            else:
                break
        if merged:
            continue
        if verbose > 2:
            log += "\n"
        al = align_overlap(ao, bo, verbose > 2)
        good = False
        if al:
            t_pos, h_pos, cons, matches, text = al
            log += text
            identity = np.float32(matches) / np.float32(len(cons))
            good = matches >= 20 and identity >= np.float32(0.9)
            if verbose > 2:
                log += "%d / %d = %s%s\n" % (matches, len(cons), "%g" % identity, " (too few)" if matches < 20 else " (too low)" if identity < np.float32(0.9) else " (good)")
        if good:
            seq = seq[:len(seq) - ov + t_pos] + cons.encode() + s[h_pos + 1:]
        else:
            log += "warning: the head of %s does not match the tail of the previous contig\n%s\n%s\n%s\n" % (
                names(node), ao.decode(), bo.decode(), " ".join(names(u) for u in nodes))
            seq += b"n" + s
    return seq, flagged, log


# ---- the goldens

_files, golden, cases = golden_archive.bind("mergecontigs")


def rules():
    return json.load(open(os.path.join(HERE, "golden", "mergecontigs_rules.json")))


def needs_device(case):
    """does the run reach a path of two or more nodes?  (every case that ends well and has one; the error cases stop earlier or not, and
    are run on the GPU machine only)"""
    if case["status"] != 0 or case.get("refused"):
        return None
    path = case["argv"][-1] if case["argv"] else ""
    if path != "-" and path not in case["inputs"]:
        return None  # (--help, --version)
    text = golden(case["stdin"]) if path == "-" else golden(path)
    return any(len(line.split()) > 2 for line in text.decode().splitlines())


def run_case(cmd, case, d, env=None):
    """(status, stdout, stderr, -o file, -g file) of cmd + argv in a directory that holds the inputs"""
    for name in case["inputs"]:
        (d / name).write_bytes(golden(name))
    e = dict(os.environ, **(env or {}))
    e.pop("COLUMNS", None)
    r = subprocess.run(list(cmd) + case["argv"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120,
                       input=golden(case["stdin"]) if case["stdin"] else b"")
    read = lambda f: (d / f).read_bytes() if (d / f).exists() else None
    return r.returncode, r.stdout, r.stderr.decode(), read("out.fa"), read("out.g")


def check_case(case, got):
    status, out, err, fa, graph = got
    if case.get("refused"):  # colour-space contigs: the reference merges them, this build says it does not
        assert status == 1 and err.startswith("MergeContigs: error: ") and any(i in err for i in case["inputs"]), (status, err)
        return
    if case.get("aborts"):  # the reference's lines up to its assert, then one line of the drop-in's own that names the input
        assert status == 1 and err.startswith(case["stderr"]), (status, err)
        rest = err[len(case["stderr"]):]
        assert rest == "" or (rest.startswith("MergeContigs: error: ") and rest.count("\n") == 1), rest
        assert rest or case["stderr"].strip().startswith("error:") or "\nerror:" in case["stderr"], err
        return
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    err = "".join(re.sub(r"^\S*/(MergeContigs|mc_check): ", "MergeContigs: ", ln) for ln in err.splitlines(True))
    assert err == case["stderr"], (err, case["stderr"])
    assert status == case["status"]
    assert out == (golden(case["stdout"]) if case["stdout"] else b"")
    assert fa == (golden(case["out"]) if case["out"] else None)
    if graph is not None:  # (the SAM header holds the command line, argv[0] included)
        graph = re.sub(rb"\tCL:\S*/(MergeContigs|mc_check) ", b"\tCL:MergeContigs ", graph)
    assert graph == (golden(case["graph"]) if case["graph"] else None)


# ---- readers of a case's inputs: what api.PathMerge.merge takes

def read_fasta(data):
    """[(name, sequence)]"""
    out = []
    for rec in data.split(b">")[1:]:
        head, _, body = rec.partition(b"\n")
        out.append((head.split()[0].decode(), body.replace(b"\n", b"")))
    return out


def read_adj(data, k):
    """names in file order and {(u, v): d} over vertices 2 * index + sense"""
    rows = [l.split(";") for l in data.decode().splitlines() if l.strip()]
    names = [r[0].split()[0] for r in rows]
    ids = {n: i for i, n in enumerate(names)}
    edges = {}
    for head, right, left in rows:
        u = 2 * ids[head.split()[0]]
        for sense, part in ((0, right), (1, left)):
            for m in re.finditer(r"(\S+)([+-])(?:\s*\[d=(-?\d+)\])?(?=\s|$)", part):
                v = 2 * ids[m.group(1)] + (m.group(2) == "-")
                edges[(u ^ sense, v ^ sense)] = int(m.group(3)) if m.group(3) else -(k - 1)
    return names, edges


def case_paths(case):
    """(k, contigs in graph order, [(id, nodes, overlaps)]) of an ADJ case: its paths of two or more nodes"""
    k = int(next(a for a in case["argv"] if a.startswith("-k"))[2:])
    args = [a for a in case["argv"] if a in case["inputs"]]
    fasta, adj, path = args if len(args) == 3 else (args[0], None, args[1])
    records = read_fasta(golden(fasta))
    if adj:
        names, edges = read_adj(golden(adj), k)
        by_name = dict(records)
        contigs = [by_name[n] for n in names]
    else:
        names, edges, contigs = [n for n, _ in records], {}, [s for _, s in records]
    ids = {n: i for i, n in enumerate(names)}
    out = []
    for line in golden(path).decode().splitlines():
        words = line.split()
        if len(words) < 3:
            continue
        nodes = [-int(w[:-1]) if w.endswith("N") else 2 * ids[w[:-1]] + (w[-1] == "-") for w in words[1:]]
        ov = [0] + [k - 1 if u < 0 or v < 0 else -edges[(u, v)] for u, v in zip(nodes, nodes[1:])]
        out.append((words[0], nodes, ov))
    return k, contigs, out


# ---- generated inputs for the GPU tests

def chains(seed, k, npaths, lengths, overlap=None, senses=None):
    """npaths chains cut from random sequence, consecutive contigs sharing `overlap` (default k - 1): (contigs, [(nodes, overlaps)])"""
    rng = random.Random(seed)
    ov = k - 1 if overlap is None else overlap
    contigs, paths = [], []
    for p in range(npaths):
        ls = lengths(p) if callable(lengths) else lengths
        genome = bytes(rng.choice(b"ACGT") for _ in range(sum(ls) - ov * (len(ls) - 1)))
        at, nodes = 0, []
        for j, l in enumerate(ls):
            sense = (senses or "+-+")[(p + j) % len(senses or "+-+")] == "-"
            piece = genome[at:at + l]
            contigs.append(rc(piece) if sense else piece)
            nodes.append(2 * (len(contigs) - 1) + sense)
            at += l - ov
        paths.append((nodes, [0] + [ov] * (len(ls) - 1)))
    return contigs, paths


# ---- generated inputs with content: case, N, codes, gaps, overlaps that differ within a path, planned conflicts

def _superset(rng, c, strict=False):
    """a code that holds every base of c, in c's case; strict: a larger one that is not N (N when there is no other)"""
    m = MASK[c.upper()]
    masks = [x for x in range(1, 16) if x & m == m and not (strict and x in (m, 15))] or [15]
    out = UNMASK[rng.choice(masks)]
    return out.lower() if c.islower() else out


def _agree(rng, t, dirt):
    """a head character that has a consensus with the tail character t"""
    if t in "Nn":  # gives way to anything
        return rng.choice("ACGT") if rng.random() >= dirt else rng.choice("NnacgtRYKMSWBDHVry")
    if rng.random() >= dirt:
        return t
    return (t.lower(), rng.choice("Nn"), _superset(rng, t), _superset(rng, t, True))[rng.randrange(4)]


def _body(rng, dirt):
    if rng.random() >= dirt:
        return rng.choice("ACGT")
    return (rng.choice("Nn"), rng.choice("acgt"), rng.choice("MRWSYKVHDB"), rng.choice("mrwsykvhdb"))[rng.randrange(4)]


def _edit(rng, t, kind):
    """the character a planned edit puts where t is (a head character: where the tail has t)"""
    if kind in ("N", "n"):
        return kind
    if kind == "lower":
        return t.lower()
    if kind == "code":
        return _superset(rng, t, True)
    m = MASK[t.upper()]
    if kind == "solid":  # a plain base that t holds: the consensus there is no N
        return rng.choice([b for b in "ACGT" if MASK[b] & m])
    assert kind == "break" and m != 15, (t, kind)  # a base that t does not hold: no consensus
    return rng.choice([b for b in "ACGT" if not MASK[b] & m])


class Grow:
    """One path built from left to right over the merged sequence so far, py_merge_path's.  Its contigs are appended to `contigs`."""

    def __init__(self, rng, contigs, k, dirt=0.0):
        self.rng, self.contigs, self.k, self.dirt = rng, contigs, k, dirt
        self.nodes, self.ov, self.seq = [], [], b""

    def _merged(self):
        self.seq = py_merge_path(self.contigs, self.k, self.nodes, self.ov)[0]

    def gap(self, n, ov=None):
        """the gap of n, joined by k - 1 as MergeContigs joins it, or by `ov`"""
        ov = self.k - 1 if ov is None else ov
        assert self.nodes and self.nodes[-1] >= 0 and 0 < ov <= min(self.k - 1, len(self.seq)) and n > 0
        self.nodes.append(-n)
        self.ov.append(ov)
        self._merged()

    def contig(self, length, sense, ov=0, edits=None):
        """a contig of `length` characters in the path's sense, the first `ov` of them a head that has a consensus with the current
        tail (every character the same, in lower case, an N or a superset code, `dirt` of the time), the rest random; stored reverse
        complemented where sense is true.  edits: {position in the path's sense: "lower", "N", "n", "code", "solid" or "break"}"""
        ov = ov if self.nodes else 0
        assert ov <= length and ov <= len(self.seq) and (ov > 0 or not self.nodes)
        tail = self.seq[len(self.seq) - ov:].decode() if ov else ""
        s = [_agree(self.rng, t, self.dirt) for t in tail] + [_body(self.rng, self.dirt) for _ in range(length - ov)]
        for at, kind in sorted((edits or {}).items()):
            s[at] = _edit(self.rng, tail[at] if at < ov else s[at], kind)
        s = "".join(s).encode()
        self.contigs.append(rc(s) if sense else s)
        self.nodes.append(2 * (len(self.contigs) - 1) + bool(sense))
        self.ov.append(ov)
        self._merged()

    def path(self):
        return self.nodes, self.ov


def dirty_paths(seed, k, npaths, dirt=0.15, gaps=True, breaks=None, nodes=(2, 8), overlap=(1, 90), length=None):
    """(contigs, [(nodes, overlaps)], plan): paths of nodes[0] .. nodes[1] nodes in either sense whose junctions all have a consensus,
    with overlaps drawn per junction, nodes that are all window, lower case, N and codes in heads and bodies, and gaps (never first,
    last or two in a row; of 1, k - 2, k - 1, k, k + 1 and up to 2k; the head after a short gap agrees with what its window reaches
    before the gap, since it is made from the merged tail).  length: (lo, hi) of a node's whole length, where the default is its
    overlap and up to 120 more.  breaks: {path: (junction, position)}, junction j being that of node j with what precedes it: that
    window gets one pair without a consensus there; such a path has no gap.  plan["flagged"]: the paths with a break."""
    rng = random.Random(seed)
    breaks = breaks or {}
    contigs, paths = [], []
    for p in range(npaths):
        brk = breaks.get(p)
        n = max(rng.randint(*nodes), brk[0] + 1 if brk else 0)
        g = Grow(rng, contigs, k, dirt)
        ahead = 0  # the overlap of the junction with the break, drawn a node early
        while len(g.nodes) < n:
            j = len(g.nodes)
            if gaps and not brk and 0 < j < n - 1 and g.nodes[-1] >= 0 and len(g.seq) >= k - 1 and rng.random() < 0.25:
                g.gap(rng.choice([1, k - 2, k - 1, k, k + 1, rng.randint(1, 2 * k)]))
                continue
            after_gap = j > 0 and g.nodes[-1] < 0
            edits = {}
            if length:
                ln = max(rng.randint(*length), k - 1 if after_gap else 1)
                ov = k - 1 if after_gap else min(rng.randint(*overlap), ln, len(g.seq))
            else:
                ov = 0 if j == 0 else k - 1 if after_gap else ahead if brk and j == brk[0] else min(rng.randint(*overlap), len(g.seq))
                ln = ov + (0 if j and rng.random() < 0.2 else rng.randint(1, 120))
            if brk and j == brk[0] - 1:  # the tail character of the pair: no N, and inside this node
                ahead = rng.randint(max(brk[1] + 1, overlap[0]), max(brk[1] + 1, overlap[1]))
                ln = max(ln, ahead)
                edits[ln - ahead + brk[1]] = "solid"
            if brk and j == brk[0]:
                assert not length and ov == ahead
                edits[brk[1]] = "break"
            g.contig(ln, rng.random() < 0.5, ov, edits)
        paths.append(g.path())
    return contigs, paths, {"flagged": sorted(breaks), "breaks": dict(breaks)}


def dump_paths(path, k, contigs, paths):
    """what `mc_check splice` reads: "k contigs paths", a contig a line, then a path a line: its number of nodes, then node and overlap
    of each"""
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (k, len(contigs), len(paths)))
        for c in contigs:
            f.write(c.decode() + "\n")
        for nodes, ov in paths:
            f.write(" ".join(["%d" % len(nodes)] + ["%d %d" % (u, o) for u, o in zip(nodes, ov)]) + "\n")


WINDOW_OVERLAPS = (63, 64, 65, 128, 129)


def window_positions(w):
    """the ends of a window and both sides of the second trip of a wave's lanes over it"""
    return [q for q in sorted({0, 62, 63, 64, w - 1}) if q < w]


def _window_set(k):
    """paths of two nodes, ACGT but for one character: a lower-case base or an N in the tail, or a superset code in the head"""
    rng = random.Random(2)
    contigs, paths, marks = [], [], []
    for kind in ("lower", "code", "N"):
        for w in WINDOW_OVERLAPS:
            for q in window_positions(w):
                g = Grow(rng, contigs, k)
                first = w + 3 + len(paths) % 40
                g.contig(first, len(paths) & 1, 0, {first - w + q: kind} if kind != "code" else None)
                g.contig(w + 1 + len(paths) % 23, len(paths) & 2, w, {q: kind} if kind == "code" else None)
                marks.append((len(paths), first - w + q, kind))
                paths.append(g.path())
    return dict(k=k, contigs=contigs, paths=paths, marks=marks)


CONFLICT_AT = (0, 31, 63, 64, 129)
CONFLICTS = [(w, q, place) for place in (1, 2, 3) for w in WINDOW_OVERLAPS for q in window_positions(w)]
CONFLICT_SETS = (len(CONFLICTS) + len(CONFLICT_AT) - 1) // len(CONFLICT_AT)


def _conflict_set(k, which):
    """130 paths of four nodes, ACGT only; those at CONFLICT_AT have one pair without a consensus, five of CONFLICTS in turn: the
    overlap of the junction, the position in its window, and which of the three junctions it is"""
    rng = random.Random(300 + which)
    contigs, paths, breaks = [], [], {}
    for p in range(130):
        ovs = [WINDOW_OVERLAPS[(p + j) % 5] for j in range(3)]
        edits = {}
        if p in CONFLICT_AT:
            w, q, place = CONFLICTS[(which * len(CONFLICT_AT) + CONFLICT_AT.index(p)) % len(CONFLICTS)]
            ovs[place - 1] = w
            edits = {place: {q: "break"}}
            breaks[p] = (place, q)
        g = Grow(rng, contigs, k)
        g.contig(131 + p % 7, p & 1)
        for j in (1, 2, 3):
            g.contig(ovs[j - 1] + (p + j) % 9, (p >> j) & 1, min(ovs[j - 1], len(g.seq)), edits.get(j))
        assert not edits or g.ov[breaks[p][0]] == w
        paths.append(g.path())
    return dict(k=k, contigs=contigs, paths=paths, flagged=sorted(breaks), breaks=breaks)


RING_OVERLAPS = (1023, 1024, 1025)


def _ring_sets(k):
    """for each overlap around the ring's size a path [3000, ov, ov + 3, 2 ov + 7, 37]: the second node is all window, the last is
    joined by 7, and lower-case marks sit at positions 0 and ov - 1 of the windows of the three large junctions (the first's in the
    tail; the second's come down with the first's consensus; the third's in the head and in the tail).  With 20 small paths, in three
    orders: the path the ring cannot hold in the middle, first and last."""
    rng = random.Random(4)
    contigs, big = [], []
    for i, ov in enumerate(RING_OVERLAPS):
        g = Grow(rng, contigs, k)
        sense = lambda j: "+-+--+-+"[(i + j) % 8] == "-"
        g.contig(3000, sense(0), 0, {3000 - ov: "lower", 2999: "lower"})
        g.contig(ov, sense(1), ov)
        g.contig(ov + 3, sense(2), ov, {ov + 2: "lower"})
        g.contig(2 * ov + 7, sense(3), ov, {0: "lower"})
        g.contig(37, sense(4), 7)
        big.append(g.path())
    more, small, _ = dirty_paths(5, k, 20)
    small = [([u + 2 * len(contigs) if u >= 0 else u for u in nodes], ov) for nodes, ov in small]
    contigs = contigs + more
    orders = {"mid": small[:10] + [big[0], big[2], big[1]] + small[10:], "first": [big[2], big[0], big[1]] + small, "last": small + big}
    return {"ring." + name: dict(k=k, contigs=contigs, paths=paths, host=[i for i, (_, ov) in enumerate(paths) if max(ov) > 1024])
            for name, paths in orders.items()}


GAP_SIZES = (1, 15, 16, 17, 23, 24, 25, 26, 40)


def _gap_set(k):
    """[contig, gap n, contig] for every n of GAP_SIZES, the first contig as long as puts the gap's first own byte at offsets 0, 1 and
    15 of a 16-byte chunk of the flat output of one batch"""
    rng = random.Random(6)
    contigs, paths, gap_at, at = [], [], [], 0
    for target in (0, 1, 15):
        for n in GAP_SIZES:
            g = Grow(rng, contigs, k, 0.15)
            first = 30 + len(paths) % 5
            first += (target - at - first) % 16
            g.contig(first, len(paths) & 1)
            g.gap(n)
            g.contig(k - 1 + 5 + len(paths) % 19, len(paths) & 2, k - 1)
            gap_at.append((at + first, target))
            at += len(g.seq)
            paths.append(g.path())
    return dict(k=k, contigs=contigs, paths=paths, gap_at=gap_at)


def _short_gap_set(k):
    """[contig, gap n, contig] with the gap joined by fewer than k - 1 and the contig after it by fewer than n.  Joined by k - 1 on
    both sides, as in every other set, a gap keeps bytes of its own in the layout only when n >= k, and those are all N: its k - 1
    leading N lie in the window before it, and n < k of n lie in the window after it, which the consensus writes.  Only these paths
    lay out the N run and the n run of one gap (n < k) side by side, and any n run at all."""
    rng = random.Random(9)
    contigs, paths = [], []
    for n in (2, 5, 16, 17, k - 1, k, 40):
        for before in (1, 7, k - 2):
            for after in (1, 3):
                if after < n:
                    g = Grow(rng, contigs, k, 0.15)
                    g.contig(26 + len(paths) % 16, len(paths) & 1)
                    g.gap(n, before)
                    g.contig(after + 4 + len(paths) % 21, len(paths) & 2, after)
                    paths.append(g.path())
    return dict(k=k, contigs=contigs, paths=paths)


DIRTY_SETS = ("dirty", "dirty.breaks", "window") + tuple("conflict.%d" % which for which in range(CONFLICT_SETS)) + \
    ("ring.mid", "ring.first", "ring.last", "gaps", "gaps.short", "seams")


@functools.lru_cache(maxsize=None)
def dirty_sets():
    """the generated sets of the device tests, which tests/test_mergecontigs_host.py runs through `mc_check splice` too:
    name -> dict(k, contigs, paths, flagged: paths with a junction that has no consensus, host: paths the ring cannot hold, ...)"""
    k = 25
    sets = {}
    contigs, paths, plan = dirty_paths(1, k, 257)
    sets["dirty"] = dict(k=k, contigs=contigs, paths=paths, flagged=plan["flagged"])
    contigs, paths, plan = dirty_paths(7, k, 40, breaks={0: (1, 0), 5: (3, 17), 11: (2, 89), 39: (7, 40)})
    sets["dirty.breaks"] = dict(k=k, contigs=contigs, paths=paths, flagged=plan["flagged"], breaks=plan["breaks"])
    sets["window"] = _window_set(k)
    for which in range(CONFLICT_SETS):
        sets["conflict.%d" % which] = _conflict_set(k, which)
    sets.update(_ring_sets(k))
    sets["gaps"] = _gap_set(k)
    sets["gaps.short"] = _short_gap_set(k)
    contigs, paths, plan = dirty_paths(8, k, 64, dirt=0.2, gaps=False, nodes=(8, 8), overlap=(1, 3), length=(1, 5))
    sets["seams"] = dict(k=k, contigs=contigs, paths=paths, flagged=plan["flagged"])
    for s in sets.values():
        s.setdefault("flagged", [])
        s.setdefault("host", [])
    assert tuple(sets) == DIRTY_SETS
    return sets


@functools.lru_cache(maxsize=None)
def expected(name):
    """py_merge_path of every path of a set of dirty_sets(): [(sequence, flagged, log)], computed once"""
    s = dirty_sets()[name]
    return tuple(py_merge_path(s["contigs"], s["k"], nodes, ov) for nodes, ov in s["paths"])
