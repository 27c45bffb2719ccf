"""Shared by the MergeContigs tests: the goldens of tests/golden/mergecontigs (made by tests/golden/make_mergecontigs.py from the
unmodified reference), readers of their inputs, generated inputs for the GPU tests and a plain-Python restatement of the merge
(MergePaths/MergeContigs.cpp:159-313 with Align/smith_waterman.cpp) that owes nothing to abg_mc.h: it builds the sequence as a string,
junction by junction, as the reference does."""
import functools
import json
import os
import random
import re
import subprocess
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mergecontigs")
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

@functools.lru_cache(maxsize=None)
def _data():
    with tarfile.open(os.path.join(GOLDEN, "data.tar.gz")) as tar:
        return {m.name: tar.extractfile(m).read() for m in tar.getmembers() if m.isfile()}


def golden(name):
    return _data()[name]


@functools.lru_cache(maxsize=None)
def cases():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))


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
