"""Shared by the SimpleGraph tests: the goldens of tests/golden/simplegraph (made by tests/golden/make_simplegraph.py from the
unmodified reference), search files of tests/hostcheck/sg_check, the small shapes of the search tests and a plain-Python restatement
of the recursive search (Graph/ConstrainedSearch.h:56-144) that owes nothing to abg_sg.h: it recurses as the reference does and keeps
the reference's bound-sorted copy and its nextConstraint walk."""
import functools
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np

import golden_archive

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_COST, MAX_PATHS = 100000, 200
SATISFIED = 2 ** 31 - 1


# ---- the restatement

def py_search(graph, origin, constraints, max_cost=MAX_COST, max_paths=MAX_PATHS, reverse_ties=False):
    """(numVisited, solutions) of constrainedSearch.  graph: vertex -> [(target, distance)] in edge order, and graph.length[vertex];
    constraints: [(vertex, bound)] in any order.  reverse_ties: sort the copy by bound so that equal bounds come in the other order,
    which the result must not depend on."""
    if not constraints:
        return 0, []
    cons = sorted([v, b] for v, b in constraints)  # by vertex, then by bound
    queue = sorted(([v, b] for v, b in cons), key=lambda c: c[1])
    if reverse_ties:
        queue = sorted(reversed(queue), key=lambda c: c[1])
    state = {"visited": 0}
    solutions = []
    path = []

    def find(v):
        lo, hi = 0, len(cons)
        while lo < hi:
            mid = (lo + hi) // 2
            if cons[mid][0] < v:
                lo = mid + 1
            else:
                hi = mid
        return cons[lo] if lo < len(cons) and cons[lo][0] == v else None

    def rec(u, nxt, satisfied, distance):
        if path:
            v = path[-1]
            c = find(v)
            if c is not None and c[1] != SATISFIED:
                if distance > c[1]:
                    return True
                satisfied += 1
                if satisfied == len(cons):
                    solutions.append(list(path))
                    return len(solutions) <= max_paths
                bound = c[1]
                c[1] = SATISFIED
                if not rec(u, nxt, satisfied, distance):
                    return False
                c[1] = bound
                return True
            state["visited"] += 1
            if state["visited"] >= max_cost:
                return False
            pruned = None
            while True:
                if nxt >= len(queue):  # the reference reads past the end of its list here (a vertex listed twice, every entry
                    pruned = False     # looking satisfied): undefined there; no prune here, as in abg_sg.h
                    break
                if distance > queue[nxt][1] and find(queue[nxt][0])[1] == SATISFIED:
                    nxt += 1
                    continue
                pruned = distance > queue[nxt][1]
                break
            if pruned:
                return True
            distance += graph.length[v]
            u = v
        path.append(None)
        for v, d in graph.out[u]:
            path[-1] = v
            if not rec(u, nxt, satisfied, distance + d):
                return False
        path.pop()
        return True

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20000))
    try:
        rec(origin, 0, 0, 0)
    finally:
        sys.setrecursionlimit(limit)
    return state["visited"], solutions


class Graph:
    """oriented vertices 2 * contig + sense; out[u] = [(v, d)] in insertion order"""

    def __init__(self, lengths):
        self.length = [l for l in lengths for _ in (0, 1)]
        self.out = [[] for _ in self.length]

    def edge(self, u, v, d):
        """as ContigGraph::add_edge: the edge and its complement"""
        self.out[u].append((v, d))
        if u != v ^ 1:
            self.out[v ^ 1].append((u ^ 1, d))

    def csr(self):
        off = np.zeros(len(self.out) + 1, dtype=np.uint64)
        np.cumsum([len(o) for o in self.out], out=off[1:])
        tgt = np.array([v for o in self.out for v, _ in o], dtype=np.uint32)
        dist = np.array([d for o in self.out for _, d in o], dtype=np.int32)
        return off, np.array(self.length, dtype=np.uint32), tgt, dist


# ---- the goldens

_files, golden, cases = golden_archive.bind("simplegraph")


def rules():
    return json.load(open(os.path.join(HERE, "golden", "simplegraph_rules.json")))


def needs_device(case):
    """whether the run searches at all (the reference's own "Total paths attempted")"""
    return case.get("searches", 0) > 0


def run_case(prefix, case, tmp, env=None):
    """runs `prefix + argv` in tmp as the generator ran the reference: (status, stdout, stderr, the -o file or None)"""
    tmp = str(tmp)
    for name in case["inputs"]:
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(golden(name))
    e = dict(os.environ)
    e.pop("COLUMNS", None)
    e.update(env or {})
    r = subprocess.run(list(prefix) + list(case["argv"]), cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    written = None
    for f in ("out.path", "x.path"):
        p = os.path.join(tmp, f)
        if os.path.exists(p):
            written = open(p, "rb").read()
            os.remove(p)
    return r.returncode, r.stdout, r.stderr.decode(), written


def check_case(case, got):
    """every byte of stdout, the -o file, stderr and the status against what the reference wrote.  Where the reference aborts (a name
    the graph lacks) the drop-in exits 1 and its first line of stderr is the reference's."""
    status, out, err, path = got
    if case.get("aborts"):
        assert status == 1 and err.splitlines()[0] == case["stderr"].splitlines()[0], err
        return
    assert status == case["status"], err
    want_out = golden(case["stdout"]) if case["stdout"] else case["stdout_text"].encode()
    assert out == want_out
    if case["status"] == 0:
        assert path == (golden(case["out"]) if case["out"] else None)
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    assert [re.sub(r"^\S*/(SimpleGraph|sg_check): ", "SimpleGraph: ", ln) for ln in err.splitlines()] == case["stderr"].splitlines()


def parse_adj(text, k):
    """an ADJ file -> (Graph, names): the edges in the order Graph/AdjIO.h adds them"""
    lines = [l for l in text.decode().splitlines() if l.strip()]
    names = [l.split()[0] for l in lines]
    ids = {n: i for i, n in enumerate(names)}
    g = Graph([int(l.split()[1]) for l in lines])
    for l in lines:
        u = 2 * ids[l.split()[0]]
        parts = l.split(";")
        for sense in (0, 1):
            for m in re.finditer(r"(\S+)([+-])(?:\s*\[d=(-?\d+)\])?", parts[1 + sense]):
                v = 2 * ids[m.group(1)] + (m.group(2) == "-")
                g.out[u ^ sense].append((v ^ sense, int(m.group(3)) if m.group(3) else -(k - 1)))
    return g, names


def verbose_blocks(stdout):
    """the -v text of a run -> [(origin name, constraints as written, Paths lines, 'Solutions:' line)]"""
    blocks = []
    for chunk in stdout.decode().split("\n* ")[1:]:
        lines = chunk.split("\n")
        cons = [(c.rsplit(",", 1)[0], int(c.rsplit(",", 1)[1])) for c in lines[1][len("Constraints:"):].split()]
        paths = []
        sol = next(l for l in lines if l.startswith("Solutions: "))
        if any(l.startswith("Paths: ") for l in lines):
            at = next(i for i, l in enumerate(lines) if l.startswith("Paths: "))
            n = int(lines[at][7:])
            per = 1 + len(cons)
            paths = [lines[at + 1 + i * per] for i in range(n)]
        blocks.append((lines[0], cons, paths, sol))
    return blocks


# ---- search files (tests/hostcheck/sg_check.cc)

def write_searches(path, graph, searches, max_cost=MAX_COST, max_paths=MAX_PATHS):
    off, length, tgt, dist = graph.csr()
    coff = np.zeros(len(searches) + 1, dtype="<u8")
    np.cumsum([len(c) for _, c in searches], out=coff[1:])
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(length)))
        f.write(off.astype("<u8").tobytes() + length.astype("<u4").tobytes() + tgt.astype("<u4").tobytes() + dist.astype("<i4").tobytes())
        f.write(struct.pack("<IIQ", max_cost, max_paths, len(searches)))
        f.write(np.array([o for o, _ in searches], dtype="<u4").tobytes() + coff.tobytes())
        f.write(np.array([v for _, c in searches for v, _ in c], dtype="<u4").tobytes())
        f.write(np.array([b for _, c in searches for _, b in c], dtype="<i4").tobytes())


def read_results(path, n):
    b = np.fromfile(path, dtype="<u4")
    at, out = 0, []
    for _ in range(n):
        visited, npaths = int(b[at]), int(b[at + 1])
        at += 2
        paths = []
        for _ in range(npaths):
            l = int(b[at])
            paths.append(b[at + 1:at + 1 + l].tolist())
            at += 1 + l
        out.append((visited, paths))
    assert at == len(b)
    return out


# ---- the small shapes

K = 32
D = -(K - 1)


def ladder(n, lengths=(50, 51), spine=100):
    """s0 -> {a1, b1} -> s1 -> ... -> sn; contigs in the order s0, a1, b1, s1, a2, ...: spine(i) and branch(i, j) give vertices"""
    per = 1 + len(lengths)
    g = Graph([spine] + [l for _ in range(n) for l in list(lengths) + [spine]])
    g.spine = lambda i: 0 if i == 0 else 2 * (per * i)
    g.branch = lambda i, j: 2 * (per * (i - 1) + 1 + j)
    for i in range(1, n + 1):
        for j in range(len(lengths)):
            g.edge(g.spine(i - 1), g.branch(i, j), D)
    for i in range(1, n + 1):
        for j in range(len(lengths)):
            g.edge(g.branch(i, j), g.spine(i), D)
    return g


def along(g, path):
    """the distance at which the last vertex of path starts, from the end of the origin"""
    return sum(D + g.length[v] for v in path[:-1]) + D


class Shape:
    def __init__(self, name, graph, searches, max_cost=MAX_COST, claim=None):
        self.name, self.graph, self.searches, self.max_cost, self.claim = name, graph, searches, max_cost, claim

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return [py_search(self.graph, o, c, self.max_cost) for o, c in self.searches]


@functools.lru_cache(maxsize=None)
def small_shapes():
    shapes = []
    g1 = ladder(1)
    far = along(g1, [g1.branch(1, 1), g1.spine(1)])
    # a single edge; a bound met exactly and one missed by one
    shapes.append(Shape("single_edge", g1, [(0, [(g1.branch(1, 0), D)]), (0, [(g1.branch(1, 0), D - 1)])], claim=[(1, None), (0, None)]))
    shapes.append(Shape("bound_missed_by_one", g1, [(0, [(g1.spine(1), far)]), (0, [(g1.spine(1), far - 1)]), (0, [(g1.spine(1), far - 2)])],
                        claim=[(2, None), (1, None), (0, None)]))
    for n in (1, 3, 8):
        g = ladder(n)
        end = along(g, [v for i in range(1, n + 1) for v in (g.branch(i, 1), g.spine(i))])
        searches = [(0, [(g.spine(n), end)])] + ([(0, [(g.spine(n), end), (g.spine(1), far)])] if n > 1 else [])
        shapes.append(Shape("bubbles_%d" % n, g, searches, claim=[(min(2 ** n, 201), None)] * len(searches)))
    # cost at the exact visit count of the 8-bubble search, one below and one above
    g8 = ladder(8)
    end8 = along(g8, [v for i in range(1, 9) for v in (g8.branch(i, 1), g8.spine(i))])
    visits = py_search(g8, 0, [(g8.spine(8), end8)])[0]
    for delta in (-1, 0, 1):
        shapes.append(Shape("cost_%+d" % delta, g8, [(0, [(g8.spine(8), end8)])], max_cost=visits + delta, claim=[(201 if delta == 1 else None, visits + min(delta, 0))]))
    # backtracking over a satisfied constraint: s1 is satisfied on the a-branch, its bound fails on the b-branch of a longer rung, and
    # the sibling must see it unsatisfied again
    gb = ladder(3, lengths=(50, 70))
    shapes.append(Shape("backtrack", gb, [(0, [(gb.spine(1), along(gb, [gb.branch(1, 0), gb.spine(1)]) + 5),
                                              (gb.spine(3), along(gb, [v for i in (1, 2, 3) for v in (gb.branch(i, 1), gb.spine(i))]))])], claim=[(4, None)]))
    # a vertex listed twice can never be fully satisfied
    shapes.append(Shape("duplicate", g1, [(0, [(g1.spine(1), far), (g1.spine(1), far + 9)])], claim=[(0, None)]))
    # two estimates with equal bounds
    g3 = ladder(3)
    b = along(g3, [g3.branch(1, 1), g3.spine(1), g3.branch(2, 1), g3.spine(2)])
    shapes.append(Shape("equal_bounds", g3, [(0, [(g3.spine(2), b), (g3.spine(1), b)]), (0, [(g3.spine(1), b), (g3.branch(2, 0), b), (g3.spine(2), b)])],
                        claim=[(4, None), (2, None)]))
    # a self-loop on the origin and an inverted edge
    gl = Graph([60, 90])
    gl.edge(0, 0, D)
    gl.edge(0, 2, D)
    shapes.append(Shape("self_loop", gl, [(0, [(2, along(gl, [0, 0, 2]) + 9), (0, D + 9)])], claim=[(2, None)]))
    gi = Graph([70, 55])
    gi.edge(0, 2, D)
    gi.edge(2, 3, D)
    shapes.append(Shape("inverted_edge", gi, [(0, [(1, along(gi, [2, 3, 1]) + 9), (3, along(gi, [2, 3]) + 46)])], claim=[(1, None)]))
    return shapes


@functools.lru_cache(maxsize=None)
def wave_shape(n):
    """n searches on a 17-bubble ladder: one can never be met and runs to the default cost (the constraint on a branch of the last
    rung's other side keeps every path open), the rest take a handful of steps"""
    g = ladder(17)
    end = along(g, [v for i in range(1, 18) for v in (g.branch(i, 1), g.spine(i))])
    hard = (0, [(g.spine(17), end), (g.spine(0) ^ 1, 5000)])
    easy = []
    for i in range(n):
        r = 1 + i % 17
        easy.append((g.spine(r - 1), [(g.spine(r), along(g, [g.branch(r, i % 2), g.spine(r)]) + (i % 3))]))
    if n > 2:
        easy[n // 3] = hard
    return Shape("wave_%d" % n, g, easy)
