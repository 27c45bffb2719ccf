#!/usr/bin/env python3
"""Regenerates tests/golden/simplegraph/*: what the UNMODIFIED reference SimpleGraph writes.

It compiles SimpleGraph/SimpleGraph.cpp with Common/*.cpp, Common/city.cc and DataBase/DB.cc against oracle/shim and the stand-in
Boost headers of make_overlap.py, with -pthread.  Nothing under oracle/ is changed.

The inputs: the graphs and estimates of our own previous stage (the Overlap goldens: what `Overlap -g` wrote next to the .dist it
read), ladders of bubbles built here (a spine contig of 100 between rungs of two branches, 50 and 51 long), small graphs made for one
outcome each (a self-loop, an inverted edge, a bound that holds where the estimate does not, an estimate listed twice, two equal
bounds, a vertex of four out-edges written out of order), and the graph and estimates that the reference's own chain makes from the
real unitigs of tests/pipeline_cases.py:asm().  cases.json + data.tar.gz hold the inputs and every stdout, stderr and -o file.  Each
case asserts the summary line it is there for, so a change here cannot quietly empty it.

    python tests/golden/make_simplegraph.py            the goldens and simplegraph_rules.json
    python tests/golden/make_simplegraph.py --time     the CPU figure: the reference at -j1 and -j16 on the files tools/sg_bench.py makes
"""
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_map as mm  # noqa: E402
import make_overlap as mo  # noqa: E402
import overlap_golden as og  # noqa: E402

REF = mm.REF
OUT = os.path.join(HERE, "simplegraph")
RULES_OUT = os.path.join(HERE, "simplegraph_rules.json")
K = 32
D = -(K - 1)


def compile_reference(tmp):
    for name, text in mo.BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-w", "-pthread", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/vendor"]
    srcs = sorted(set(["Common/" + f for f in os.listdir(REF + "/Common") if f.endswith(".cpp")] +
                      ["Common/city.cc", "DataBase/DB.cc", "SimpleGraph/SimpleGraph.cpp"]))

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, srcs))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir, exist_ok=True)
    subprocess.run(["g++", "-pthread", "-o", os.path.join(bindir, "SimpleGraph")] + objs + ["-ldl"], check=True)
    return bindir


# ---- graphs built here ------------------------------------------------------------------------------------------------------------

class G:
    """contigs (name, length) and edges between oriented vertices; an edge is written once, from its tail (and, as ContigGraph holds
    it, from the complement of its head)"""

    def __init__(self):
        self.contigs, self.edges = [], []

    def contig(self, name, length):
        self.contigs.append((name, length))

    def edge(self, u, v, d=D):
        self.edges.append((u, v, d))

    @staticmethod
    def comp(v):
        return v[:-1] + ("-" if v.endswith("+") else "+")

    def out_edges(self):
        """vertex -> [(target, d)] in the order written, each edge with its complement"""
        out = {}
        for u, v, d in self.edges:
            out.setdefault(u, []).append((v, d))
            if u != self.comp(v):
                out.setdefault(self.comp(v), []).append((self.comp(u), d))
        return out

    def adj(self):
        out = self.out_edges()

        def fmt(lst, flip):
            return "".join(" %s%s" % (self.comp(v) if flip else v, "" if d == D else " [d=%d]" % d) for v, d in lst)
        return "".join("%s %d %d\t;%s\t;%s\n" % (n, l, 10 * l, fmt(out.get(n + "+", []), False), fmt(out.get(n + "-", []), True))
                       for n, l in self.contigs)

    def dot(self):
        out = self.out_edges()
        lines = ["digraph adj {\n", "graph [k=%d]\n" % K, "edge [d=%d]\n" % D]
        for n, l in self.contigs:
            for s in "+-":
                lines.append('"%s%s" [l=%d C=%d]\n' % (n, s, l, 10 * l))
        for n, l in self.contigs:
            for s in "+-":
                for v, d in out.get(n + s, []):
                    lines.append('"%s%s" -> "%s"%s\n' % (n, s, v, "" if d == D else " [d=%d]" % d))
        lines.append("}\n")
        return "".join(lines)

    def length(self, v):
        return dict(self.contigs)[v[:-1]]

    def along(self, origin, path):
        """the distance from the end of origin to the start of the last vertex of path, every edge at the default distance"""
        return sum(D + self.length(v) for v in path[:-1]) + D


def ladder(n, branches=("a", "b"), lengths=(50, 51), order=None):
    """s0 -> {a1, b1} -> s1 -> {a2, b2} -> ... -> sn"""
    g = G()
    g.contig("s0", 100)
    for i in range(1, n + 1):
        for b, l in zip(branches, lengths):
            g.contig("%s%d" % (b, i), l)
        g.contig("s%d" % i, 100)
    for i in range(1, n + 1):
        for b in (order or branches):
            g.edge("s%d+" % (i - 1), "%s%d+" % (b, i))
    for i in range(1, n + 1):
        for b in branches:
            g.edge("%s%d+" % (b, i), "s%d+" % i)
    return g


def adj_to_dot(text, k):
    """an ADJ file as GraphViz: the vertices, then every vertex's out-edges in the order the ADJ reader adds them"""
    rows = [l.split(";") for l in text.decode().splitlines() if l.strip()]
    lines = ["digraph adj {\n", "graph [k=%d]\n" % k, "edge [d=%d]\n" % -(k - 1)]
    for head, _, _ in rows:
        name, length, cov = head.split()
        lines += ['"%s%s" [l=%s C=%s]\n' % (name, s, length, cov) for s in "+-"]
    for head, right, left in rows:
        name = head.split()[0]
        for sense, part in (("+", right), ("-", left)):
            for m in re.finditer(r"(\S+)([+-])(?:\s*\[d=(-?\d+)\])?", part):
                v = m.group(1) + (m.group(2) if sense == "+" else "+-"[m.group(2) == "+"])
                lines.append('"%s%s" -> "%s"%s\n' % (name, sense, v, " [d=%s]" % m.group(3) if m.group(3) else ""))
    lines.append("}\n")
    return "".join(lines)


def dist_line(name, right, left=()):
    f = lambda e: " %s,%d,%d,%.1f" % e
    return "%s%s ;%s\n" % (name, "".join(f(e) for e in right), "".join(f(e) for e in left))


# ---- running and recording ---------------------------------------------------------------------------------------------------------

def run(bindir, d, argv):
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"])
    env.pop("COLUMNS", None)
    r = subprocess.run(["SimpleGraph"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return r.returncode, r.stdout, r.stderr


def summary(text):
    return dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^([A-Z][A-Za-z ]+): (\d+)$", text, re.M))


def record(cases, files, bindir, d, name, argv, inputs, must_pass=True):
    """argv with OUT standing for the -o file.  With -j above 1 the reference writes its lines in the order its threads finish, so
    what is recorded for such a case is the reference's -j1 run: the drop-in takes -j and changes nothing."""
    real = ["out.path" if a == "OUT" else a for a in argv]
    p = os.path.join(d, "out.path")
    if os.path.exists(p):
        os.remove(p)
    st, so, se = run(bindir, d, ["-j1" if re.match(r"-j\d+$", a) else a for a in real])
    assert not must_pass or st == 0, (name, st, se)
    rec = {"name": name, "inputs": inputs, "argv": real, "status": st, "stdout": name + ".stdout", "stderr": se.decode(), "out": None, "searches": 0}
    files[name + ".stdout"] = so
    if st == 0:
        files[name + ".out"] = open(p, "rb").read()
        rec["out"] = name + ".out"
        rec["searches"] = summary(so.decode())["Total paths attempted"]
    cases.append(rec)
    return rec, so.decode()


def make_rules():
    """the SimpleGraph command lines of bin/abyss-pe's -4.path1 rule"""
    out = {"_source": "bin/abyss-pe of the reference under `make -n` (tests/golden/make_simplegraph.py)"}
    runs = [
        ("plain", ["name=asm", "k=64", "in=a1.fq a2.fq", "asm-4.path1"]),
        ("v", ["name=asm", "k=64", "in=a1.fq a2.fq", "v=-v", "asm-4.path1"]),
        ("adj_options", ["name=asm", "k=96", "in=a1.fq a2.fq", "graph=adj", "d=10", "SIMPLEGRAPH_OPTIONS=--no-scaffold --max-cost=5000", "j=4", "asm-4.path1"]),
    ]
    for name, args in runs:
        g = "adj" if "graph=adj" in args else "dot"  # (abyss-pe's default graph format is dot)
        with tempfile.TemporaryDirectory() as td:
            for f in ["a1.fq", "a2.fq", "asm-4." + g, "asm-3.dist"]:
                open(os.path.join(td, f), "w").write("")
                os.utime(os.path.join(td, f), (1, 1) if f.endswith(".fq") else None)
            r = subprocess.run(["make", "-n", "-rRf", os.path.join(REF, "bin", "abyss-pe")] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = r.stdout.decode().replace("\\\n", " ")
            lines = [l for l in text.splitlines() if "SimpleGraph" in l.split()]
            assert len(lines) == 1, (name, r.stdout, r.stderr)
            words = shlex.split(lines[0])
            argv = words[words.index("SimpleGraph") + 1:]
            out[name] = {"make_args": args, "recipe": lines[0], "argv": argv, "target": "asm-4.path1", "inputs": ["asm-4." + g, "asm-3.dist"]}
    json.dump(out, open(RULES_OUT, "w"), indent=1)
    open(RULES_OUT, "a").write("\n")


def time_reference(bindir, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sg_bench
    for variant in ("contigs", "bubbles"):
        adj, dist, k = sg_bench.write_inputs(tmp, variant)
        for j in (1, 16):
            t0 = time.time()
            r = subprocess.run([os.path.join(bindir, "SimpleGraph"), "-k%d" % k, "-j%d" % j, "-o", "o.path", adj, dist], cwd=tmp, check=True, stdout=subprocess.PIPE)
            seconds = round(time.time() - t0, 2)
            paths = open(os.path.join(tmp, "o.path"), "rb").read()
            if j > 1:  # the threads write in the order they finish
                paths = b"".join(sorted(paths.splitlines(True)))
            # the digests are what tools/sg_bench.py prints for the drop-in on the same files (at -j1: the same bytes)
            print(json.dumps({"input": variant, "j": j, "cpus": os.cpu_count(), "seconds": seconds, "path_lines": paths.count(b"\n"),
                              "path_sha256" if j == 1 else "sorted_path_sha256": sg_bench.digest(paths), "stdout_sha256": sg_bench.digest(r.stdout)}))


def real_unitigs(d):
    """-4.dot and -3.dist as the reference's own chain makes them from real unitigs: (graph text, dist text, k)"""
    import pipeline_cases as pc
    if not pc.have_ref():
        sys.exit("the reference binaries of oracle/_ref are needed (abyss_amd.build.build_oracle)")
    work = os.path.join(d, "chain")
    os.makedirs(work)
    ref = pc.tools("ref")
    pc.chain(ref, ref, work, pc.asm())
    o = pc.stage_overlap(ref, work, "unitigs.fa", extra=["--dot"])
    return o["out.adj"], pc.read(work, "lib.dist"), pc.K


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference sources are needed (%s)" % REF)
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        bindir = compile_reference(tmp)
        if "--time" in sys.argv:
            return time_reference(bindir, tmp)
        files, cases = {}, []
        d = os.path.join(tmp, "work")
        os.makedirs(d)

        def put(name, text):
            data = text if isinstance(text, bytes) else text.encode()
            files[name] = data
            open(os.path.join(d, name), "wb").write(data)

        base = ["-k%d" % K, "-o", "OUT"]

        # ---- our own previous stage's files: what Overlap -g wrote and the .dist it read, in ADJ and in GraphViz
        for inp in ("main", "samesense", "ambig"):
            put(inp + ".adj", og.golden(inp + ".default.out_g"))
            put(inp + ".dist", og.golden(inp + ".dist"))
        put("main.dot", og.golden("main.fmt_dot.out_g"))
        ins = ["main.adj", "main.dist"]
        rec, so = record(cases, files, bindir, d, "main.default", base + ins, ins)
        s = summary(so)
        assert (s["Total paths attempted"], s["Unique path"], s["No possible paths"]) == (41, 36, 5), s
        rec, so2 = record(cases, files, bindir, d, "main.dot", base + ["main.dot", "main.dist"], ["main.dot", "main.dist"])
        assert summary(so2) == s and files["main.dot.out"] == files["main.default.out"]
        for suffix, extra in (("v", ["-v"]), ("vv", ["-v", "-v"]), ("dot_vv", None), ("j4", ["-j4"]), ("extend", ["--extend"]), ("extend_v", ["--extend", "-v"]),
                              ("no_scaffold", ["--no-scaffold"]), ("d0", ["-d0"]), ("d0_v", ["-d", "0", "-v"]), ("n", ["-n21"]), ("s", ["-s300"]),
                              ("n_s_v", ["--npairs=21", "--seed-length=300", "--verbose"])):
            if extra is None:
                record(cases, files, bindir, d, "main." + suffix, ["-vv"] + base + ["main.dot", "main.dist"], ["main.dot", "main.dist"])
                continue
            rec, so2 = record(cases, files, bindir, d, "main." + suffix, extra + base + ins, ins)
            s2 = summary(so2)
            if suffix == "j4":
                assert s2 == s and files["main.j4.out"] == files["main.default.out"]
                st4, so4, _ = run(bindir, d, ["-j4", "-k%d" % K, "-o", "out.path"] + ins)  # the threaded run: the same lines in some order
                assert st4 == 0 and summary(so4.decode()) == s
                assert sorted(open(os.path.join(d, "out.path"), "rb").read().splitlines()) == sorted(files["main.default.out"].splitlines())
            if suffix == "s":
                assert s2["Seed too short"] > 0 and s2["Total paths attempted"] < s["Total paths attempted"], s2
            if suffix == "d0_v":
                assert " buffer: 15 " in files["main.v.stdout"].decode() and " buffer: 15 " not in so2 and " buffer: 9 " in so2
        for inp in ("samesense", "ambig"):
            for suffix, extra in (("default", []), ("v", ["-v"])):
                record(cases, files, bindir, d, "%s.%s" % (inp, suffix), extra + base + [inp + ".adj", inp + ".dist"], [inp + ".adj", inp + ".dist"])
            put(inp + ".dot", adj_to_dot(og.golden(inp + ".default.out_g"), K))
            for suffix, extra in (("dot", []), ("dot_v", ["-v"])):
                record(cases, files, bindir, d, "%s.%s" % (inp, suffix), extra + base + [inp + ".dot", inp + ".dist"], [inp + ".dot", inp + ".dist"])
            assert files[inp + ".dot.out"] == files[inp + ".default.out"] and files[inp + ".dot_v.stdout"] == files[inp + ".v.stdout"]
        # -n needs estimates of different support: main's, with every third estimate's pairs cut to 5
        count = [0]

        def thin(m):
            count[0] += 1
            return "%s,%s,%s" % (m.group(1), "5" if count[0] % 3 == 0 else m.group(2), m.group(3))
        put("thin.dist", re.sub(r"(-?\d+),(\d+),(\d+\.\d)", thin, og.golden("main.dist").decode()))
        ins_t = ["main.adj", "thin.dist"]
        rec, so = record(cases, files, bindir, d, "thin.default", base + ins_t, ins_t)
        assert "The minimum number of pairs in a distance estimate is 5." in so, so
        rec, so2 = record(cases, files, bindir, d, "thin.n10", ["-n10"] + base + ins_t, ins_t)
        s2 = summary(so2)
        assert s2["Edges removed"] > 0 and s2["Total paths attempted"] > 0, s2
        record(cases, files, bindir, d, "thin.n10_v", ["-n10", "-v"] + base + ins_t, ins_t)

        # ---- ladders
        for n in (1, 3, 7, 8, 17):
            g = ladder(n)
            put("ladder%d.adj" % n, g.adj())
            put("ladder%d.dot" % n, g.dot())
        for n in (3, 7):
            g = ladder(n)
            short = ["a%d+" % i if j == 0 else "s%d+" % i for i in range(1, n + 1) for j in (0, 1)]
            end = g.along("s0+", short) + n // 2  # between the shortest and the longest way
            put("ladder%d.dist" % n, dist_line("s0", [("s1+", g.along("s0+", ["a1+", "s1+"]), 12, 1.0), ("s%d+" % n, end, 15, 2.0)]))
            for fmt in ("adj", "dot"):
                for suffix, extra in (("default", []), ("v", ["-v"]), ("vv", ["-vv"]), ("no_scaffold", ["--no-scaffold", "-v"]), ("extend", ["--extend", "-v"])):
                    if fmt == "dot" and suffix not in ("default", "v"):
                        continue
                    inputs = ["ladder%d.%s" % (n, fmt), "ladder%d.dist" % n]
                    rec, so = record(cases, files, bindir, d, "ladder%d.%s_%s" % (n, fmt, suffix), extra + base + inputs, inputs)
                    assert summary(so)["Multiple valid paths"] == 1, so
                    line = files[rec["out"]].decode()
                    # the longest way between the spines: n rungs of 51, n - 1 spines of 100, 2n overlaps of k - 1, plus k - 1
                    gap = {3: 198, 7: 554}[n]
                    assert gap == 51 * n + 100 * (n - 1) - (K - 1) * 2 * n + (K - 1)
                    assert line == ("" if suffix == "no_scaffold" else "s0\ts0+ %dN s%d+\n" % (gap, n)), line
        g = ladder(8)
        short = ["a%d+" % i if j == 0 else "s%d+" % i for i in range(1, 9) for j in (0, 1)]
        put("ladder8.dist", dist_line("s0", [("s8+", g.along("s0+", short) + 4, 10, 2.0)]))
        ins8 = ["ladder8.adj", "ladder8.dist"]
        rec, so = record(cases, files, bindir, d, "ladder8.default", base + ins8, ins8)
        assert summary(so)["Too many solutions"] == 1, so
        rec, so = record(cases, files, bindir, d, "ladder8.v", ["-v"] + base + ins8, ins8)
        assert "Paths: 201\n" in so and "(too many solutions)" in so, so[:400]
        record(cases, files, bindir, d, "ladder8.dot_v", ["-v"] + base + ["ladder8.dot", "ladder8.dist"], ["ladder8.dot", "ladder8.dist"])
        rec, so = record(cases, files, bindir, d, "ladder8.cost50", ["--max-cost=50", "-v"] + base + ins8, ins8)
        assert summary(so)["Too complex"] == 1 and "(too complex)" in so, so
        # the >= boundary: the smallest --max-cost at which the reference no longer says "too complex" is the visit count plus one
        lo, hi = 50, 100000
        while hi - lo > 1:
            mid = (lo + hi) // 2
            st, o, e = run(bindir, d, ["--max-cost=%d" % mid, "-k%d" % K, "-o", "out.path"] + ins8)
            if summary(o.decode())["Too complex"] == 1:
                lo = mid
            else:
                hi = mid
        visits = lo
        for c, want in ((visits - 1, "Too complex"), (visits, "Too complex"), (visits + 1, "Too many solutions")):
            rec, so = record(cases, files, bindir, d, "ladder8.cost_%s" % {visits - 1: "below", visits: "exact", visits + 1: "above"}[c],
                             ["--max-cost=%d" % c, "-v"] + base + ins8, ins8)
            assert summary(so)[want] == 1, (c, so)
            rec["visits"] = visits
        # 17 bubbles and an estimate no path can meet (x lies off the ladder): the search runs to the default cost
        g = ladder(17)
        g.contig("x", 80)
        put("ladder17.adj", g.adj())
        short = ["a%d+" % i if j == 0 else "s%d+" % i for i in range(1, 18) for j in (0, 1)]
        put("ladder17.dist", dist_line("s0", [("s17+", g.along("s0+", short) + 8, 10, 2.0), ("x+", 3000, 9, 5.0)]) +
            dist_line("s1", [("s2+", g.along("s1+", ["a2+", "s2+"]), 20, 1.0)], [("s0+", g.along("s0+", ["b1+", "s1+"]), 20, 1.0)]))
        ins17 = ["ladder17.adj", "ladder17.dist"]
        rec, so = record(cases, files, bindir, d, "ladder17.default", base + ins17, ins17)
        assert summary(so)["Too complex"] == 1 and summary(so)["Multiple valid paths"] == 2, so
        record(cases, files, bindir, d, "ladder17.v", ["-v"] + base + ins17, ins17)

        # more searches than a wave has lanes: 150 ladders in one graph, six of them 17 rungs long with an estimate nothing can meet
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import sg_bench
        sg_bench._ladders(d, 150)
        for f, name in (("b.adj", "many.adj"), ("b.dist", "many.dist")):
            put(name, open(os.path.join(d, f), "rb").read())
        insm = ["many.adj", "many.dist"]
        rec, so = record(cases, files, bindir, d, "many.default", base + insm, insm)
        s = summary(so)
        assert s["Total paths attempted"] == 150 and s["Too complex"] == 6 and s["Multiple valid paths"] == 144, s
        record(cases, files, bindir, d, "many.v", ["-v"] + base + insm, insm)

        # ---- one outcome each
        # a self-loop on the seed: r+ -> r+ -> t+.  The estimate to t fits the path r t; r is listed too, and where the path holds it
        # twice it is off the distance map, so its estimate is ignored
        g = G()
        g.contig("r", 60)
        g.contig("t", 90)
        g.edge("r+", "r+")
        g.edge("r+", "t+")
        put("loop.adj", g.adj())
        put("loop.dot", g.dot())
        put("loop.dist", dist_line("r", [("t+", g.along("r+", ["r+", "r+", "t+"]), 11, 1.0), ("r+", D, 7, 1.0)]))
        for fmt in ("adj", "dot"):
            inputs = ["loop." + fmt, "loop.dist"]
            rec, so = record(cases, files, bindir, d, "loop.%s_v" % fmt, ["-v"] + base + inputs, inputs)
            assert summary(so)["Repetitive"] == 1 and "\tignored\n" in so and "Repeat: r+" in so, so
        # an inverted edge: x+ -> u+ -> u- -> x-
        g = G()
        g.contig("x", 70)
        g.contig("u", 55)
        g.edge("x+", "u+")
        g.edge("u+", "u-")
        put("inverted.adj", g.adj())
        put("inverted.dot", g.dot())
        put("inverted.dist", dist_line("x", [("x-", g.along("x+", ["u+", "u-", "x-"]), 8, 1.0), ("u-", g.along("x+", ["u+", "u-"]) + 40, 6, 0.0)]))
        for fmt in ("adj", "dot"):
            inputs = ["inverted." + fmt, "inverted.dist"]
            rec, so = record(cases, files, bindir, d, "inverted.%s_v" % fmt, ["-v"] + base + inputs, inputs)
            assert summary(so)["Repetitive"] == 1 and " ignored\n" in so, so
        # a chain s0 -> m -> t in which several things go wrong, a record each
        g = ladder(1)
        put("chain.dist",
            # the bound holds (it is only an upper one) and the estimate does not: no valid paths
            dist_line("s0", [("s1+", 400, 10, 1.0)]) +
            # listed twice with different distances: the second entry is never found, so nothing is ever a solution
            dist_line("a1", [("s1+", D, 10, 1.0), ("s1+", D + 9, 10, 1.0)]) +
            # missed by one: the bound is one below the distance
            dist_line("b1", [("s1+", D - 10, 10, 1.0)], [("s0+", D, 10, 1.0)]))
        inputs = ["ladder1.adj", "chain.dist"]
        rec, so = record(cases, files, bindir, d, "chain.v", ["-v"] + base + inputs, inputs)
        s = summary(so)
        assert s["No valid paths"] == 1 and s["No possible paths"] == 2 and s["Unique path"] == 1, so
        record(cases, files, bindir, d, "chain.default", base + inputs, inputs)
        # two estimates with equal bounds: d1 + ceil(3 * sd1 + 6) = d2 + ceil(3 * 0 + 6)
        g = ladder(3)
        d1, d2 = g.along("s0+", ["a1+", "s1+"]) + 1, g.along("s0+", ["a1+", "s1+", "b2+", "s2+"]) - 4
        assert (d2 - d1) % 3 == 0, (d1, d2)
        put("equal.dist", dist_line("s0", [("s2+", d2, 10, 0.0), ("s1+", d1, 10, (d2 - d1) / 3.0)]))
        inputs = ["ladder3.adj", "equal.dist"]
        rec, so = record(cases, files, bindir, d, "equal.v", ["-v"] + base + inputs, inputs)
        assert "Constraints: s2+,%d s1+,%d\n" % (d2 + 6, d2 + 6) in so and summary(so)["Multiple valid paths"] == 1, so
        # four out-edges written out of order, four rungs: 256 paths, of which the order of the edges decides the 201 kept
        g = ladder(4, branches=("a", "b", "c", "e"), lengths=(50, 51, 52, 53), order=("c", "a", "e", "b"))
        put("fan.adj", g.adj())
        put("fan.dot", g.dot())
        far = g.along("s0+", [v for i in range(1, 5) for v in ("e%d+" % i, "s%d+" % i)])
        put("fan.dist", dist_line("s0", [("s4+", far - 6, 10, 2.0)]))
        outs = []
        for fmt in ("adj", "dot"):
            inputs = ["fan." + fmt, "fan.dist"]
            rec, so = record(cases, files, bindir, d, "fan.%s_v" % fmt, ["-v"] + base + inputs, inputs)
            assert summary(so)["Too many solutions"] == 1 and "Paths: 201\nc1+ s1+ c2+ s2+ c3+ s3+ c4+ s4+\n" in so, so[:600]
            outs.append(so)
        assert outs[0] == outs[1]

        # ---- real unitigs: the reference's chain on tests/pipeline_cases.py:asm()
        gtext, dtext, k = real_unitigs(tmp)
        put("asm-4.dot", gtext)
        put("asm-3.dist", dtext)
        inputs = ["asm-4.dot", "asm-3.dist"]
        rec, so = record(cases, files, bindir, d, "asm.default", ["-k%d" % k, "-o", "OUT"] + inputs, inputs)
        assert summary(so)["Total paths attempted"] >= 20 and summary(so)["Unique path"] >= 5, so
        record(cases, files, bindir, d, "asm.v", ["-v", "-k%d" % k, "-o", "OUT"] + inputs, inputs)
        record(cases, files, bindir, d, "asm.s_n", ["-s100", "-n12", "-j2", "-k%d" % k, "-o", "OUT"] + inputs, inputs)

        # ---- no search at all: an empty .dist, and one whose every estimate falls to -n
        put("empty.dist", "")
        rec, so = record(cases, files, bindir, d, "nosearch.empty", base + ["ladder1.adj", "empty.dist"], ["ladder1.adj", "empty.dist"])
        assert summary(so)["Total paths attempted"] == 0
        rec, so = record(cases, files, bindir, d, "nosearch.n", ["-n100", "-v"] + base + ["ladder3.adj", "ladder3.dist"], ["ladder3.adj", "ladder3.dist"])
        assert summary(so)["Total paths attempted"] == 0 and summary(so)["Edges removed"] == 2
        rec, so = record(cases, files, bindir, d, "nosearch.s", ["-s101"] + base + ["ladder3.adj", "ladder3.dist"], ["ladder3.adj", "ladder3.dist"])
        assert summary(so)["Total paths attempted"] == 0 and summary(so)["Seed too short"] == 1

        # ---- option and argument errors, --help, --version, an absent file, a contig the graph lacks
        put("stranger.dist", dist_line("s0", [("s1+", 20, 10, 1.0)]) + dist_line("zz", [("s1+", 20, 10, 1.0)]))
        for argv in ([], ["--help"], ["--version"], ["-k32"], ["-o", "x.path"], ["-k32", "-o", "x.path", "a"], ["-k32", "-o", "x.path", "a", "b", "c"],
                     ["-k3x", "-o", "x.path", "a", "b"], ["-n", "1y", "-k32", "-o", "x.path", "a", "b"], ["--max-cost=5x", "-k32", "-o", "x.path", "a", "b"],
                     ["--nonesuch", "-k32", "-o", "x.path", "a", "b"], ["-k32", "-o", "x.path", "nonesuch.adj", "ladder3.dist"],
                     ["-k32", "-o", "x.path", "ladder3.adj", "nonesuch.dist"], ["-v", "-k32", "-o", "x.path", "ladder3.adj", "nonesuch.dist"],
                     ["-k32", "-o", "x.path", "ladder3.adj", "stranger.dist"]):
            st, so, se = run(bindir, d, argv)
            rec = {"name": "error.argv " + " ".join(argv), "inputs": ["ladder3.adj", "ladder3.dist", "stranger.dist"], "argv": argv, "status": st, "stdout": None,
                   "stdout_text": so.decode(), "stderr": se.decode(), "out": None, "searches": 0}
            if st < 0:  # Dictionary::getIndex aborts (Common/Dictionary.h:60-68): the drop-in exits 1 after the same first line
                assert "stranger.dist" in argv and se.decode().startswith("error: unexpected ID: `zz'\n"), (argv, st, se)
                rec["aborts"] = True
            cases.append(rec)
            if os.path.exists(os.path.join(d, "x.path")):
                os.remove(os.path.join(d, "x.path"))

    mm.OUT = OUT
    mm.write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in cases) + "\n]\n")
    make_rules()
    assert any(b"Consider increasing" in v for n, v in files.items() if n.endswith(".stdout")), "no case prints the advice"
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), len(cases), "cases")


if __name__ == "__main__":
    main()
