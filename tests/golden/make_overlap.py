#!/usr/bin/env python3
"""Regenerates tests/golden/overlap/*: what the UNMODIFIED reference Overlap writes.

It compiles Overlap/Overlap.cpp with Common/*.cpp, Common/city.cc, DataLayer/FastaReader.cpp and DataBase/DB.cc against oracle/shim,
the stand-in Boost headers of make_map.py and make_distanceest.py, and three more written here: boost/ref.hpp (std::ref, std::cref)
and boost/lambda/{lambda,bind}.hpp (a placeholder _1, bind(f, cref, ref, _1) and operator!, all that Overlap.cpp:457-461 uses).
Nothing under oracle/ is changed.

Every input is simulated: a genome cut into contigs, every other one reverse-complemented, with junctions of each kind the program
tells apart, an adjacency graph and distance estimates written here.  cases.json + data.tar.gz hold the inputs and every stdout,
stderr, -o and -g file.  Each case asserts the summary line it is there for, so another seed cannot quietly empty it.

    python tests/golden/make_overlap.py            the goldens and overlap_rules.json
    python tests/golden/make_overlap.py --time     the CPU figure: the reference on the files tools/ov_bench.py times the drop-in on
"""
import json
import os
import random
import re
import shlex
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_map as mm  # noqa: E402
import make_distanceest as md  # noqa: E402
import overlap_golden as og  # noqa: E402

REF = mm.REF
OUT = os.path.join(HERE, "overlap")
RULES_OUT = os.path.join(HERE, "overlap_rules.json")
BOOST = dict(md.BOOST)
BOOST["boost/ref.hpp"] = "#pragma once\n#include <functional>\nnamespace boost { using std::ref; using std::cref; }\n"
BOOST["boost/lambda/lambda.hpp"] = """#pragma once
namespace boost { namespace lambda {
struct placeholder1_ { };
static const placeholder1_ _1 = placeholder1_();
template <class F, class A, class B> struct bound_ {
	F f; A a; B b;
	template <class E> bool operator()(const E& e) const { return f(a.get(), b.get(), e); }
};
template <class T> struct not_ { T t; template <class E> bool operator()(const E& e) const { return !t(e); } };
template <class F, class A, class B> not_<bound_<F, A, B> > operator!(const bound_<F, A, B>& b) { not_<bound_<F, A, B> > n = { b }; return n; }
template <class F, class A, class B> bound_<F, A, B> bind(F f, A a, B b, placeholder1_) { bound_<F, A, B> x = { f, a, b }; return x; }
} }
"""
BOOST["boost/lambda/bind.hpp"] = "#pragma once\n#include <boost/lambda/lambda.hpp>\n"
K = 32


def compile_reference(tmp):
    for name, text in BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-w", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/vendor"]
    srcs = sorted(set(["Common/" + f for f in os.listdir(REF + "/Common") if f.endswith(".cpp")] +
                      ["Common/city.cc", "DataLayer/FastaReader.cpp", "DataBase/DB.cc", "Overlap/Overlap.cpp"]))

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, srcs))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir, exist_ok=True)
    subprocess.run(["g++", "-o", os.path.join(bindir, "Overlap")] + objs + ["-ldl"], check=True)
    return bindir


# ---- simulated inputs -------------------------------------------------------------------------------------------------------------

def rc(s):
    return og.revcomp(s)


class Sim:
    """Contigs laid along a genome.  add(kind) appends the next contig and the junction between it and the one before:
         ('ov', n)      the two share n bases (a true overlap, found when n >= -m)
         ('gap', n)     n bases of the genome lie between them (scaffolded with N, or the single n when the estimate says <= 0)
         ('none', d)    they share nothing and the estimate says d <= 0
         ('homo', n) / ('motif', p, n)   they share a run of n bases of period 1 / p
         ('adj',)       they overlap by k - 1 and the adjacency graph says so: neither end is blunt
       Every other contig is stored reverse-complemented (or those that `flipped` says)."""

    def __init__(self, rng, k=K, flipped=lambda i: i % 2 == 1):
        self.rng, self.k, self.flipped = rng, k, flipped
        self.fwd = []      # the contigs in genome orientation
        self.junctions = []  # (i, i + 1, true distance, sd, kind)
        self.adj = []

    def rand(self, n, avoid=""):
        while True:
            s = mm.rand_seq(self.rng, n)
            if not avoid or (s[0] != avoid[-1] and s[:3] != avoid[-3:]):
                return s

    def first(self, n=300):
        self.fwd.append(self.rand(n))

    def add(self, kind, n=300):
        prev = self.fwd[-1]
        i = len(self.fwd) - 1
        rng = self.rng
        if kind[0] == "ov":
            s = prev[-kind[1]:] + self.rand(n)
            d = -kind[1]
        elif kind[0] == "gap":
            s = self.rand(n)
            d = kind[1]
        elif kind[0] == "none":
            s = self.rand(n, avoid=prev)
            while any(prev[-l:] == s[:l] for l in range(1, 40)):
                s = self.rand(n, avoid=prev)
            d = kind[1]
        elif kind[0] in ("homo", "motif"):
            p = 1 if kind[0] == "homo" else kind[1]
            run = kind[-1]
            unit = mm.rand_seq(rng, p)
            while len(set(unit)) < min(p, 2) or (p > 1 and unit == unit[0] * p) or any(unit == unit[:q] * (p // q) for q in range(1, p) if p % q == 0):
                unit = mm.rand_seq(rng, p)
            rep = (unit * (run // p + 2))[:run]
            # the shared run: prev ends with it and s begins with it; flank with bases that break the period
            brk = [c for c in "ACGT" if c != rep[-p % len(rep)] and c != rep[0] and c != rep[-1]][0]
            self.fwd[-1] = prev[:-run - 1] + brk + rep
            nxt = (unit * (run // p + 3))[run % p:][:p]  # what would continue the period after rep
            brk2 = [c for c in "ACGT" if c != nxt[0]][0]
            s = rep + brk2 + self.rand(n)
            d = -run
        elif kind[0] == "adj":
            s = prev[-(self.k - 1):] + self.rand(n)
            d = -(self.k - 1)
            self.adj.append((i, i + 1))
        else:
            raise ValueError(kind)
        self.fwd.append(s)
        self.junctions.append((i, i + 1, d, kind))

    def stored(self):
        """(name, sequence as stored) and the orientation of each: odd contigs are reverse-complemented"""
        return [(str(i), rc(s) if self.flipped(i) else s) for i, s in enumerate(self.fwd)]

    def node(self, i, flip=False):
        """the vertex name of contig i read along the genome (flip: against it)"""
        sense = self.flipped(i) != flip
        return "%d%s" % (i, "-" if sense else "+")


def adj_text(sim, contigs, cov=50):
    """the ADJ file: "name length coverage\\t; out-edges\\t; in-edges" with the default distance -(k - 1) left unsaid"""
    outs = {i: [[], []] for i in range(len(contigs))}
    for a, b in sim.adj:
        # a -> b along the genome: an out-edge of node(a), and of the complement of node(b) to the complement of node(a)
        na, nb = sim.node(a), sim.node(b)
        outs[a][na.endswith("-")].append(nb if na.endswith("+") else sim.node(b, True))
        ncb = sim.node(b, True)
        outs[b][ncb.endswith("-")].append(sim.node(a, True) if ncb.endswith("+") else sim.node(a))
    lines = []
    for i, (name, s) in enumerate(contigs):
        lines.append("%s %d %d\t;%s\t;%s\n" % (name, len(s), cov * len(s), "".join(" " + v for v in outs[i][0]), "".join(" " + v for v in outs[i][1])))
    return "".join(lines)


def dot_adj_text(sim, contigs, cov=50, k=K):
    lines = ["digraph adj {\n", "graph [k=%d]\n" % k, "edge [d=%d]\n" % -(k - 1)]
    for name, s in contigs:
        for sign in "+-":
            lines.append('"%s%s" [l=%d C=%d]\n' % (name, sign, len(s), cov * len(s)))
    for a, b in sim.adj:
        lines.append('"%s" -> "%s"\n' % (sim.node(a), sim.node(b)))
        lines.append('"%s" -> "%s"\n' % (sim.node(b, True), sim.node(a, True)))
    lines.append("}\n")
    return "".join(lines)


def estimates_of(sim, rng, one_sided=(), duplicated=(), noise=2, sd=3.0, n=20):
    """per contig the estimates of a .dist record: [to the right of the contig as stored], [to its left].  A junction a -> b along
    the genome is seen from a (towards b) and from b (towards a), unless it is in one_sided (then from a only).  A junction in
    `duplicated` is listed twice from a, the second time with another distance."""
    est = {i: ([], []) for i in range(len(sim.fwd))}

    def add(ref, t, h, dd):
        # ref's record holds the estimate: findOverlap(refID, rc, pair) takes t = ref+, h = pair from the first list and t = pair,
        # h = ref+ from the second (Overlap.cpp:338-340)
        if t == "%d+" % ref:
            est[ref][0].append((h, dd, n, sd))
        elif h == "%d+" % ref:
            est[ref][1].append((t, dd, n, sd))
        else:
            raise AssertionError((ref, t, h))
    for idx, (a, b, d, kind) in enumerate(sim.junctions):
        dist = d + (rng.randrange(-noise, noise + 1) if kind[0] == "gap" else 0)
        if kind[0] == "gap":
            dist = max(dist, 1)
        # the junction is the pair (node(a), node(b)) or, the same thing, its complement (node(b)^, node(a)^)
        ta, hb = sim.node(a), sim.node(b)
        pair = (ta, hb) if ta.endswith("+") else (sim.node(b, True), sim.node(a, True))
        add(a, pair[0], pair[1], dist)
        if idx in duplicated:
            add(a, pair[0], pair[1], dist + 1)
        if idx not in one_sided:
            pair = (ta, hb) if hb.endswith("+") else (sim.node(b, True), sim.node(a, True))
            add(b, pair[0], pair[1], dist)
    return est


def dist_text(est):
    lines = []
    for i in sorted(est):
        r, l = est[i]
        if not r and not l:
            continue
        f = lambda e: " %s,%d,%d,%.1f" % e
        lines.append("%d%s ;%s\n" % (i, "".join(f(e) for e in r), "".join(f(e) for e in l)))
    return "".join(lines)


def dot_est_text(est, k=K):
    """the scaffold graph as `abyss-todot --dist -e` gives it: one edge per estimate, u -> v [d= e= n=], parallel edges merged by
    the reader's caller there, so each ordered pair is written once here"""
    lines = ["digraph dist {\n", "graph [k=%d]\n" % k]
    seen = set()
    for i in sorted(est):
        r, l = est[i]
        for (h, d, n, sd) in r:
            if ("%d+" % i, h) not in seen:
                seen.add(("%d+" % i, h))
                lines.append('"%d+" -> "%s" [d=%d e=%.1f n=%d]\n' % (i, h, d, sd, n))
        for (t, d, n, sd) in l:
            # (t, i+) seen from i's other strand is the edge i- -> t^
            u, v = "%d-" % i, t[:-1] + ("-" if t.endswith("+") else "+")
            if (u, v) not in seen:
                seen.add((u, v))
                lines.append('"%s" -> "%s" [d=%d e=%.1f n=%d]\n' % (u, v, d, sd, n))
    lines.append("}\n")
    return "".join(lines)


def build_main(rng):
    """the input most option sets run on: every junction kind, every other contig reverse-complemented"""
    sim = Sim(rng)
    sim.first()
    kinds = [("ov", 5), ("ov", 12), ("ov", K - 2), ("ov", 1), ("ov", 4), ("ov", 3), ("gap", 40), ("gap", 7), ("none", -3), ("none", 0),
             ("homo", 9), ("motif", 2, 10), ("motif", 3, 12), ("motif", 7, 22), ("adj",), ("ov", 8), ("adj",), ("gap", 120), ("ov", 20), ("ov", 2),
             ("homo", 6), ("gap", 15), ("ov", 30)]
    for kd in kinds:
        sim.add(kd, n=rng.randrange(120, 400))
    return sim


def mutate_bytes(contigs, rng):
    """N, IUPAC codes and lower case inside the contigs (away from the ends, and one N at an overlapping end pair)"""
    out = []
    for i, (name, s) in enumerate(contigs):
        s = list(s)
        mid = len(s) // 2
        if i % 3 == 0:
            s[mid] = "N"
        if i % 3 == 1:
            s[mid] = rng.choice("MRWSYKVHDB")
            s[mid + 1] = rng.choice("mrwsykvhdb")
        if i % 4 == 2:
            s[mid - 20:mid - 5] = [c.lower() for c in s[mid - 20:mid - 5]]
        out.append((name, "".join(s)))
    return out


def run(bindir, d, argv):
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"])
    env.pop("COLUMNS", None)
    r = subprocess.run(["Overlap"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return r.returncode, r.stdout, r.stderr


def record(cases, files, bindir, d, inp, suffix, argv, inputs, must_pass=True):
    """argv with OUT_FA / OUT_G standing for the -o and -g files"""
    name = "%s.%s" % (inp, suffix)
    names = {"OUT_FA": "out.fa", "OUT_G": "out.g"}
    real = [names.get(a, a) for a in argv]
    for f in names.values():
        if os.path.exists(os.path.join(d, f)):
            os.remove(os.path.join(d, f))
    st, so, se = run(bindir, d, real)
    assert not must_pass or st == 0, (name, st, se)
    rec = {"name": name, "input": inp, "inputs": inputs, "argv": real, "status": st, "stdout": name + ".stdout", "stderr": se.decode(),
           "out_fa": None, "out_g": None}
    files[name + ".stdout"] = so
    for key, f in (("out_fa", "out.fa"), ("out_g", "out.g")):
        p = os.path.join(d, f)
        if f in real and os.path.exists(p):
            files[name + "." + key] = open(p, "rb").read()
            rec[key] = name + "." + key
    # how many pairs reach findOverlap: its -v lines (Overlap.cpp:168-175), "t<TAB>h" and then the lengths
    if st == 0:
        _, vo, _ = run(bindir, d, ["-v"] + real)
        rec["searched"] = len(re.findall(r"^[^\t\n]+\t[^\t\n]+(?:\t\d+)*$", vo.decode(), re.M))
        for f in names.values():
            if os.path.exists(os.path.join(d, f)):
                os.remove(os.path.join(d, f))
    cases.append(rec)
    return rec, so.decode()


def summary(text):
    return dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^([A-Z][A-Za-z ]+?)(?: \(<\d+bp\))?: (\d+)$", text, re.M))


def make_rules():
    """the Overlap command lines of bin/abyss-pe's -4.fa rule"""
    out = {"_source": "bin/abyss-pe of the reference under `make -n` (tests/golden/make_overlap.py)"}
    runs = [
        ("plain", ["name=asm", "k=64", "in=a1.fq a2.fq", "asm-4.fa"]),
        ("ss_v", ["name=asm", "k=64", "in=a1.fq a2.fq", "SS=--SS", "v=-v", "asm-4.fa"]),
        ("adj_options", ["name=asm", "k=96", "in=a1.fq a2.fq", "graph=adj", "OVERLAP_OPTIONS=--no-scaffold -m8", "asm-4.fa"]),
    ]
    for name, args in runs:
        g = "adj" if "graph=adj" in args else "dot"  # (abyss-pe's default graph format is dot)
        with tempfile.TemporaryDirectory() as td:
            for f in ["a1.fq", "a2.fq", "asm-3.fa", "asm-3." + g, "asm-3.dist"]:
                open(os.path.join(td, f), "w").write("")
                os.utime(os.path.join(td, f), (1, 1) if f.endswith(".fq") else None)
            both = []
            for target in ("asm-4.fa", "asm-4." + g):  # the rule has two targets: asking for either prints the one recipe
                r = subprocess.run(["make", "-n", "-rRf", os.path.join(REF, "bin", "abyss-pe")] + args[:-1] + [target], cwd=td, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE)
                text = r.stdout.decode().replace("\\\n", " ")
                lines = [l for l in text.splitlines() if l.split() and os.path.basename(l.split()[0]) == "Overlap"]
                assert len(lines) == 1, (name, target, r.stdout, r.stderr)
                both.append(lines[0])
            assert both[0] == both[1], both
            argv = shlex.split(lines[0])[1:]
            out[name] = {"make_args": args, "recipe": lines[0], "argv": argv, "targets": ["asm-4.fa", "asm-4." + g]}
    json.dump(out, open(RULES_OUT, "w"), indent=1)
    open(RULES_OUT, "a").write("\n")


def time_reference(bindir, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ov_bench
    ov_bench.write_inputs(tmp, 92_000, 7)
    t0 = time.time()
    subprocess.run([os.path.join(bindir, "Overlap"), "-k64", "-g", "o.adj", "-o", "o.fa", "c.fa", "c.adj", "c.dist"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    print(json.dumps({"contigs": 92_000, "cpus": os.cpu_count(), "seconds": round(time.time() - t0, 2)}))


FORMATS = ["--adj", "--asqg", "--dot", "--gfa", "--gfa1", "--gfa2", "--gv", "--sam"]


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference sources are needed (%s)" % REF)
    rng = random.Random(20261019)
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        bindir = compile_reference(tmp)
        if "--bin" in sys.argv:  # (for looking at the reference by hand: keep the binary)
            import shutil
            shutil.copy(os.path.join(bindir, "Overlap"), sys.argv[sys.argv.index("--bin") + 1])
            return
        if "--time" in sys.argv:
            return time_reference(bindir, tmp)
        files, cases = {}, []
        d = os.path.join(tmp, "work")
        os.makedirs(d)

        def put(name, text):
            data = text if isinstance(text, bytes) else text.encode()
            files[name] = data
            open(os.path.join(d, name), "wb").write(data)

        # ---- main: every junction kind
        sim = build_main(rng)
        contigs = mutate_bytes(sim.stored(), rng)
        dup = [[i for i, j in enumerate(sim.junctions) if j[3][0] == kd][0] for kd in ("homo", "motif", "ov", "none", "gap")]
        one = [i for i, j in enumerate(sim.junctions) if i % 5 == 2]
        est = estimates_of(sim, rng, one_sided=one, duplicated=dup)
        put("main.fa", mm.fasta(contigs))
        put("main.adj", adj_text(sim, contigs))
        put("main.dot", dot_adj_text(sim, contigs))
        put("main.dist", dist_text(est))
        put("main.dist.dot", dot_est_text(est))
        base = ["-k%d" % K, "-g", "OUT_G", "-o", "OUT_FA"]
        ins = ["main.fa", "main.adj", "main.dist"]
        ins_dot = ["main.fa", "main.dot", "main.dist.dot"]
        rec, so = record(cases, files, bindir, d, "main", "default", base + ins, ins)
        s = summary(so)
        assert s["Overlap"] >= 5 and s["Scaffold"] >= 3 and s["No overlap"] >= 2 and s["Insignificant"] >= 3 and s["Homopolymer"] >= 2 \
            and s["Motif"] >= 3, s
        assert b"n" in files["main.default.out_fa"].replace(b"\n", b" ").split(b" ")[-1] or any(
            l.strip() and set(l.strip()) - set(b"ACGTN") for l in files["main.default.out_fa"].splitlines() if not l.startswith(b">")), "no single-n gap contig"
        for suffix, extra in (("v", ["-v"]), ("vv", ["-v", "-v"]), ("m8", ["-m8"]), ("m2", ["--min=2"]), ("no_scaffold", ["--no-scaffold"]),
                              ("no_merge_repeat", ["--no-merge-repeat"]), ("no_merge_repeat_v", ["--no-merge-repeat", "-v"]),
                              ("no_both", ["--no-scaffold", "--no-merge-repeat"]), ("ss", ["--SS"]), ("ss_v", ["--SS", "-v"]),
                              ("no_g", None)):
            if extra is None:
                rec, so2 = record(cases, files, bindir, d, "main", suffix, ["-k%d" % K, "-o", "OUT_FA"] + ins, ins)
                continue
            rec, so2 = record(cases, files, bindir, d, "main", suffix, extra + base + ins, ins)
            s2 = summary(so2)
            if suffix == "m8":
                assert s2["Insignificant"] > s["Insignificant"], (s, s2)
            if suffix == "m2":
                assert s2["Insignificant"] < s["Insignificant"], (s, s2)
            if suffix == "no_scaffold":
                assert s2["Scaffold"] == 0 and s2["Overlap"] >= 5, s2
            if suffix == "no_merge_repeat":
                # a masked pair adds no edge, so its duplicate estimate is searched and counted again
                assert s2["Homopolymer"] + s2["Motif"] > s["Homopolymer"] + s["Motif"], (s, s2)
        for fmt in FORMATS:
            record(cases, files, bindir, d, "main", "fmt" + fmt.replace("--", "_"), [fmt] + base + ins, ins)
        # the other input forms
        record(cases, files, bindir, d, "main", "dotadj", base + ["main.fa", "main.dot", "main.dist"], ["main.fa", "main.dot", "main.dist"])
        rec, so3 = record(cases, files, bindir, d, "main", "dotest", base + ["main.fa", "main.adj", "main.dist.dot"], ["main.fa", "main.adj", "main.dist.dot"])
        assert summary(so3)["Overlap"] >= 5 and summary(so3)["Scaffold"] >= 3, so3
        for suffix, extra in (("dotboth_v", ["-v"]), ("dotboth_vv", ["-v", "-v", "--dot"]), ("dotboth_no_scaffold", ["--no-scaffold"]),
                              ("dotboth_no_merge_repeat", ["--no-merge-repeat"]), ("dotboth_ss", ["--SS", "--gfa2"])):
            record(cases, files, bindir, d, "main", suffix, extra + base + ins_dot, ins_dot)

        # ---- samesense: neighbours stored in the same orientation, so a scaffolded canonical edge can have both senses set (--SS)
        sim4 = Sim(rng, flipped=lambda i: i % 4 in (1, 2))
        sim4.first()
        for kd in (("gap", 30), ("gap", 12), ("ov", 9), ("gap", 50), ("none", -2), ("gap", 25), ("ov", 14), ("gap", 33)):
            sim4.add(kd, n=rng.randrange(120, 300))
        c4 = sim4.stored()
        est4 = estimates_of(sim4, rng)
        put("samesense.fa", mm.fasta(c4))
        put("samesense.adj", adj_text(sim4, c4))
        put("samesense.dist", dist_text(est4))
        put("samesense.dist.dot", dot_est_text(est4))
        ins4 = ["samesense.fa", "samesense.adj", "samesense.dist"]
        rec, so = record(cases, files, bindir, d, "samesense", "default", base + ins4, ins4)
        rec, so4 = record(cases, files, bindir, d, "samesense", "ss", ["--SS"] + base + ins4, ins4)
        assert files["samesense.ss.out_fa"] != files["samesense.default.out_fa"] and summary(so4)["Scaffold"] >= 4, so4
        record(cases, files, bindir, d, "samesense", "ss_v", ["--SS", "-v"] + base + ins4, ins4)
        record(cases, files, bindir, d, "samesense", "ss_dotest_v", ["--SS", "-v", "--dot"] + base + ["samesense.fa", "samesense.adj", "samesense.dist.dot"],
               ["samesense.fa", "samesense.adj", "samesense.dist.dot"])

        # ---- ambiguous: a t with two candidate heads, both overlapping; and one with two scaffolded candidates
        sim2 = Sim(rng)
        sim2.first()
        sim2.add(("ov", 10))
        sim2.add(("gap", 30))
        sim2.add(("ov", 15))
        c2 = sim2.stored()
        est2 = estimates_of(sim2, rng)
        # a second head for contig 0's right end: a new contig that also begins with the last 9 bases of contig 0
        extra_h = sim2.fwd[0][-9:] + mm.rand_seq(rng, 200)
        c2.append((str(len(c2)), extra_h))
        est2[len(c2) - 1] = ([], [])
        est2[0][0].append(("%d+" % (len(c2) - 1), -9, 20, 3.0))
        # and a second, gapped candidate after contig 2 (as stored: even, so its + strand reads along the genome)
        c2.append((str(len(c2)), mm.rand_seq(rng, 250)))
        est2[len(c2) - 1] = ([], [])
        est2[2][0].append(("%d+" % (len(c2) - 1), 25, 20, 3.0))
        sim2.fwd += [extra_h, c2[-1][1]]
        put("ambig.fa", mm.fasta(c2))
        put("ambig.adj", adj_text(sim2, c2))
        put("ambig.dist", dist_text(est2))
        put("ambig.dist.dot", dot_est_text(est2))
        ins2 = ["ambig.fa", "ambig.adj", "ambig.dist"]
        rec, so = record(cases, files, bindir, d, "ambig", "default", base + ins2, ins2)
        assert summary(so)["Ambiguous"] >= 2, so
        record(cases, files, bindir, d, "ambig", "v", ["-v"] + base + ins2, ins2)
        record(cases, files, bindir, d, "ambig", "dotest_vv", ["-v", "-v"] + base + ["ambig.fa", "ambig.adj", "ambig.dist.dot"], ["ambig.fa", "ambig.adj", "ambig.dist.dot"])

        # ---- nosearch: nothing reaches findOverlap (positive estimates beyond the allowed error, non-blunt ends, self pairs)
        sim3 = Sim(rng)
        sim3.first()
        sim3.add(("gap", 200))
        sim3.add(("adj",))
        sim3.add(("gap", 90))
        c3 = sim3.stored()
        est3 = estimates_of(sim3, rng, noise=0)
        est3[0][0].append(("0-", 50, 20, 3.0))  # the same contig: skipped
        put("nosearch.fa", mm.fasta(c3))
        put("nosearch.adj", adj_text(sim3, c3))
        put("nosearch.dist", dist_text(est3))
        put("nosearch.dist.dot", dot_est_text({k2: v for k2, v in est3.items()}).replace('"0+" -> "0-" [d=50 e=3.0 n=20]\n', ""))
        ins3 = ["nosearch.fa", "nosearch.adj", "nosearch.dist"]
        rec, so = record(cases, files, bindir, d, "nosearch", "default", base + ins3, ins3)
        s = summary(so)
        assert s["Scaffold"] >= 2 and s["Overlap"] == s["No overlap"] == s["Insignificant"] == 0, s
        record(cases, files, bindir, d, "nosearch", "v", ["-v"] + base + ins3, ins3)
        record(cases, files, bindir, d, "nosearch", "no_scaffold", ["--no-scaffold"] + base + ins3, ins3)
        record(cases, files, bindir, d, "nosearch", "dotest_v", ["-v"] + base + ["nosearch.fa", "nosearch.adj", "nosearch.dist.dot"],
               ["nosearch.fa", "nosearch.adj", "nosearch.dist.dot"])
        put("empty.dist", "")
        record(cases, files, bindir, d, "nosearch", "empty_dist", base + ["nosearch.fa", "nosearch.adj", "empty.dist"], ["nosearch.fa", "nosearch.adj", "empty.dist"])

        # ---- option and argument errors, --help, --version
        for argv in ([], ["--help"], ["--version"], ["-k32"], ["-o", "x.fa"], ["-k32", "-o", "x.fa", "a", "b"], ["-k32", "-o", "x.fa", "a", "b", "c", "d"],
                     ["-k3x", "-o", "x.fa", "a", "b", "c"], ["-m", "1y", "-k32", "-o", "x.fa", "a", "b", "c"], ["--nonesuch", "-k32", "-o", "x.fa", "a", "b", "c"],
                     ["-k32", "-o", "x.fa", "nosearch.fa", "nonesuch.adj", "nosearch.dist"], ["-k32", "-o", "x.fa", "nosearch.fa", "nosearch.adj", "nonesuch.dist"]):
            st, so, se = run(bindir, d, argv)
            cases.append({"name": "error.argv " + " ".join(argv), "input": "nosearch", "inputs": ["nosearch.fa", "nosearch.adj", "nosearch.dist"], "argv": argv,
                          "status": st, "stdout": None, "stdout_text": so.decode(), "stderr": se.decode(), "out_fa": None, "out_g": None})
            if os.path.exists(os.path.join(d, "x.fa")):
                os.remove(os.path.join(d, "x.fa"))

    mm.OUT = OUT
    mm.write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in cases) + "\n]\n")
    make_rules()
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), len(cases), "cases")


if __name__ == "__main__":
    main()
