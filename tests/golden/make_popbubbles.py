#!/usr/bin/env python3
"""Regenerates tests/golden/popbubbles/*: what the UNMODIFIED reference PopBubbles writes.

It compiles PopBubbles/PopBubbles.cpp with Align/alignGlobal.cc, Common/*.cpp, Common/city.cc, DataLayer/FastaReader.cpp and
DataBase/DB.cc against oracle/shim and the stand-in Boost headers of make_overlap.py, with three stand-ins more, written here: the
depth-first visit PopBubbles' topological sort calls (boost/graph/depth_first_search.hpp, with vector_property_map), and a
boost::lambda that covers the binds of getAlignmentIdentity.  Nothing under oracle/ is changed.

cases.json + data.tar.gz hold, for each case, the inputs, argv, stdout, stderr (with the "Using ...B of memory." clause removed), the
status and the -g file.

    python tests/golden/make_popbubbles.py            the goldens and popbubbles_rules.json
    python tests/golden/make_popbubbles.py --time     the CPU figure: the reference on the files tools/pb_bench.py makes
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
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_map as mm  # noqa: E402
import make_overlap as mo  # noqa: E402
import make_mergecontigs as mmc  # noqa: E402

REF = mm.REF
OUT = os.path.join(HERE, "popbubbles")
RULES_OUT = os.path.join(HERE, "popbubbles_rules.json")
MEMORY = re.compile(rb" Using [^\n]*?B of memory\.")

BOOST = dict(mo.BOOST)
# A depth-first visit as Boost.Graph's: out-edges in the graph's order, a vertex finished when its last out-edge is done.  Kept on an
# explicit stack, as Boost's is, so that a long unambiguous run of contigs does not grow the call stack.
BOOST["boost/graph/depth_first_search.hpp"] = """#pragma once
#include <boost/graph/graph_traits.hpp>
#include <boost/graph/properties.hpp>
#include <utility>
#include <vector>
namespace boost {
struct default_dfs_visitor {
	template <class V, class G> void initialize_vertex(const V&, const G&) { }
	template <class V, class G> void start_vertex(const V&, const G&) { }
	template <class V, class G> void discover_vertex(const V&, const G&) { }
	template <class E, class G> void examine_edge(const E&, const G&) { }
	template <class E, class G> void tree_edge(const E&, const G&) { }
	template <class E, class G> void back_edge(const E&, const G&) { }
	template <class E, class G> void forward_or_cross_edge(const E&, const G&) { }
	template <class E, class G> void finish_edge(const E&, const G&) { }
	template <class V, class G> void finish_vertex(const V&, const G&) { }
};
template <class T, class IndexMap> class vector_property_map {
	std::vector<T>* store_;
	IndexMap index_;
  public:
	typedef T value_type;
	typedef T& reference;
	explicit vector_property_map(unsigned n = 0, const IndexMap& index = IndexMap()) : store_(new std::vector<T>(n)), index_(index) { }
	template <class K> T& operator[](const K& k) const
	{
		const size_t i = get(index_, k);
		if (i >= store_->size()) store_->resize(i + 1);
		return (*store_)[i];
	}
};
template <class T, class I, class K> inline T get(const vector_property_map<T, I>& m, const K& k) { return m[k]; }
template <class T, class I, class K, class V> inline void put(const vector_property_map<T, I>& m, const K& k, const V& v) { m[k] = v; }
template <class T, class I> struct property_traits<vector_property_map<T, I> > { typedef T value_type; };
namespace detail {
struct nontruth2 { template <class A, class B> bool operator()(const A&, const B&) const { return false; } };
template <class G, class Vis, class ColorMap, class Term>
void depth_first_visit_impl(const G& g, typename graph_traits<G>::vertex_descriptor u, Vis& vis, ColorMap color, Term)
{
	typedef typename graph_traits<G>::vertex_descriptor V;
	typedef typename graph_traits<G>::out_edge_iterator Eit;
	typedef typename property_traits<ColorMap>::value_type Color;
	typedef color_traits<Color> C;
	std::vector<std::pair<V, std::pair<Eit, Eit> > > stack;
	put(color, u, C::gray());
	vis.discover_vertex(u, g);
	stack.push_back(std::make_pair(u, out_edges(u, g)));
	while (!stack.empty()) {
		V s = stack.back().first;
		Eit it = stack.back().second.first, last = stack.back().second.second;
		stack.pop_back();
		while (it != last) {
			V v = target(*it, g);
			vis.examine_edge(*it, g);
			const Color c = get(color, v);
			if (c == C::white()) {
				vis.tree_edge(*it, g);
				stack.push_back(std::make_pair(s, std::make_pair(++it, last)));
				s = v;
				put(color, s, C::gray());
				vis.discover_vertex(s, g);
				std::pair<Eit, Eit> r = out_edges(s, g);
				it = r.first;
				last = r.second;
			} else {
				if (c == C::gray()) vis.back_edge(*it, g);
				else vis.forward_or_cross_edge(*it, g);
				++it;
			}
		}
		put(color, s, C::black());
		vis.finish_vertex(s, g);
	}
}
}
}
"""
# boost::lambda as far as PopBubbles.cpp goes: bind(f, a, b, _1), bind(f, a, _1, c), bind(f, a, _1), and the sum of such
BOOST["boost/lambda/lambda.hpp"] = """#pragma once
#include <functional>
namespace boost { using std::ref; using std::cref; }
namespace boost { namespace lambda {
struct placeholder1_ { };
static const placeholder1_ _1 = placeholder1_();
template <class T> inline const T& arg_(const T& t) { return t; }
template <class T> inline T& arg_(const std::reference_wrapper<T>& t) { return t.get(); }
template <class D> struct expr_ { const D& self() const { return static_cast<const D&>(*this); } };
template <class F, class A, class B> struct bind_ab1_ : expr_<bind_ab1_<F, A, B> > {
	F f; A a; B b;
	bind_ab1_(F f, A a, B b) : f(f), a(a), b(b) { }
	template <class X> auto operator()(const X& x) const -> decltype(f(arg_(a), arg_(b), x)) { return f(arg_(a), arg_(b), x); }
};
template <class F, class A, class C> struct bind_a1c_ : expr_<bind_a1c_<F, A, C> > {
	F f; A a; C c;
	bind_a1c_(F f, A a, C c) : f(f), a(a), c(c) { }
	template <class X> auto operator()(const X& x) const -> decltype(f(arg_(a), x, arg_(c))) { return f(arg_(a), x, arg_(c)); }
};
template <class F, class A> struct bind_a1_ : expr_<bind_a1_<F, A> > {
	F f; A a;
	bind_a1_(F f, A a) : f(f), a(a) { }
	template <class X> auto operator()(const X& x) const -> decltype(f(arg_(a), x)) { return f(arg_(a), x); }
};
template <class L, class R> struct sum_ : expr_<sum_<L, R> > {
	L l; R r;
	sum_(const L& l, const R& r) : l(l), r(r) { }
	template <class X> auto operator()(const X& x) const -> decltype(l(x) + r(x)) { return l(x) + r(x); }
};
template <class F, class A, class B> bind_ab1_<F, A, B> bind(F f, A a, B b, placeholder1_) { return bind_ab1_<F, A, B>(f, a, b); }
template <class F, class A, class C> bind_a1c_<F, A, C> bind(F f, A a, placeholder1_, C c) { return bind_a1c_<F, A, C>(f, a, c); }
template <class F, class A> bind_a1_<F, A> bind(F f, A a, placeholder1_) { return bind_a1_<F, A>(f, a); }
template <class L, class R> sum_<L, R> operator+(const expr_<L>& l, const expr_<R>& r) { return sum_<L, R>(l.self(), r.self()); }
} }
"""


def compile_reference(tmp):
    for name, text in BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-w", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/Align", "-I" + REF + "/vendor"]
    srcs = sorted(set(["Common/" + f for f in os.listdir(REF + "/Common") if f.endswith(".cpp")] +
                      ["Common/city.cc", "DataLayer/FastaReader.cpp", "DataBase/DB.cc", "Align/alignGlobal.cc", "PopBubbles/PopBubbles.cpp"]))

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, srcs))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir, exist_ok=True)
    subprocess.run(["g++", "-o", os.path.join(bindir, "PopBubbles")] + objs + ["-ldl"], check=True)
    return bindir


# ---- inputs built here -------------------------------------------------------------------------------------------------------------

rc, dna, Set = mmc.rc, mmc.dna, mmc.Set


def substitute(rng, seq, positions):
    b = bytearray(seq)
    for p in positions:
        b[p] = ord("ACGT"[("ACGT".index(chr(b[p]).upper()) + 1 + rng.randrange(3)) % 4])
    return bytes(b)


def bubble(s, rng, name, middles, covs=None, senses=None, flank=90, left=None, right=None):
    """contigs <name>L and <name>R (or the given ones) and between them one branch a middle, each overlapping both by k - 1; a '-'
    branch is stored reverse-complemented.  Returns (left, branches, right) as vertex names."""
    k = s.k
    if left is None:
        left = name + "L"
        s.contig(left, dna(rng, flank))
    if right is None:
        right = name + "R"
        s.contig(right, dna(rng, flank))
    lseq, rseq = s.seq(left), s.seq(right)
    names = []
    for i, mid in enumerate(middles):
        seq = lseq[-(k - 1):] + mid + rseq[:k - 1]
        sense = senses[i] if senses else "+"
        n = "%sb%d" % (name, i)
        s.contig(n, seq if sense == "+" else rc(seq), None if covs is None else covs[i])
        s.edge(left + "+", n + sense)
        s.edge(n + sense, right + "+")
        names.append(n + sense)
    return left + "+", names, right + "+"


def run(bindir, d, argv):
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"])
    env.pop("COLUMNS", None)
    r = subprocess.run(["PopBubbles"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return r.returncode, r.stdout, r.stderr


class Recorder:
    def __init__(self, bindir, d):
        self.bindir, self.d, self.files, self.cases = bindir, d, {}, []

    def put(self, name, data):
        data = data if isinstance(data, bytes) else data.encode()
        self.files[name] = data
        open(os.path.join(self.d, name), "wb").write(data)

    def put_set(self, stem, s, dot=False):
        self.put(stem + ".fa", s.fasta())
        self.put(stem + (".dot" if dot else ".adj"), s.dot() if dot else s.adj())
        return [stem + ".fa", stem + (".dot" if dot else ".adj")]

    def record(self, name, argv, inputs, family, must_pass=True):
        """argv with GRAPH for the -g file"""
        real = ["out.g" if a == "GRAPH" else "--graph=out.g" if a == "--graph=GRAPH" else a for a in argv]
        if os.path.exists(os.path.join(self.d, "out.g")):
            os.remove(os.path.join(self.d, "out.g"))
        st, so, se = run(self.bindir, self.d, real)
        assert not must_pass or st == 0, (name, st, se)
        rec = {"name": name, "family": family, "inputs": inputs, "argv": real, "status": st, "stdout": None, "stderr": None, "graph": None}
        if st < 0:  # an assert or an abort: the drop-in exits 1 after the same lines and a message of its own
            lines = se.decode().splitlines(True)
            cut = next((i for i, l in enumerate(lines) if "Assertion" in l or "terminate called" in l), len(lines))
            se = "".join(lines[:cut]).encode()
            rec["aborts"] = True
        rec["stderr"] = MEMORY.sub(b"", se).decode()
        if so and st >= 0:
            self.files[name + ".stdout"] = so
            rec["stdout"] = name + ".stdout"
        p = os.path.join(self.d, "out.g")
        if st == 0 and os.path.exists(p):
            self.files[name + ".graph"] = open(p, "rb").read()
            rec["graph"] = name + ".graph"
        self.cases.append(rec)
        return rec, so.decode(), se.decode()


def make_rules():
    """the PopBubbles command lines of bin/abyss-pe's %-2.path rule"""
    out = {"_source": "bin/abyss-pe of the reference under `make -n` (tests/golden/make_popbubbles.py)"}
    runs = [
        ("default", ["name=asm", "k=64", "in=a1.fq a2.fq", "asm-2.path"], ["asm-1.fa", "asm-1.dot", "asm-2.fa", "asm-2.dot"]),
        ("adj_v_a3", ["name=asm", "k=64", "in=a1.fq a2.fq", "graph=adj", "v=-v", "a=3", "j=4", "asm-2.path"], ["asm-1.fa", "asm-1.adj", "asm-2.fa", "asm-2.adj"]),
        ("ss_p95", ["name=asm", "k=96", "in=a1.fq a2.fq", "SS=--SS", "p=0.95", "asm-2.path"], ["asm-1.fa", "asm-1.dot", "asm-2.fa", "asm-2.dot"]),
    ]
    for name, args, inputs in runs:
        with tempfile.TemporaryDirectory() as td:
            for f in ["a1.fq", "a2.fq"] + inputs:
                open(os.path.join(td, f), "w").write("")
                os.utime(os.path.join(td, f), (1, 1) if f.endswith(".fq") else None)
            r = subprocess.run(["make", "-n", "-rRf", os.path.join(REF, "bin", "abyss-pe")] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = r.stdout.decode().replace("\\\n", " ")
            lines = [l for l in text.splitlines() if "PopBubbles" in l.split()]
            assert len(lines) == 1, (name, r.stdout, r.stderr)
            words = shlex.split(lines[0])
            argv = words[words.index("PopBubbles") + 1:]
            cut = next(i for i, w in enumerate(argv) if w.startswith(">"))
            target = argv[cut][1:] or argv[cut + 1]
            out[name] = {"make_args": args, "recipe": lines[0], "argv": argv[:cut], "target": target}
            assert target == "asm-2.path", lines
    json.dump(out, open(RULES_OUT, "w"), indent=1)
    open(RULES_OUT, "a").write("\n")


def time_reference(bindir, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pb_bench
    out = {"cpus": os.cpu_count()}
    for which in ("snp", "long"):
        fa, adj, k = pb_bench.write_inputs(tmp, which)
        t0 = time.time()
        r = subprocess.run([os.path.join(bindir, "PopBubbles"), "-k%d" % k, "-g", "ref.adj", fa, adj], cwd=tmp, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out[which] = {"seconds": round(time.time() - t0, 2), "stdout_sha256": pb_bench.digest(r.stdout),
                      "graph_sha256": pb_bench.digest(open(os.path.join(tmp, "ref.adj"), "rb").read())}
    print(json.dumps(out))


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference sources are needed (%s)" % REF)
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        bindir = compile_reference(tmp)
        if "--time" in sys.argv:
            return time_reference(bindir, tmp)
        d = os.path.join(tmp, "work")
        os.makedirs(d)
        R = Recorder(bindir, d)
        rng = random.Random(20261019)

        # ---- 1. SNP bubbles, and indels of 1 to 70 bases
        for k in (25, 64):
            s = Set(k)
            for j in range(6):
                x = dna(rng, 1)
                bubble(s, rng, "s%d" % j, [x, substitute(rng, x, [0])], covs=[300 + j, 900 - j] if j % 2 else [900, 300], senses="+-" if j % 3 == 0 else "++")
            for n in (1, 2, 5, 17, 33, 64, 70):
                m = dna(rng, 30)
                bubble(s, rng, "i%d" % n, [m, m[:15] + dna(rng, n) + m[15:]], covs=[500, 400])
            s.contig("lone", dna(rng, 200))
            ins = R.put_set("simple%d" % k, s)
            rec, so, se = R.record("simple.k%d" % k, ["-k%d" % k] + ins, ins, 1)
            assert len(so.split()) >= 8, so
            R.record("simple.k%d_g_vv" % k, ["-k%d" % k, "-vv", "-g", "GRAPH"] + ins, ins, 1)
            R.record("simple.k%d_p0" % k, ["-k%d" % k, "-p0", "-v", "-g", "GRAPH"] + ins, ins, 1)
            R.record("simple.k%d_p0_noverbose" % k, ["-k%d" % k, "--identity=0"] + ins, ins, 1)

        # ---- 2. codes, case, ties
        k = 25
        s = Set(k)
        m = dna(rng, 40)
        low = m[:10] + m[10:20].lower() + m[20:]
        code = bytearray(m)
        for p in (3, 17, 31):
            code[p] = ord({"A": "R", "C": "Y", "G": "R", "T": "Y"}[chr(code[p])])
        other = bytearray(m)
        for p in (5, 22):
            other[p] = ord({"A": "Y", "C": "R", "G": "Y", "T": "R"}[chr(other[p])])
        bubble(s, rng, "lc", [m, low])
        bubble(s, rng, "cd", [m, bytes(code)])
        bubble(s, rng, "nc", [bytes(code), bytes(other)])
        bubble(s, rng, "nn", [m, m[:12] + b"NNN" + m[15:]])
        for tag, (a, b) in {"hp": (b"A" * 10, b"A" * 13), "hq": (b"C" * 31, b"C" * 30), "tr": (b"AC" * 8, b"AC" * 10), "tt": (b"ACG" * 9, b"ACG" * 7 + b"AC"),
                            "mix": (b"A" * 9 + m[:9] + b"T" * 8, b"A" * 7 + m[:9] + b"T" * 11)}.items():
            bubble(s, rng, tag, [a, b])
        ins = R.put_set("codes", s)
        R.record("codes.default", ["-k25", "-vv"] + ins, ins, 2)
        R.record("codes.p95_g", ["-k25", "-vvv", "-p0.95", "-g", "GRAPH"] + ins, ins, 2)

        # ---- 3. identity just above and below the threshold: 40 bases between overlaps of 24, d substitutions: (88 - d) / 88
        s = Set(k)
        for dsub in (0, 4, 8, 9, 10, 17, 18):
            m = dna(rng, 40)
            bubble(s, rng, "e%d" % dsub, [m, substitute(rng, m, range(2, 2 + 2 * dsub, 2))])
        for n in (3, 8, 9, 10):  # a length difference alone decides: max_identity, no alignment
            m = dna(rng, 40)
            bubble(s, rng, "l%d" % n, [m, m + dna(rng, n)])
        ins = R.put_set("identity", s)
        for p in ("0.9", "0.8", "0.95", "1", "0.897", "0.8978"):
            R.record("identity.p" + p, ["-k25", "-vv", "-p" + p] + ins, ins, 3)
        R.record("identity.long_option", ["--kmer=25", "--verbose", "--verbose", "--identity=0.85", "--threads=3"] + ins, ins, 3)

        # ---- 4. too long, too many, not simple, palindromes
        s = Set(k)
        m = dna(rng, 30)
        bubble(s, rng, "ok", [m, substitute(rng, m, [4])])
        bubble(s, rng, "lg", [dna(rng, 160), dna(rng, 150)])
        m = dna(rng, 20)
        bubble(s, rng, "t3", [m, substitute(rng, m, [3]), substitute(rng, m, [9])], covs=[100, 300, 200])
        m = dna(rng, 20)
        bubble(s, rng, "t4", [m, substitute(rng, m, [3]), substitute(rng, m, [9]), m[:10] + b"T" + m[10:]], covs=[100, 400, 200, 300])
        # a branch of two contigs in a row; a branch with a way out; branches that end in different places
        l, names, r = bubble(s, rng, "two", [dna(rng, 30)])
        x = dna(rng, 60)
        s.contig("twox", s.seq("twoL")[-24:] + x)
        s.contig("twoy", x[-24:] + dna(rng, 20) + s.seq("twoR")[:24])
        s.edge("twoL+", "twox+"), s.edge("twox+", "twoy+"), s.edge("twoy+", "twoR+")
        l, names, r = bubble(s, rng, "esc", [dna(rng, 30), dna(rng, 31)])
        s.contig("escout", dna(rng, 70))
        s.edge("escb1+", "escout+")
        l, names, r = bubble(s, rng, "open", [dna(rng, 30)])
        s.contig("openz", s.seq("openL")[-24:] + dna(rng, 50))
        s.edge("openL+", "openz+")
        # a palindrome: both branches lead back to the complement of where they came from
        s.contig("palL", dna(rng, 90))
        for j in range(2):
            s.contig("palb%d" % j, dna(rng, 60))
            s.edge("palL+", "palb%d+" % j), s.edge("palb%d+" % j, "palL-")
        ins = R.put_set("shapes", s)
        for extra, tag in (([], "default"), (["-b200"], "b200"), (["-b180"], "b180"), (["-a3"], "a3"), (["-a4"], "a4"), (["--branches=4", "--bubble-length=100"], "a4_b100")):
            R.record("shapes." + tag, ["-k25", "-vvv"] + extra + ["-g", "GRAPH"] + ins, ins, 4)
        R.record("shapes.vvvv", ["-k25", "-vvvv", "-a3"] + ins, ins, 4)
        R.record("shapes.v", ["-k25", "-v", "-a4", "-g", "GRAPH"] + ins, ins, 4)
        R.record("shapes.quiet_a4", ["-k25", "-a4"] + ins, ins, 4)

        # ---- 5. --scaffold, -c, --bubble-graph, --SS
        for opts, tag in ((["--scaffold"], "scaffold"), (["--scaffold", "-a4", "-p0.95"], "scaffold_a4_p95"), (["--scaffold", "--no-scaffold"], "noscaffold"),
                          (["--bubble-graph"], "bubblegraph"), (["--bubble-graph", "--scaffold", "-a3"], "bubblegraph_scaffold"), (["--SS"], "ss"), (["--SS", "--no-SS"], "noss"),
                          (["--SS", "--scaffold"], "ss_scaffold"), (["-c12"], "c12"), (["-c", "9.5", "-a3"], "c9.5"), (["--coverage=1000"], "c1000")):
            R.record("modes." + tag, ["-k25", "-vv"] + opts + ["-g", "GRAPH"] + ins, ins, 5)
        R.record("modes.scaffold_nograph", ["-k25", "--scaffold"] + ins, ins, 5)
        s2 = Set(k)
        s2.contigs, s2.edges = [(n, q, 100 if n.startswith("ok") else c) for n, q, c in s.contigs], list(s.edges)
        ins2 = R.put_set("thin", s2)
        R.record("modes.c_thin", ["-k25", "-v", "-c11"] + ["-g", "GRAPH"] + ins2, ins2, 5)

        # ---- 6. the six formats of -g, from ADJ and from GraphViz
        dots = R.put_set("shapes_dot", s, dot=True)
        for src, tag in ((ins, "adj"), (dots, "dot")):
            for fmt in ("--adj", "--asqg", "--dot", "--gv", "--gfa", "--gfa1", "--gfa2", "--sam"):
                R.record("formats.%s_to%s" % (tag, fmt.lstrip("-")), ["-k25", "-a3", "--graph=GRAPH", fmt] + src, src, 6)
        R.record("formats.dot_v_scaffold", ["-k25", "-v", "--scaffold", "-g", "GRAPH", "--dot"] + dots, dots, 6)

        # ---- 7. errors: options, arguments and each refusal
        R.put("empty.fa", b"")
        R.put("shuffled.fa", b"".join(b">%s\n%s\n" % (n.encode(), q) for n, q, c in reversed(s.contigs)))
        R.put("colour.fa", b"".join(b">%s\n%s\n" % (n.encode(), b"0123" * 30) for n, q, c in s.contigs))
        R.put("short.fa", b"".join(b">%s\n%s\n" % (n.encode(), q[:40] if n == "okb1" else q) for n, q, c in s.contigs))
        R.put("g.gfa", b"H\tVN:Z:1.0\n")
        fa, adj = ins
        for argv in ([], ["--help"], ["--version"], ["-k25"], ["-k25", "a"], ["-k25", "a", "b", "c"], ["a", "b"], ["-k2x", "a", "b"], ["-k25", "-a2x", "a", "b"],
                     ["-k25", "-b1.5", "a", "b"], ["-k25", "-p0.9x", "a", "b"], ["-k25", "-cx", "a", "b"], ["-k25", "-j2x", "a", "b"], ["-k25", "-g", "", fa, adj],
                     ["--nonesuch", "-k25", "a", "b"], ["-k25", "-x", "a", "b"], ["-k25", "nonesuch.fa", adj], ["-k25", "-v", "nonesuch.fa", adj], ["-k25", fa, "nonesuch.adj"],
                     ["-k25", "-v", fa, "nonesuch.adj"], ["-k25", "-p0", "nonesuch.fa", adj], ["-k25", "-g", "nonesuch/out.adj", fa, adj], ["-k25", "empty.fa", adj],
                     ["-k25", "-p0", "empty.fa", adj], ["-k25", "shuffled.fa", adj], ["-k25", "colour.fa", adj], ["-k25", "short.fa", adj], ["-k26", fa, "shapes_dot.dot"]):
            inputs = [a for a in argv if a in R.files]
            rec, so, se = R.record("error.argv " + " ".join(argv), argv, inputs, 7, must_pass=False)
            if "colour.fa" in argv:  # the reference aligns colour-space contigs; the drop-in refuses them
                rec["refused"] = True

        # ---- 8. one long bubble, near 3,000 x 2,900
        s = Set(k)
        m = dna(rng, 3000)
        other = bytearray(substitute(rng, m, rng.sample(range(3000), 150)))
        del other[1200:1290]
        del other[2500:2510]
        bubble(s, rng, "big", [m, bytes(other)], covs=[5000, 9000])
        ins = R.put_set("big", s)
        rec, so, se = R.record("big.vv_g", ["-k25", "-vv", "-g", "GRAPH"] + ins, ins, 8)
        assert "(dissimilar)" not in se and so.split()[0] == "bigb0", (so, se)
        R.record("big.p97", ["-k25", "-vv", "-p0.97"] + ins, ins, 8)

        # ---- 9. real input: the unitigs of pipeline_cases.asm() and the graph the chain makes of them
        fa, adj, paths, kk, npaths = mmc.real_unitigs(tmp)
        R.put("asm.fa", fa)
        R.put("asm.adj", adj)
        ins = ["asm.fa", "asm.adj"]
        R.record("asm.default", ["-k%d" % kk] + ins, ins, 9)
        R.record("asm.vv_g", ["-k%d" % kk, "-vv", "-g", "GRAPH"] + ins, ins, 9)
        R.record("asm.scaffold_a3_g", ["-k%d" % kk, "-v", "--scaffold", "-a3", "-g", "GRAPH", "--dot"] + ins, ins, 9)

        # ---- the chain around it: MergeContigs -> PopBubbles -> MergeContigs, all three the reference's, on the same unitigs
        mcdir = os.path.join(tmp, "mc")
        os.makedirs(mcdir)
        mcbin = os.path.join(mmc.compile_reference(mcdir), "MergeContigs")
        R.put("asm.path", paths)
        pop = os.path.join(bindir, "PopBubbles")
        subprocess.run([mcbin, "-k%d" % kk, "--adj", "-g", "chain.1.adj", "-o", "chain.1.fa", "asm.fa", "asm.adj", "asm.path"], cwd=d, check=True, stderr=subprocess.PIPE)
        r = subprocess.run([pop, "-k%d" % kk, "-g", "chain.2.adj", "chain.1.fa", "chain.1.adj"], cwd=d, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        open(os.path.join(d, "chain.2.path"), "wb").write(r.stdout)
        subprocess.run([mcbin, "-k%d" % kk, "-o", "chain.3.fa", "chain.1.fa", "chain.1.adj", "chain.2.path"], cwd=d, check=True, stderr=subprocess.PIPE)
        for f in ("chain.1.adj", "chain.1.fa", "chain.2.adj", "chain.2.path", "chain.3.fa"):
            R.files[f] = open(os.path.join(d, f), "rb").read()
        R.files["chain.k"] = b"%d\n" % kk

        files, cases = R.files, R.cases
    mm.OUT = OUT
    mm.write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in cases) + "\n]\n")
    make_rules()
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), len(cases), "cases")
    for c in cases:
        if c["status"] != 0:
            print(c["status"], c["name"], "|", c["stderr"].strip().replace("\n", " / ")[:150])


if __name__ == "__main__":
    main()
