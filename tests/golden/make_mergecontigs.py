#!/usr/bin/env python3
"""Regenerates tests/golden/mergecontigs/*: what the UNMODIFIED reference MergeContigs writes.

It compiles MergePaths/MergeContigs.cpp with Common/*.cpp, Common/city.cc, DataLayer/FastaReader.cpp, Align/smith_waterman.cpp and
DataBase/DB.cc against oracle/shim and the stand-in Boost headers of make_overlap.py.  Nothing under oracle/ is changed.

cases.json + data.tar.gz hold, for each case, the inputs, argv, stdout, stderr (with the "Using ...B of memory." clause removed), the
status and the -o and -g files.  The families are those of the tests' docstrings: exact overlaps, chained windows, the consensus
rules, gaps, junctions the host redoes, the file handling, the errors and real unitigs.

    python tests/golden/make_mergecontigs.py            the goldens and mergecontigs_rules.json
    python tests/golden/make_mergecontigs.py --time     the CPU figure: the reference on the files tools/mc_bench.py makes
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

REF = mm.REF
OUT = os.path.join(HERE, "mergecontigs")
RULES_OUT = os.path.join(HERE, "mergecontigs_rules.json")
MEMORY = re.compile(rb" Using [^\n]*?B of memory\.")


def compile_reference(tmp):
    for name, text in mo.BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-w", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/Align", "-I" + REF + "/vendor"]
    srcs = sorted(set(["Common/" + f for f in os.listdir(REF + "/Common") if f.endswith(".cpp")] +
                      ["Common/city.cc", "DataLayer/FastaReader.cpp", "DataBase/DB.cc", "Align/smith_waterman.cpp", "MergePaths/MergeContigs.cpp"]))

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, srcs))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir, exist_ok=True)
    subprocess.run(["g++", "-o", os.path.join(bindir, "MergeContigs")] + objs + ["-ldl"], check=True)
    return bindir


# ---- inputs built here -------------------------------------------------------------------------------------------------------------

COMP = bytes.maketrans(b"ACGTacgtMRWSYKVHDBNmrwsykvhdbn", b"TGCAtgcaKYWSRMBDHVNkywsrmbdhvn")


def rc(s):
    return s.translate(COMP)[::-1]


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def comp(v):
    return v[:-1] + ("-" if v.endswith("+") else "+")


class Set:
    """contigs (name, sequence, coverage) and edges between oriented vertices, written once from the tail (and, as ContigGraph holds
    an edge, from the complement of its head)"""

    def __init__(self, k):
        self.k, self.contigs, self.edges, self.paths = k, [], [], []

    def contig(self, name, seq, cov=None):
        self.contigs.append((name, seq, 10 * len(seq) if cov is None else cov))

    def edge(self, u, v, d=None):
        self.edges.append((u, v, -(self.k - 1) if d is None else d))

    def chain(self, rng, prefix, lengths, senses=None, overlaps=None, pid=None):
        """contigs cut from one random sequence so that consecutive ones share overlaps[j] (default k - 1); a '-' contig is stored
        reverse-complemented.  Returns the node names; with pid, adds the path."""
        n = len(lengths)
        senses = senses or "+" * n
        overlaps = overlaps or [self.k - 1] * (n - 1)
        total = sum(lengths) - sum(overlaps)
        genome = dna(rng, total)
        at, names = 0, []
        for j in range(n):
            piece = genome[at:at + lengths[j]]
            self.contig("%s%d" % (prefix, j), piece if senses[j] == "+" else rc(piece))
            names.append("%s%d%s" % (prefix, j, senses[j]))
            if j + 1 < n:
                at += lengths[j] - overlaps[j]
        for j in range(n - 1):
            self.edge(names[j], names[j + 1], -overlaps[j])
        if pid is not None:
            self.paths.append((pid, names))
        return names

    def seq(self, name):
        return next(s for n, s, _ in self.contigs if n == name)

    def set_seq(self, name, seq):
        self.contigs = [(n, seq if n == name else s, c) for n, s, c in self.contigs]

    def fasta(self):
        return b"".join(b">%s %d %d\n%s\n" % (n.encode(), len(s), c, s) for n, s, c in self.contigs)

    def out_edges(self):
        out = {}
        for u, v, d in self.edges:
            out.setdefault(u, []).append((v, d))
            if u != comp(v):
                out.setdefault(comp(v), []).append((comp(u), d))
        return out

    def adj(self):
        out, dflt = self.out_edges(), -(self.k - 1)

        def fmt(lst, flip):
            return "".join(" %s%s" % (comp(v) if flip else v, "" if d == dflt else " [d=%d]" % d) for v, d in lst)
        return "".join("%s %d %d\t;%s\t;%s\n" % (n, len(s), c, fmt(out.get(n + "+", []), False), fmt(out.get(n + "-", []), True))
                       for n, s, c in self.contigs).encode()

    def dot(self):
        out, dflt = self.out_edges(), -(self.k - 1)
        lines = ["digraph adj {\n", "graph [k=%d]\n" % self.k, "edge [d=%d]\n" % dflt]
        for n, s, c in self.contigs:
            for sense in "+-":
                lines.append('"%s%s" [l=%d C=%d]\n' % (n, sense, len(s), c))
        for n, s, c in self.contigs:
            for sense in "+-":
                for v, d in out.get(n + sense, []):
                    lines.append('"%s%s" -> "%s"%s\n' % (n, sense, v, "" if d == dflt else " [d=%d]" % d))
        lines.append("}\n")
        return "".join(lines).encode()

    def path_file(self):
        return "".join("%s\t%s\n" % (pid, " ".join(nodes)) for pid, nodes in self.paths).encode()


# ---- running and recording ---------------------------------------------------------------------------------------------------------

def run(bindir, d, argv, stdin=None):
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"])
    env.pop("COLUMNS", None)
    r = subprocess.run(["MergeContigs"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, input=stdin)
    return r.returncode, r.stdout, r.stderr


class Recorder:
    def __init__(self, bindir, d):
        self.bindir, self.d, self.files, self.cases = bindir, d, {}, []

    def put(self, name, data):
        data = data if isinstance(data, bytes) else data.encode()
        self.files[name] = data
        open(os.path.join(self.d, name), "wb").write(data)

    def put_set(self, stem, s):
        self.put(stem + ".fa", s.fasta())
        self.put(stem + ".adj", s.adj())
        self.put(stem + ".path", s.path_file())
        return [stem + ".fa", stem + ".adj", stem + ".path"]

    def record(self, name, argv, inputs, family, stdin=None, must_pass=True):
        """argv with OUT for the -o file and GRAPH for the -g file; stdin: the name of the input to feed"""
        real = ["out.fa" if a == "OUT" else "out.g" if a == "GRAPH" else a for a in argv]
        for f in ("out.fa", "out.g"):
            if os.path.exists(os.path.join(self.d, f)):
                os.remove(os.path.join(self.d, f))
        st, so, se = run(self.bindir, self.d, real, stdin=self.files[stdin] if stdin else None)
        assert not must_pass or st == 0, (name, st, se)
        rec = {"name": name, "family": family, "inputs": inputs, "argv": real, "stdin": stdin, "status": st, "stdout": None, "stderr": None, "out": None, "graph": None}
        if st < 0:  # an assert or an abort: the drop-in exits 1 after the same lines and a message of its own
            lines = se.decode().splitlines(True)
            cut = next((i for i, l in enumerate(lines) if "Assertion" in l or "terminate called" in l), len(lines))
            se = "".join(lines[:cut]).encode()
            rec["aborts"] = True
        rec["stderr"] = MEMORY.sub(b"", se).decode()
        if so:
            self.files[name + ".stdout"] = so
            rec["stdout"] = name + ".stdout"
        if st == 0:
            for key, f in (("out", "out.fa"), ("graph", "out.g")):
                p = os.path.join(self.d, f)
                if os.path.exists(p):
                    self.files[name + "." + key] = open(p, "rb").read()
                    rec[key] = name + "." + key
        self.cases.append(rec)
        return rec, so, se.decode()


def make_rules():
    """the MergeContigs command lines of bin/abyss-pe's -3.fa and -6.fa rules"""
    out = {"_source": "bin/abyss-pe of the reference under `make -n` (tests/golden/make_mergecontigs.py)"}
    runs = [
        ("contigs", ["name=asm", "k=64", "in=a1.fq a2.fq", "asm-3.fa"], "asm-3.fa", ["asm-2.fa", "asm-2.dot", "asm-2.path"]),
        ("contigs_adj_v", ["name=asm", "k=64", "in=a1.fq a2.fq", "graph=adj", "v=-v", "asm-3.fa"], "asm-3.fa", ["asm-2.fa", "asm-2.adj", "asm-2.path"]),
        ("pe_contigs", ["name=asm", "k=96", "in=a1.fq a2.fq", "asm-6.fa"], "asm-6.fa", ["asm-3.fa", "asm-4.dot", "asm-5.path", "asm-4.fa", "asm-5.fa"]),
    ]
    for name, args, target, inputs in runs:
        with tempfile.TemporaryDirectory() as td:
            for f in ["a1.fq", "a2.fq"] + inputs:
                open(os.path.join(td, f), "w").write("")
                os.utime(os.path.join(td, f), (1, 1) if f.endswith(".fq") else None)
            r = subprocess.run(["make", "-n", "-rRf", os.path.join(REF, "bin", "abyss-pe")] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = r.stdout.decode().replace("\\\n", " ")
            lines = [l for l in text.splitlines() if "MergeContigs" in l.split()]
            assert len(lines) >= 1, (name, r.stdout, r.stderr)
            recipes = []
            for line in lines:  # (the last is the target's own; those before it make its prerequisites)
                words = shlex.split(line)
                argv = words[words.index("MergeContigs") + 1:]
                argv = argv[:next((i for i, w in enumerate(argv) if w in ("|", ">", ";", "&&")), len(argv))]
                recipes.append({"recipe": line, "argv": argv, "target": argv[argv.index("-o") + 1], "stdin": "|" in words[:words.index("MergeContigs")]})
            assert recipes[-1]["target"] == target, (name, lines)
            out[name] = {"make_args": args, "recipes": recipes}
    json.dump(out, open(RULES_OUT, "w"), indent=1)
    open(RULES_OUT, "a").write("\n")


def time_reference(bindir, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mc_bench
    fa, adj, path, k = mc_bench.write_inputs(tmp)
    t0 = time.time()
    subprocess.run([os.path.join(bindir, "MergeContigs"), "-k%d" % k, "-o", "ref.fa", "-g", "ref.dot", fa, adj, path], cwd=tmp, check=True, stderr=subprocess.PIPE)
    seconds = round(time.time() - t0, 2)
    print(json.dumps({"cpus": os.cpu_count(), "seconds": seconds, "fa_sha256": mc_bench.digest(open(os.path.join(tmp, "ref.fa"), "rb").read()),
                      "graph_sha256": mc_bench.digest(open(os.path.join(tmp, "ref.dot"), "rb").read())}))


def real_unitigs(d):
    """the unitigs of tests/pipeline_cases.py:asm() and their graph as the reference's own chain makes them up to Overlap, whose
    edges join blunt unitigs, and the maximal contiguous chains of that graph as paths: (FASTA, ADJ, path file, k)"""
    import pipeline_cases as pc
    if not pc.have_ref():
        sys.exit("the reference binaries of oracle/_ref are needed (abyss_amd.build.build_oracle)")
    work = os.path.join(d, "chain")
    os.makedirs(work)
    ref = pc.tools("ref")
    inp = pc.asm()
    for name, data in inp.files.items():
        pc.write(work, name, data)
    made = pc.chain(ref, ref, work, inp)  # the unitigs, then the contigs Overlap adds; the graph Overlap writes, with its edges
    fa, adj = made["unitigs.fa"] + made["out.fa"], made["out.adj"]
    rows = [l.split(";") for l in adj.decode().splitlines() if l.strip()]
    names = [r[0].split()[0] for r in rows]
    out = {}
    for head, right, left in rows:
        n = head.split()[0]
        out[n + "+"] = re.findall(r"(\S+[+-])(?=\s|$)", right)
        out[n + "-"] = [comp(v) for v in re.findall(r"(\S+[+-])(?=\s|$)", left)]

    def contiguous(u):  # contiguous_out, ContigGraphAlgorithms.h:40-44
        return len(out[u]) == 1 and len(out[comp(out[u][0])]) == 1 and out[u][0][:-1] != u[:-1]
    used, paths, fresh = set(), [], max(int(n) for n in names) + 1
    for n in names:
        u = n + "+"
        if n in used:
            continue
        start, steps = u, 0
        while contiguous(comp(start)) and steps < len(names):  # walk back to the head of the chain
            start, steps = comp(out[comp(start)][0]), steps + 1
        chain = [start]
        while contiguous(chain[-1]) and out[chain[-1]][0][:-1] not in [c[:-1] for c in chain]:
            chain.append(out[chain[-1]][0])
        if len(chain) > 1 and not any(c[:-1] in used for c in chain):
            used.update(c[:-1] for c in chain)
            paths.append((str(fresh), chain))
            fresh += 1
    return fa, adj, "".join("%s\t%s\n" % (pid, " ".join(c)) for pid, c in paths).encode(), pc.K, len(paths)


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

        def base(k):
            return ["-k%d" % k, "-o", "OUT"]

        # ---- 1. exact overlaps: + and - nodes, paths of 2, 3, 4 and 65 nodes, overlaps one below, at and above a wave
        for k in (25, 64, 65, 96):
            s = Set(k)
            s.chain(rng, "a", [150, 130], "+-", pid="p2")
            s.chain(rng, "b", [120, 110, 140], "-+-", pid="p3")
            s.chain(rng, "c", [130, 120, 110, 150], "++-+", pid="p4")
            s.chain(rng, "e", [k + 5 + (j % 7) for j in range(65)], "".join("+-"[(j * 5 // 3) % 2] for j in range(65)), pid="p65")
            s.contig("lone", dna(rng, 210))
            ins = R.put_set("exact%d" % k, s)
            rec, so, se = R.record("exact.k%d" % k, base(k) + ins, ins, 1)
            text = R.files[rec["out"]]
            assert b",...," in text and text.count(b">") == 5 and not se.count("warning"), se
            R.record("exact.k%d_g" % k, base(k) + ["-g", "GRAPH"] + ins, ins, 1)
        s = Set(32)
        s.chain(rng, "a", [90, 80, 100], "+-+", overlaps=[1, 5], pid="short")
        ins = R.put_set("exact_small", s)
        R.record("exact.ov1_ov5", base(32) + ["-g", "GRAPH", "--adj"] + ins, ins, 1)

        # ---- 2. chained windows: a middle contig of length exactly k between two k - 1 overlaps
        k = 25
        s = Set(k)
        s.chain(rng, "m", [80, k, 90], "+++", pid="mid")
        s.chain(rng, "r", [80, k, 90], "+-+", pid="midrc")
        ins = R.put_set("window", s)
        R.record("window.plain", base(k) + ins, ins, 2)
        # the shared part of m0 / m1 / m2 is m1[1 : k - 1]: codes in m0's copy change the first junction's consensus, which the second sees
        m0 = bytearray(s.seq("m0"))
        m0[-10], m0[-11], m0[-12] = ord("N"), ord(chr(m0[-11]).lower()), ord({"A": "R", "C": "Y", "G": "R", "T": "Y"}[chr(m0[-12])])
        m0[-13] = ord(chr(m0[-13]).lower())
        s.set_seq("m0", bytes(m0))
        m2 = bytearray(s.seq("m2"))
        m2[5] = ord("N")
        m2[7] = ord(chr(m2[7]).lower())
        s.set_seq("m2", bytes(m2))
        r1 = bytearray(s.seq("r1"))
        r1[3], r1[9] = ord("N"), ord(chr(r1[9]).lower())
        s.set_seq("r1", bytes(r1))
        ins = R.put_set("window_codes", s)
        rec, so, se = R.record("window.codes", base(k) + ins, ins, 2)
        assert "warning" not in se, se

        # ---- 3. the consensus rules
        k = 25
        s = Set(k)
        code = lambda x: "R" if x in "AG" else "Y"  # the two-base code that covers x
        for tag, (fa, fb) in {"case": (str.lower, str), "na": (lambda x: "N", str), "nb": (str, lambda x: "N"), "lown": (lambda x: "n", str),
                               "ra": (code, str), "ar": (str, code), "both": (lambda x: code(x).lower(), str), "codes": (code, code)}.items():
            s.chain(rng, tag, [70, 75], "++", pid="c_" + tag)
            a, b = bytearray(s.seq(tag + "0")), bytearray(s.seq(tag + "1"))
            for pos in (0, 7, k - 2):  # the first, an inner and the last character of the window
                x = chr(b[pos])
                a[len(a) - (k - 1) + pos], b[pos] = ord(fa(x)), ord(fb(x))
            s.set_seq(tag + "0", bytes(a))
            s.set_seq(tag + "1", bytes(b))
        ins = R.put_set("rules", s)
        rec, so, se = R.record("consensus.rules", base(k) + ins, ins, 3)
        assert "warning" not in se and b"R" in R.files[rec["out"]], se
        s = Set(k)
        s.chain(rng, "x", [70, 75], "++", pid="nonsubset")
        b = bytearray(s.seq("x1"))
        b[7] = ord("R") if chr(s.seq("x0")[-(k - 1) + 7]) in "CT" else ord("Y")
        s.set_seq("x1", bytes(b))
        ins = R.put_set("nonsubset", s)
        R.record("consensus.nonsubset", ["-v", "-v", "-v"] + base(k) + ins, ins, 3)

        # ---- 4. gaps
        def gap_path(s, pid, spec):
            """spec: (name, sense, length) for a contig, n for a gap.  A contig after a gap begins with what the window then holds,
            the gap's Ns filled in, so that every junction has a consensus; the sequence so far is followed as the reference builds it."""
            k, seq, nodes = s.k, b"", []
            for item in spec:
                if isinstance(item, int):
                    run = (b"n" if item < k else b"N") * item
                    seq = (seq + run) if seq else b"N" * (k - 1) + run  # (N gives way: the window keeps its characters)
                    nodes.append("%dN" % item)
                    continue
                name, sense, length = item
                tail = seq[-(k - 1):] if seq else b""
                head = bytes(rng.choice(b"ACGT") if c in b"Nn" else c for c in tail.upper())
                piece = head + dna(rng, length - len(head))
                s.contig(name, piece if sense == "+" else rc(piece))
                nodes.append(name + sense)
                merged = bytes((h + 32 if t in b"acgtn" else h) for t, h in zip(tail, head))
                seq = seq[:len(seq) - len(tail)] + merged + piece[len(head):]
            s.paths.append((pid, nodes))

        for k in (25, 65):
            s = Set(k)
            for n in (1, k - 2, k - 1, k, 200):
                gap_path(s, "gap%d" % n, [("w%d_0" % n, "+", 60 + k), n, ("w%d_1" % n, "-", 60 + k)])
            gap_path(s, "start", [7, ("h0", "+", k + 3)])
            gap_path(s, "between", [("i0", "-", k), 3, ("i1", "+", k), k - 2, ("i2", "+", k + 1), 1, ("i3", "+", k + 2)])
            gap_path(s, "twogaps", [("j0", "+", k + 1), 2, k, ("j1", "-", k + 2)])
            ins = R.put_set("gaps%d" % k, s)
            rec, so, se = R.record("gaps.k%d" % k, base(k) + ins, ins, 4)
            assert b"n" in R.files[rec["out"]] and "warning" not in se, se
            R.record("gaps.k%d_nograph" % k, base(k) + [ins[0], ins[2]], [ins[0], ins[2]], 4, must_pass=False)

        # ---- 5. junctions the host redoes
        k = 41
        s = Set(k)
        s.chain(rng, "ch", [90, 100], "++", pid="chomp")
        s.set_seq("ch0", s.seq("ch0") + b"nn")
        s.chain(rng, "mm", [90, 100], "+-", pid="mismatch")
        a = bytearray(s.seq("mm0"))
        a[-9] = ord("ACGT"[("ACGT".index(chr(a[-9])) + 1) % 4])
        s.set_seq("mm0", bytes(a))
        s.chain(rng, "in", [90, 100], "++", pid="indel")
        b = s.seq("in1")
        s.set_seq("in1", b[:20] + b[21:])
        s.chain(rng, "lo", [90, 100], "++", pid="lowidentity")
        b = bytearray(s.seq("lo1"))
        for i in range(2, 38, 5):
            b[i] = ord("ACGT"[("ACGT".index(chr(b[i])) + 2) % 4])
        s.set_seq("lo1", bytes(b))
        s.chain(rng, "ok", [90, 100, 80], "+-+", pid="fine")
        s.chain(rng, "tw", [90, 100, 95], "+++", pid="twice")  # a failed junction, then the window holds the joined n
        b = bytearray(s.seq("tw1"))
        for i in range(1, 40, 3):
            b[i] = ord("ACGT"[("ACGT".index(chr(b[i])) + 1) % 4])
        s.set_seq("tw1", bytes(b))
        ins = R.put_set("redo", s)
        rec, so, se = R.record("redo.default", base(k) + ins, ins, 5)
        assert se.count("warning: the head of") >= 2, se
        rec, so, se = R.record("redo.vvv", ["-v", "-v", "-v"] + base(k) + ins, ins, 5)
        assert "(good)" in se and "(too low)" in se, se
        s = Set(16)
        s.chain(rng, "few", [60, 70], "++", pid="toofew")
        b = bytearray(s.seq("few1"))
        b[4] = ord("ACGT"[("ACGT".index(chr(b[4])) + 1) % 4])
        s.set_seq("few1", bytes(b))
        ins = R.put_set("redo_few", s)
        rec, so, se = R.record("redo.toofew_vvv", ["-vvv"] + base(16) + ins, ins, 5)
        assert "(too few)" in se, se
        R.record("redo.toofew", base(16) + ins, ins, 5)

        # ---- 6. files
        k = 32
        s = Set(k)
        s.chain(rng, "f", [100, 90, 120, 95], "+-++", pid="900")
        s.chain(rng, "u", [100, 90], "++")
        s.chain(rng, "q", [100, 90, 80], "+++")
        s.contig("drop", dna(rng, 250), cov=0)
        s.contig("keep", dna(rng, 260), cov=100)
        s.edge("keep+", "f0+")
        s.edge("f3+", "keep-")
        s.edge("f3+", "u0+")
        s.paths.append(("drop", []))
        s.paths.append(("u0", ["u0+", "u1+"]))            # an ID that is a contig's name
        s.paths.append(("901", ["q2-", "q1-"]))
        s.paths.append(("902", ["keep-"]))
        fa = s.fasta().replace(b">keep 260 100\n", b">keep\n")
        R.put("files.fa", fa + b">stranger 5 0\nACGTA\n")
        R.put("files.adj", s.adj())
        R.put("files.dot", s.dot())
        R.put("files.path", s.path_file())
        ins = ["files.fa", "files.adj", "files.path"]
        rec, so, se = R.record("files.default", base(k) + ins, ins, 6)
        assert b">stranger" not in R.files[rec["out"]] and b">drop" not in R.files[rec["out"]]
        R.record("files.merged", base(k) + ["--merged"] + ins, ins, 6)
        R.record("files.stdout", ["-k%d" % k] + ins, ins, 6)
        R.record("files.v", ["-v"] + base(k) + ins, ins, 6)
        R.record("files.vv_g", ["-v", "--verbose", "-g", "GRAPH"] + base(k) + ins, ins, 6, must_pass=False)
        R.record("files.stdin_fasta", base(k) + ["-", "files.adj", "files.path"], ins, 6, stdin="files.fa")
        R.record("files.stdin_paths", base(k) + ["files.fa", "files.adj", "-"], ins, 6, stdin="files.path")
        R.put("fresh.path", b"900\tf0+ f1- f2+ f3+\ndrop\n901\tq2- q1-\n")
        for graph in ("adj", "dot"):
            gin = ["files.fa", "files." + graph, "fresh.path"]
            for fmt in ("--adj", "--dot", "--gv", "--dot-meancov", "--gfa", "--gfa1", "--gfa2", "--sam"):
                R.record("files.%s_to%s" % (graph, fmt.lstrip("-")), base(k) + ["-g", "GRAPH", fmt] + gin, gin, 6)
            R.record("files.%s_g_default_v" % graph, ["-v"] + base(k) + ["--graph=GRAPH"] + gin, gin, 6)
        # a palindromic edge at a path end
        s = Set(k)
        names = s.chain(rng, "pal", [100, 90], "++", pid="700")
        half = dna(rng, (k - 1) // 2 + 1)
        pal = (half + rc(half))[:k - 1] if (k - 1) % 2 == 0 else None
        tail = half[:(k - 1 + 1) // 2]
        palin = tail + rc(tail)[(1 if (k - 1) % 2 else 0):]
        s.set_seq("pal1", s.seq("pal1")[:-(k - 1)] + palin[:k - 1])
        s.edge("pal1+", "pal1-")
        s.contig("other", dna(rng, 80))
        ins = R.put_set("palindrome", s)
        R.record("files.palindrome_g", base(k) + ["-g", "GRAPH", "--adj"] + ins, ins, 6, must_pass=False)
        # no graph argument with single-node paths; no paths at all; the coverage lines
        s = Set(k)
        for j in range(3):
            s.contig("s%d" % j, dna(rng, 100 + j))
        s.paths = [("10", ["s0+"]), ("11", ["s2-"])]
        ins = R.put_set("single", s)
        R.record("files.nograph_single", base(k) + [ins[0], ins[2]], [ins[0], ins[2]], 6)
        R.record("files.nograph_single_v", ["-v"] + base(k) + [ins[0], ins[2]], [ins[0], ins[2]], 6)
        R.put("none.path", b"")
        R.record("files.nopaths", base(k) + ["-g", "GRAPH", ins[0], ins[1], "none.path"], [ins[0], ins[1], "none.path"], 6)
        R.record("files.nopaths_v", ["-v"] + base(k) + [ins[0], ins[1], "none.path"], [ins[0], ins[1], "none.path"], 6)
        s = Set(k)
        s.chain(rng, "lowc", [100, 90], "++", pid="20")
        s.contigs = [(n, q, 50 if n == "lowc0" else 700) for n, q, c in s.contigs]
        s.contig("thin", dna(rng, 120), cov=9)
        ins = R.put_set("advice", s)
        rec, so, se = R.record("files.coverage_advice", base(k) + ins, ins, 6)
        assert "Consider increasing" in se, se
        s.contigs = [(n, q, 5000 if n == "thin" else c) for n, q, c in s.contigs]
        ins = R.put_set("noadvice", s)
        rec, so, se = R.record("files.coverage_noadvice", base(k) + ins, ins, 6)
        assert "Consider increasing" not in se and "The minimum coverage" in se, se
        s.contigs = [(n, q, 0) for n, q, c in s.contigs]
        ins = R.put_set("infcov", s)
        rec, so, se = R.record("files.coverage_inf", base(k) + ins, ins, 6)
        assert "inf" in se, se

        # ---- 7. errors: options, arguments and each refusal
        s = Set(k)
        s.chain(rng, "z", [100, 90, 95], "+++", pid="30")
        s.contig("far", dna(rng, 99))
        s.edge("z2+", "far+", 4)
        ins = R.put_set("err", s)
        R.put("noedge.path", b"30\tz0+ z1+ z2+\n31\tz0+ far+\n")
        R.put("positive.path", b"31\tz2+ far+\n")
        R.put("badname.path", b"31\tz0+ z1\n")
        R.put("unknown.path", b"31\tz0+ nonesuch+\n")
        R.put("zerogap.path", b"31\tz0+ 0N z1+\n")
        R.put("empty.fa", b"")
        R.put("shuffled.fa", b"".join(b">%s\n%s\n" % (n.encode(), q) for n, q, c in reversed(s.contigs)))
        R.put("colour.fa", b"".join(b">%s\n%s\n" % (n.encode(), b"0123" * 30) for n, q, c in s.contigs))
        for argv in ([], ["--help"], ["--version"], ["-k32"], ["-k32", "-o", "x.fa", "a"], ["-k32", "-o", "x.fa", "a", "b", "c", "d"], ["-o", "x.fa", "a", "b"],
                     ["-k3x", "-o", "x.fa", "a", "b"], ["-k32", "-g", "", "-o", "x.fa", "a", "b"], ["--nonesuch", "-k32", "-o", "x.fa", "a", "b"],
                     ["--path=p", "-k32", "-o", "x.fa", "a", "b"], ["-k32", "-o", "x.fa", "nonesuch.fa", "err.adj", "err.path"],
                     ["-k32", "-o", "x.fa", "err.fa", "nonesuch.adj", "err.path"], ["-k32", "-o", "x.fa", "err.fa", "err.adj", "nonesuch.path"],
                     ["-v", "-k32", "-o", "x.fa", "err.fa", "err.adj", "nonesuch.path"], ["-k32", "-o", "nonesuch/x.fa", "err.fa", "err.adj", "err.path"],
                     ["-k32", "-o", "x.fa", "err.fa", "err.adj", "noedge.path"], ["-k32", "-o", "x.fa", "err.fa", "err.adj", "positive.path"],
                     ["-k32", "-o", "x.fa", "err.fa", "err.adj", "badname.path"], ["-k32", "-o", "x.fa", "err.fa", "err.adj", "unknown.path"],
                     ["-k32", "-o", "x.fa", "err.fa", "err.adj", "zerogap.path"], ["-k32", "-o", "x.fa", "empty.fa", "err.adj", "err.path"],
                     ["-k32", "-o", "x.fa", "shuffled.fa", "err.adj", "err.path"], ["-k32", "-o", "x.fa", "colour.fa", "err.adj", "err.path"],
                     ["-k32", "-o", "x.fa", "err.fa", "noedge.path"]):
            inputs = [a for a in argv if a in R.files]
            rec, so, se = R.record("error.argv " + " ".join(argv), argv, inputs, 7, must_pass=False)
            if "colour.fa" in argv:  # the reference merges colour-space contigs; the drop-in refuses them
                assert rec["status"] == 0
                rec["refused"] = True
            for f in ("x.fa",):
                if os.path.exists(os.path.join(d, f)):
                    os.remove(os.path.join(d, f))

        # ---- 8. real input: the unitigs of pipeline_cases.asm(), paths the maximal contiguous chains of their graph
        fa, adj, paths, k, npaths = real_unitigs(tmp)
        assert npaths >= 5, npaths
        R.put("asm.fa", fa)
        R.put("asm.adj", adj)
        R.put("asm.path", paths)
        ins = ["asm.fa", "asm.adj", "asm.path"]
        rec, so, se = R.record("asm.default", base(k) + ins, ins, 8)
        assert "warning" not in se, se
        R.record("asm.g_v", ["-v"] + base(k) + ["-g", "GRAPH"] + ins, ins, 8)

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
