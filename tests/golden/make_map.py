#!/usr/bin/env python3
"""Regenerates tests/golden/map/*: abyss-index files and abyss-map output written by the UNMODIFIED reference at -j1.

It compiles Map/map.cc, Map/index.cc and FMIndex/bit_array.cc with the Common and DataLayer sources of oracle/Makefile's REFSRC
against oracle/shim, -DFMBITS=64 and three stand-in Boost headers that it writes into its temporary directory (boost/integer.hpp,
boost/tuple/tuple.hpp, boost/algorithm/string/join.hpp).  Nothing under oracle/ is changed.  Run in the build container (needs the
reference sources):
    python tests/golden/make_map.py            the goldens
    python tests/golden/make_map.py --time     the CPU figure: 200,000 reads of 150 bp against big.fa at -j1 and -j8
"""
import io
import gzip
import json
import os
import random
import subprocess
import sys
import tarfile
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import map_golden as mg  # noqa: E402

REF = os.environ.get("ABYSS_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "map")
SHIM = os.path.join(ROOT, "oracle", "shim")
COMMON = ["FMIndex/bit_array.cc", "Common/Sequence.cpp", "Common/Options.cpp", "Common/Uncompress.cpp", "Common/Fcontrol.cpp",
          "Common/SignalHandler.cpp", "Common/Log.cpp", "DataLayer/FastaReader.cpp", "DataBase/DB.cc"]

BOOST = {
    "boost/integer.hpp": """#pragma once
#include <stdint.h>
namespace boost {
template <int Bits> struct uint_t;
template <> struct uint_t<32> { typedef uint32_t least; };
template <> struct uint_t<64> { typedef uint64_t least; };
template <int Bits> struct int_t;
template <> struct int_t<32> { typedef int32_t least; };
template <> struct int_t<64> { typedef int64_t least; };
}
""",
    "boost/tuple/tuple.hpp": """#pragma once
#include <tuple>
namespace boost {
using std::tie;
template <class A, class B> struct tuple;
template <int N, class A, class B> struct tuple_get_;
template <class A, class B> struct tuple_get_<0, A, B> { static A get(const tuple<A, B>& t) { return t.a; } };
template <class A, class B> struct tuple_get_<1, A, B> { static B get(const tuple<A, B>& t) { return t.b; } };
template <class A, class B> struct tuple {
	A a; B b;
	tuple(A a, B b) : a(a), b(b) { }
	template <int N> auto get() const -> decltype(tuple_get_<N, A, B>::get(*this)) { return tuple_get_<N, A, B>::get(*this); }
};
}
""",
    "boost/algorithm/string/join.hpp": """#pragma once
#include <string>
namespace boost { namespace algorithm {
template <class Seq> std::string join(const Seq& v, const std::string& sep)
{
	std::string s;
	for (typename Seq::const_iterator it = v.begin(); it != v.end(); ++it) { if (it != v.begin()) s += sep; s += *it; }
	return s;
}
} }
""",
}


def compile_reference(tmp):
    for name, text in BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-fopenmp", "-w", "-DFMBITS=64", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/FMIndex", "-I" + REF + "/vendor"]

    def one(src):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, COMMON + ["Map/map.cc", "Map/index.cc"]))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir)
    for main, exe in (("map.cc.o", "abyss-map"), ("index.cc.o", "abyss-index")):
        keep = [o for o in objs if os.path.basename(o) not in ("map.cc.o", "index.cc.o")] + [os.path.join(tmp, main)]
        subprocess.run(["g++", "-fopenmp", "-o", os.path.join(bindir, exe)] + keep + ["-ldl"], check=True)
    return bindir


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def fasta(recs):
    return "".join(">%s\n%s\n" % r for r in recs).encode()


def make_targets(rng):
    t = {}
    big = rand_seq(rng, 40000)
    three = rand_seq(rng, 3000)
    five = rand_seq(rng, 500)
    masked = list(rand_seq(rng, 2000))
    for j in range(300, 420):
        masked[j] = masked[j].lower()
    for j in range(900, 960):
        masked[j] = "N"
    for j in range(1500, 1510):
        masked[j] = "n"
    unit = rand_seq(rng, 12)
    contigs = [("c0", rand_seq(rng, 1)), ("tag1", rand_seq(rng, 2)), ("gattaca", rand_seq(rng, 37)), ("c3", five), ("c4", three),
               ("c5 a comment", big), ("c6", three), ("c7", revcomp(five)), ("c8", big[21000:21800]), ("acgt9", "A" * 700),
               ("c10", (unit * 100)[:1200]), ("tag11", "".join(masked)), ("c12", rand_seq(rng, 4097))]
    t["letters.fa"] = (fasta(contigs), contigs)
    num = [(str(i), rand_seq(rng, n)) for i, n in enumerate([1, 3, 64, 700, 2500, 129])]
    num.append(("6", num[3][1]))
    num.append(("7", revcomp(num[4][1][100:900])))
    t["numeric.fa"] = (fasta(num), num)
    for size in (127, 128, 129, 65539):
        recs = [("0", rand_seq(rng, size // 2 - 3)), ("1", rand_seq(rng, size - (size // 2 - 3) - 8))]
        data = fasta(recs)
        assert len(data) == size, (len(data), size)
        t["edge%d.fa" % size] = (data, recs)
    not_ = [("0", "".join(rng.choice("ACG") for _ in range(300))), ("1", "".join(rng.choice("ACG") for _ in range(77)))]
    t["no_t.fa"] = (fasta(not_), not_)
    return t


def mutate(rng, s, where, to=None):
    s = list(s)
    s[where] = to or rng.choice([c for c in "ACGT" if c != s[where].upper()])
    return "".join(s)


def make_reads(rng, contigs, min_len, long_ok=True):
    """(reads1.fa, reads2.fq): unequal lengths, so the interleave runs one file dry"""
    seqs = [s for _, s in contigs]
    longest = max(seqs, key=len)
    reads = []
    lengths = [1, 2, max(1, min_len - 1), min_len, min_len + 1, 150, 400] + ([3000] if long_ok else [])
    n = 0
    for L in lengths:
        for rep in range(6):
            src = longest if len(longest) >= L else None
            if src is None:
                continue
            at = rng.randrange(0, len(src) - L + 1)
            s = src[at:at + L].upper()
            kind = rep % 6
            if kind == 1:
                s = revcomp(s)
            elif kind == 2:
                s = mutate(rng, s, 0)
            elif kind == 3:
                s = mutate(rng, s, L - 1)
            elif kind == 4:
                s = mutate(rng, s, L // 2, "N" if L > 2 else None)
            elif kind == 5:
                s = revcomp(mutate(rng, s, L // 2)).lower()
            reads.append(("r%d_%d/%d" % (L, rep, 1 + n % 2), ["", "BX:Z:AAC-1", "BX:Z:TTG-1 extra:1", "other:Z:x BX:Z:GG-1"][n % 4], s))
            n += 1
    for _, s in contigs:  # every contig, both strands, as far as a read goes
        reads.append(("w%d/1" % n, "", s[:500].upper()))
        reads.append(("w%d/2" % n, "BX:Z:W-%d" % n, revcomp(s[:500].upper())))
        n += 2
    reads.append(("allN", "", "N" * 60))
    reads.append(("allN1", "", "N"))
    if len(seqs) > 5:
        a, b = seqs[4].upper(), seqs[5].upper()
        reads.append(("join", "", a[-80:] + b[:90]))         # the end of one contig and the start of the next
        reads.append(("joinrc/1", "", revcomp(a[-70:] + b[:70])))
    reads.append(("homo", "", "A" * 150))
    reads.append(("homoT/1", "", "T" * 150))
    reads.append(("lower", "", seqs[-1][:120].lower()))
    reads.append(("mixed", "", "".join(c.lower() if i % 3 else c for i, c in enumerate(seqs[-1][10:210].upper()))))
    rng.shuffle(reads)
    cut = len(reads) * 2 // 3
    fa = "".join(">%s%s\n%s\n" % (i, " " + c if c else "", s) for i, c, s in reads[:cut])
    fq = "".join("@%s%s\n%s\n+\n%s\n" % (i, " " + c if c else "", s, "I" * len(s)) for i, c, s in reads[cut:])
    return fa.encode(), fq.encode()


def make_edge_reads(rng, contigs, count=120):
    """reads of a target of a block or so, cut from its own contigs and short enough to map on both strands: every rank query that
    decides a record falls into the table's first or last block (a text of 127 bytes has 128 rows: its last block holds no symbol)"""
    reads = []
    for n in range(count):
        src = contigs[rng.randrange(len(contigs))][1]
        L = rng.randrange(5, min(40, len(src)) + 1)
        at = rng.choice([0, len(src) - L, rng.randrange(0, len(src) - L + 1)])
        s = src[at:at + L]
        kind = n % 6
        if kind == 1:
            s = revcomp(s)
        elif kind == 2:
            s = mutate(rng, s, L // 2)
        elif kind == 3:
            s = revcomp(mutate(rng, s, rng.randrange(L)))
        elif kind == 4:
            s = mutate(rng, s, rng.randrange(L), "N")
        elif kind == 5:
            s = revcomp(s).lower()
        reads.append(("e%d/%d" % (n, 1 + (n // 6) % 2), s))  # (the mate number decides the strand under --SS)
    for i, (_, s) in enumerate(contigs):  # the whole contigs, which reach the first and the last row of the text
        reads.append(("whole%d/1" % i, s))
        reads.append(("whole%d/2" % i, revcomp(s)))
    rng.shuffle(reads)
    return "".join(">%s\n%s\n" % r for r in reads).encode()


# name, target, queries, options
MAP_CASES = [
    ("letters_l30", "letters.fa", ["reads1.fa", "reads2.fq"], ["-l30"]),
    ("letters_l30_v", "letters.fa", ["reads2.fq", "reads1.fa"], ["-v", "-l30", "--order"]),
    ("letters_l30_ss", "letters.fa", ["reads1.fa", "reads2.fq"], ["-l30", "--SS", "-v"]),
    ("letters_l2000", "letters.fa", ["reads1.fa", "reads2.fq"], ["-l2000"]),
    ("letters_l20_norc", "letters.fa", ["reads1.fa"], ["-k20", "--no-rc"]),
    ("numeric_l1", "numeric.fa", ["nreads1.fa", "nreads2.fq"], ["-l1"]),
    ("numeric_l1_ss", "numeric.fa", ["nreads1.fa", "nreads2.fq"], ["-l1", "--SS", "-v"]),
    ("numeric_l5_norc_C", "numeric.fa", ["nreads1.fa", "nreads2.fq"], ["-l5", "--no-rc", "-C"]),
    ("edge127_l5", "edge127.fa", ["ereads127.fa"], ["-l5", "-v"]),
    ("edge127_l8_ss", "edge127.fa", ["ereads127.fa"], ["-l8", "--SS", "-v"]),
    ("edge127_l6_norc", "edge127.fa", ["ereads127.fa"], ["-l6", "--no-rc"]),
    ("edge128_l5", "edge128.fa", ["ereads128.fa"], ["-l5", "-v"]),
    ("edge128_l8_ss", "edge128.fa", ["ereads128.fa"], ["-l8", "--SS"]),
    ("edge129_l5", "edge129.fa", ["ereads129.fa"], ["-l5", "-v"]),
    ("edge129_l8_ss", "edge129.fa", ["ereads129.fa"], ["-l8", "--SS"]),
    ("edge65539_l20", "edge65539.fa", ["ereads.fa"], ["-l20"]),
    ("no_t_l20", "no_t.fa", ["treads.fa"], ["-l20"]),
    ("big_l30", "big.fa", ["big_reads.fa"], ["-l30", "-v"]),
]
INDEX_TARGETS = ["letters.fa", "numeric.fa", "edge127.fa", "edge128.fa", "edge129.fa", "edge65539.fa", "no_t.fa", "big.fa"]
INDEX_EXTRA = [("numeric_s1", "numeric.fa", ["-s1"]), ("numeric_s7_fa2bwt", "numeric.fa", ["-s7", "--fa2bwt", "--fm"]),
               ("letters_fai_v", "letters.fa", ["--fai", "-v"])]
# argument errors: program, argv, compared on status and stderr
ERRORS = [
    ("abyss-map", []), ("abyss-map", ["only_one"]), ("abyss-map", ["--multi", "a", "b"]), ("abyss-map", ["-l", "x3", "a", "b"]),
    ("abyss-map", ["-j2x", "a", "b"]), ("abyss-map", ["--nonesuch", "a", "b"]),
    ("abyss-index", []), ("abyss-index", ["a", "b"]), ("abyss-index", ["-s", "1x", "a"]), ("abyss-index", ["--nonesuch", "a"]),
]


def run(bindir, prog, argv, cwd):
    env = dict(os.environ, OMP_NUM_THREADS="1", PATH=bindir + os.pathsep + os.environ["PATH"])
    r = subprocess.run([prog] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return r.returncode, r.stdout, r.stderr


def write_data(files):
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.USTAR_FORMAT) as tar:
        for name in sorted(files):
            info = tarfile.TarInfo(name)
            info.size, info.mtime, info.mode = len(files[name]), 0, 0o644
            tar.addfile(info, io.BytesIO(files[name]))
    with open(os.path.join(OUT, "data.tar.gz"), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
            z.write(raw.getvalue())


def time_reference(bindir, tmp):
    work = os.path.join(tmp, "time")
    os.makedirs(work)
    open(os.path.join(work, "big.fa"), "wb").write(mg.big_target())
    open(os.path.join(work, "reads.fa"), "wb").write(mg.big_reads(200000, 150))
    out = {"reads": 200000, "read_length": 150, "target_bytes": len(mg.big_target()), "cpus": os.cpu_count()}
    for j in (1, 8):
        t0 = time.time()
        st, so, se = run(bindir, "abyss-map", ["-j%d" % j, "-l30", "reads.fa", "big.fa"], work)
        assert st == 0, se
        out["seconds_j%d" % j] = round(time.time() - t0, 2)
    print(json.dumps(out))


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference sources are needed (%s)" % REF)
    rng = random.Random(20261018)
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        bindir = compile_reference(tmp)
        if "--time" in sys.argv:
            return time_reference(bindir, tmp)
        files, generated = {}, {"big.fa": mg.big_target(), "big_reads.fa": mg.big_reads()}
        targets = make_targets(rng)
        for name, (data, _) in targets.items():
            files[name] = data
        files["reads1.fa"], files["reads2.fq"] = make_reads(rng, targets["letters.fa"][1], 30)
        files["nreads1.fa"], files["nreads2.fq"] = make_reads(rng, targets["numeric.fa"][1], 5, long_ok=False)
        files["ereads.fa"], _ = make_reads(rng, targets["edge65539.fa"][1], 20)
        files["treads.fa"], _ = make_reads(rng, targets["no_t.fa"][1], 20, long_ok=False)
        for size in (127, 128, 129):  # (drawn last: what was drawn before them stays as it was)
            files["ereads%d.fa" % size] = make_edge_reads(rng, targets["edge%d.fa" % size][1])
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        for name, data in list(files.items()) + list(generated.items()):
            open(os.path.join(work, name), "wb").write(data)
        cases = {"index": [], "map": [], "errors": []}
        for name, target, queries, opts in MAP_CASES:  # (before any index file exists: the reference builds its own)
            argv = ["-j1"] + opts + queries + [target]
            st, out, err = run(bindir, "abyss-map", argv, work)
            assert st == 0, (name, err)
            files[name + ".sam"] = out
            cases["map"].append({"name": name, "target": target, "queries": queries, "argv": argv, "status": st, "sam": name + ".sam",
                                 "sam_sha256": mg.sha256(out), "stderr": err.decode()})
        for target in INDEX_TARGETS:
            st, out, err = run(bindir, "abyss-index", [target], work)
            assert st == 0, (target, err)
            fm, fai = (open(os.path.join(work, target + e), "rb").read() for e in (".fm", ".fai"))
            rec = {"name": target, "target": target, "argv": [target], "status": st, "stderr": err.decode(), "fm_sha256": mg.sha256(fm),
                   "fai_sha256": mg.sha256(fai), "fm": None, "fai": None}
            if target not in generated:
                files[target + ".fm"], files[target + ".fai"] = fm, fai
                rec["fm"], rec["fai"] = target + ".fm", target + ".fai"
            cases["index"].append(rec)
        for name, target, opts in INDEX_EXTRA:
            sub = os.path.join(work, name)
            os.makedirs(sub)
            open(os.path.join(sub, target), "wb").write(files[target])
            st, out, err = run(bindir, "abyss-index", opts + [target], sub)
            assert st == 0, (name, err)
            rec = {"name": name, "target": target, "argv": opts + [target], "status": st, "stderr": err.decode(), "fm": None, "fai": None}
            for e in ("fm", "fai"):
                p = os.path.join(sub, target + "." + e)
                if os.path.exists(p):
                    files["%s.%s" % (name, e)] = open(p, "rb").read()
                    rec[e] = "%s.%s" % (name, e)
                    rec[e + "_sha256"] = mg.sha256(files[rec[e]])
            cases["index"].append(rec)
        # with the index files present the reference's output is the same (checked here, so one SAM serves both)
        for name, target, queries, opts in MAP_CASES[:1] + MAP_CASES[5:6]:
            st, out, err = run(bindir, "abyss-map", ["-j1"] + opts + queries + [target], work)
            assert st == 0 and out == files[name + ".sam"], name
        # stale index files and a wrong version
        stale = os.path.join(work, "stale")
        os.makedirs(stale)
        for kind in ("fm", "fai", "version"):
            for f in os.listdir(stale):
                os.remove(os.path.join(stale, f))
            open(os.path.join(stale, "numeric.fa"), "wb").write(files["numeric.fa"])
            open(os.path.join(stale, "nreads1.fa"), "wb").write(files["nreads1.fa"])
            fm, fai = files["numeric.fa.fm"], files["numeric.fa.fai"]
            if kind == "fm":
                fm = files["no_t.fa.fm"]
            elif kind == "fai":
                fai = files["no_t.fa.fai"]
            else:
                fm = fm.replace(b"FM 64 1", b"FM 32 1", 1)
            open(os.path.join(stale, "numeric.fa.fm"), "wb").write(fm)
            open(os.path.join(stale, "numeric.fa.fai"), "wb").write(fai)
            st, out, err = run(bindir, "abyss-map", ["-j1", "-l5", "nreads1.fa", "numeric.fa"], stale)
            assert st == 1, (kind, st, err)
            cases["errors"].append({"name": "stale_" + kind, "prog": "abyss-map", "argv": ["-j1", "-l5", "nreads1.fa", "numeric.fa"], "status": st,
                                    "stdout": out.decode(), "stderr": err.decode(), "stale": kind})
        for prog, argv in ERRORS:
            st, out, err = run(bindir, prog, argv, work)
            cases["errors"].append({"name": prog + " " + " ".join(argv), "prog": prog, "argv": argv, "status": st, "stdout": out.decode(),
                                    "stderr": err.decode(), "stale": None})
        # reads the reference rejects
        open(os.path.join(work, "at.fa"), "wb").write(b">ok\nACGTACGTAC\n>@bad\nACGTACGTAC\n>after\nACGT\n")
        st, out, err = run(bindir, "abyss-map", ["-j1", "-l5", "at.fa", "numeric.fa"], work)
        files["at.fa"] = b">ok\nACGTACGTAC\n>@bad\nACGTACGTAC\n>after\nACGT\n"
        cases["errors"].append({"name": "id_at", "prog": "abyss-map", "argv": ["-j1", "-l5", "at.fa", "numeric.fa"], "status": st,
                                "stdout": out.decode(), "stderr": err.decode(), "stale": None})
    write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("{\n")
        for i, kind in enumerate(("index", "map", "errors")):
            f.write(' "%s": [\n' % kind)
            f.write(",\n".join("  " + json.dumps(r) for r in cases[kind]))
            f.write("\n ]%s\n" % ("," if i < 2 else ""))
        f.write("}\n")
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), os.path.getsize(os.path.join(OUT, "cases.json")))


if __name__ == "__main__":
    main()
