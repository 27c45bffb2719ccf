#!/usr/bin/env python3
"""Regenerates tests/golden/distanceest/*: what the UNMODIFIED reference DistanceEst writes at -j1.

It compiles Map/map.cc, ParseAligns/abyss-fixmate.cc, DistanceEst/DistanceEst.cpp and DistanceEst/MLE.cpp with Common/*.cpp,
Common/city.cc, DataBase/DB.cc and the Map sources of make_map.py, against oracle/shim, the three stand-in Boost headers of
make_map.py and two more written here (boost/unordered_map.hpp, boost/version.hpp).  Nothing under oracle/ is changed.

Every input is simulated: a genome cut into contigs, read pairs drawn from it, then
    abyss-map -j1 -l40 r1.fa r2.fa contigs.fa | abyss-fixmate -l40 -h HIST | sort -snk3 -k4
and the reference DistanceEst -j1 once per option set.  cases.json + data.tar.gz hold the sorted SAM, the histogram and every
stdout, stderr and output file.  Each case asserts the property it is there for, so another seed cannot quietly empty it.

The `short_frag` case needs an FR pair whose provisional fragment is at most 2(l-1).  With one -l throughout there is none: an
alignment of at least l bases inside its contig puts at least l bases of the fragment on either side of the junction.  So its reads
are mapped and mated with -l20 over contigs two thirds of whose gaps are 300 to 345 bp, with duplicated pairs so that some pairs miss -n,, and DistanceEst runs with -l40: its reader drops the records aligned over fewer than 40 bases, but
the mate of a kept record may be one of them, and its position reaches the fragment through ISIZE.  The reference lowers `ma` to half
the fragment, prints its warnings and exits 0.

    python tests/golden/make_distanceest.py            the goldens and distanceest_rules.json
    python tests/golden/make_distanceest.py --time     the CPU figure: DistanceEst -j1 and -j16 on a SAM of 10 M records
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

REF = mm.REF
OUT = os.path.join(HERE, "distanceest")
RULES_OUT = os.path.join(HERE, "distanceest_rules.json")
BOOST = dict(mm.BOOST)
BOOST["boost/unordered_map.hpp"] = "#pragma once\n#include <unordered_map>\nnamespace boost { using std::unordered_map; }\n"
BOOST["boost/version.hpp"] = "#pragma once\n#define BOOST_VERSION 106000\n"
K, L = 64, 40


def compile_reference(tmp):
    for name, text in BOOST.items():
        p = os.path.join(tmp, "inc", name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "w").write(text)
    flags = ["-std=c++11", "-O2", "-fopenmp", "-w", "-DFMBITS=64", "-include", "getopt.h", "-include", "unistd.h", "-I" + os.path.join(tmp, "inc"),
             "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer", "-I" + REF + "/FMIndex", "-I" + REF + "/vendor"]
    common = sorted(set(mm.COMMON + ["Common/" + f for f in os.listdir(REF + "/Common") if f.endswith(".cpp")] + ["Common/city.cc"]))
    mains = {"Map/map.cc": "abyss-map", "ParseAligns/abyss-fixmate.cc": "abyss-fixmate", "DistanceEst/DistanceEst.cpp": "DistanceEst"}

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = dict(zip(common + list(mains) + ["DistanceEst/MLE.cpp"], ex.map(one, common + list(mains) + ["DistanceEst/MLE.cpp"])))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir)
    for main, exe in mains.items():
        use = [objs[s] for s in common] + [objs[main]] + ([objs["DistanceEst/MLE.cpp"]] if exe == "DistanceEst" else [])
        subprocess.run(["g++", "-fopenmp", "-o", os.path.join(bindir, exe)] + use + ["-ldl"], check=True)
    return bindir


def make_contigs(rng, genome, lo, hi, gap_hi=200, far=None):
    """contigs lo..hi bp along the genome; neighbours overlap by k - 1 or are 1..gap_hi bp apart; every other one reverse-complemented"""
    contigs, at = [], 0
    while at + lo <= len(genome):
        n = min(rng.randrange(lo, hi + 1), len(genome) - at)
        s = genome[at:at + n]
        if len(contigs) % 2:
            s = mm.revcomp(s)
        contigs.append((str(len(contigs)), s))
        if far and len(contigs) % 3 != 1:  # (short_frag: a gap that leaves a spanning fragment only a few bases on either side)
            at += n + rng.randrange(far[0], far[1] + 1)
        else:
            at += n + (-(K - 1) if rng.random() < 0.5 else rng.randrange(1, gap_hi + 1))
    return contigs


def make_pairs(rng, genome, n, mean, sd, outward=False, read=100, dup=0):
    r1, r2, frags = [], [], []
    for i in range(n):
        f = max(read, int(round(rng.gauss(mean, sd))))
        frags.append((rng.randrange(0, len(genome) - f), f))
    frags += [frags[rng.randrange(n)] for _ in range(dup)]
    for i, (p, f) in enumerate(frags):
        a, b = genome[p:p + read], mm.revcomp(genome[p + f - read:p + f])
        if outward:
            a, b = mm.revcomp(a), mm.revcomp(b)
        r1.append(">r%d/1\n%s\n" % (i, a))
        r2.append(">r%d/2\n%s\n" % (i, b))
    return "".join(r1).encode(), "".join(r2).encode()


def pipeline(bindir, work, name, contigs, r1, r2, l=L):
    d = os.path.join(work, name)
    os.makedirs(d)
    open(os.path.join(d, "contigs.fa"), "wb").write(mm.fasta(contigs))
    open(os.path.join(d, "r1.fa"), "wb").write(r1)
    open(os.path.join(d, "r2.fa"), "wb").write(r2)
    env = dict(os.environ, OMP_NUM_THREADS="1", LC_ALL="C", PATH=bindir + os.pathsep + os.environ["PATH"])
    subprocess.run("set -o pipefail; abyss-map -j1 -l%d r1.fa r2.fa contigs.fa | abyss-fixmate -l%d -h lib.hist | sort -snk3 -k4 > lib.sam" % (l, l),
                   shell=True, executable="/bin/bash", cwd=d, env=env, check=True, stderr=subprocess.DEVNULL)
    return d


def run_de(bindir, d, argv, sam="lib.sam", out_file=None):
    env = dict(os.environ, OMP_NUM_THREADS="1", PATH=bindir + os.pathsep + os.environ["PATH"])
    env.pop("COLUMNS", None)
    with open(os.path.join(d, sam), "rb") as f:
        r = subprocess.run(["DistanceEst"] + argv, cwd=d, stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    written = None
    if out_file:
        p = os.path.join(d, out_file)
        written = open(p, "rb").read() if os.path.exists(p) else None
        if written is not None:
            os.remove(p)
    return r.returncode, r.stdout, r.stderr, written


def estimates(dist_text):
    """(target, mate, d, n) of every estimate of a .dist file"""
    out = []
    for line in dist_text.decode().splitlines():
        f = line.split()
        for e in f[1:]:
            if e != ";":
                m, d, n, _ = e.split(",")
                out.append((f[0], m, int(d), int(n)))
    return out


BASE = ["-j1", "-k%d" % K, "-l%d" % L, "-s1000", "-n10"]
# (suffix, argv after -j1; "OUT" stands for the -o file)
FR_OPTS = [
    ("dist", BASE + ["-o", "OUT", "lib.hist"]),
    ("stdout", BASE + ["--dist", "lib.hist"]),
    ("dot", BASE + ["--dot", "lib.hist"]),
    ("gfa", BASE + ["--gfa", "-o", "OUT", "lib.hist"]),
    ("mean", BASE + ["--mean", "lib.hist"]),
    ("median_dot", BASE + ["--dot", "--median", "-o", "OUT", "lib.hist"]),
    ("mean_gfa2", BASE + ["--gfa2", "--mean", "lib.hist"]),
    ("n5", ["-j1", "-k64", "-l40", "-s1000", "-n5", "lib.hist"]),
    ("n30", ["-j1", "-k64", "-l40", "-s1000", "-n30", "lib.hist"]),
    ("s500", ["-j1", "-k64", "-l40", "-s500", "-n10", "lib.hist"]),
    ("q0", BASE + ["-q0", "lib.hist"]),
    ("mind_maxd", BASE + ["--mind=-20", "--maxd=150", "lib.hist"]),
    ("v", BASE + ["-v", "lib.hist"]),
    ("vv_median", BASE + ["-v", "-v", "--median", "lib.hist"]),
    ("rf_forced", BASE + ["--rf", "-v", "lib.hist"]),
    ("vv_dot", BASE + ["-v", "-v", "--dot", "lib.hist"]),
]


def record(cases, files, bindir, d, case, suffix, argv, sam="lib.sam", must_pass=True):
    name = "%s.%s" % (case, suffix)
    out_file = "out.%s" % suffix if "OUT" in argv else None
    argv = [out_file if a == "OUT" else a for a in argv]
    st, so, se, written = run_de(bindir, d, argv, sam, out_file)
    assert not must_pass or st == 0, (name, st, se)
    files[name + ".stdout"] = so
    rec = {"name": name, "input": case, "sam": "%s.%s" % (case, sam), "hist": case + ".lib.hist", "argv": argv, "status": st, "stdout": name + ".stdout",
           "stderr": se.decode(), "out_file": out_file, "out": None}
    if written is not None:
        files[name + ".out"] = written
        rec["out"] = name + ".out"
    cases.append(rec)
    return so if written is None else written, se.decode()


def add_input(files, d, case):
    files[case + ".lib.sam"] = open(os.path.join(d, "lib.sam"), "rb").read()
    files[case + ".lib.hist"] = open(os.path.join(d, "lib.hist"), "rb").read()


def make_rules():
    """the DistanceEst command lines of bin/abyss-pe's -3.dist and -6.dist.dot rules, two libraries with their own _l/_s/_n"""
    out = {"_source": "bin/abyss-pe of the reference under `make -n` (tests/golden/make_distanceest.py)"}
    runs = [
        ("dist_pea", ["name=asm", "k=64", "j=8", "lib=pea peb", "pea=a1.fq a2.fq", "peb=b1.fq b2.fq", "pea_l=45", "pea_s=800", "pea_n=7",
                      "peb_l=50", "peb_s=1200", "peb_n=12", "pea-3.dist"], ["asm-3.fa"]),
        ("dist_peb_v", ["name=asm", "k=64", "j=8", "v=-v", "lib=pea peb", "pea=a1.fq a2.fq", "peb=b1.fq b2.fq", "pea_l=45", "pea_s=800", "pea_n=7",
                        "peb_l=50", "peb_s=1200", "peb_n=12", "peb-3.dist"], ["asm-3.fa"]),
        ("dist_defaults", ["name=asm", "k=96", "j=2", "in=a1.fq a2.fq", "DISTANCEEST_OPTIONS=--mind=-50", "asm-3.dist"], ["asm-3.fa"]),
        ("dist_from_sam_gz", ["name=asm", "k=64", "j=8", "lib=pea", "pea=a1.fq a2.fq", "pea-3.dist"], ["asm-3.fa", "pea-3.sam.gz", "pea-3.hist"]),
        ("scaffold_mpa", ["name=asm", "k=64", "j=8", "lib=pea", "pea=a1.fq a2.fq", "mp=mpa mpb", "mpa=m1.fq m2.fq", "mpb=n1.fq n2.fq", "mpa_l=60",
                          "mpb_scaf_s=2000", "mpb_scaf_n=4", "mpa-6.dist.dot"], ["asm-6.fa"]),
        ("scaffold_mpb", ["name=asm", "k=64", "j=8", "lib=pea", "pea=a1.fq a2.fq", "mp=mpa mpb", "mpa=m1.fq m2.fq", "mpb=n1.fq n2.fq", "mpa_l=60",
                          "mpb_scaf_s=2000", "mpb_scaf_n=4", "mpb-6.dist.dot"], ["asm-6.fa"]),
    ]
    for name, args, touch in runs:
        with tempfile.TemporaryDirectory() as td:
            for f in touch + ["a1.fq", "a2.fq", "b1.fq", "b2.fq", "m1.fq", "m2.fq", "n1.fq", "n2.fq"]:
                open(os.path.join(td, f), "w").write("")
                os.utime(os.path.join(td, f), (1, 1) if f.endswith(".fq") or f.endswith(".fa") else None)
            r = subprocess.run(["make", "-n", "-rRf", os.path.join(REF, "bin", "abyss-pe")] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = r.stdout.decode().replace("\\\n", " ")
            lines = [l for l in text.splitlines() if "DistanceEst" in l and "-o " + args[-1] in l]
            assert len(lines) == 1, (name, r.stdout, r.stderr)
            part = [p for p in lines[0].split("|") if "DistanceEst" in p][0]
            argv = shlex.split(part)
            argv = argv[[os.path.basename(a) for a in argv].index("DistanceEst") + 1:]
            out[name] = {"make_args": args, "recipe": lines[0], "argv": argv}
    json.dump(out, open(RULES_OUT, "w"), indent=1)
    open(RULES_OUT, "a").write("\n")


def time_reference(bindir, tmp):
    """the unmodified reference at -j1 and -j16 on the SAM that tools/de_bench.py times the drop-in on"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import de_bench
    sam, hist = os.path.join(tmp, "big.sam"), os.path.join(tmp, "big.hist")
    n = de_bench.write_sam(sam, hist, 10_000_000, 92_000, 7)
    out = {"records": n, "cpus": os.cpu_count()}
    for j in (1, 16):
        t0 = time.time()
        with open(sam, "rb") as f:
            subprocess.run([os.path.join(bindir, "DistanceEst"), "-j%d" % j, "-k64", "-l40", "-s1000", "-n10", "-o", os.path.join(tmp, "o%d.dist" % j), hist],
                           stdin=f, check=True)
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
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        files, cases = {}, []

        # fr_basic
        genome = mm.rand_seq(rng, 60000)
        contigs = make_contigs(rng, genome, 300, 4000)
        genome0 = genome
        r1, r2 = make_pairs(rng, genome, 9000, 400, 40)
        d = pipeline(bindir, work, "fr_basic", contigs, r1, r2)
        add_input(files, d, "fr_basic")
        for suffix, argv in FR_OPTS:
            got, err = record(cases, files, bindir, d, "fr_basic", suffix, argv)
            if suffix == "dist":
                est = estimates(got)
                assert len(est) >= 20, len(est)
                assert any(e[2] == -(K - 1) for e in est) and any(-(K - 1) < e[2] < 300 for e in est), est
                lens = dict((n, len(s)) for n, s in contigs)
                seen = set(l.split()[0] for l in got.decode().splitlines())
                sam_targets = set(l.split("\t")[2] for l in files["fr_basic.lib.sam"].decode().splitlines() if not l.startswith("@"))
                assert any(lens[t] < 1000 for t in sam_targets - seen), "no contig skipped for -s"
            if suffix == "rf_forced":
                assert "which differs from the detected orientation" in err

        # rf_matepair
        r1, r2 = make_pairs(rng, genome, 6000, 2000, 200, outward=True)
        d = pipeline(bindir, work, "rf_matepair", contigs, r1, r2)
        add_input(files, d, "rf_matepair")
        got, err = record(cases, files, bindir, d, "rf_matepair", "v", BASE + ["-v", "lib.hist"])
        assert "reverse-forward (RF)" in err and len(estimates(got)) >= 10, err
        record(cases, files, bindir, d, "rf_matepair", "dot", BASE + ["--dot", "-o", "OUT", "lib.hist"])
        record(cases, files, bindir, d, "rf_matepair", "gfa2", BASE + ["--gfa2", "lib.hist"])
        record(cases, files, bindir, d, "rf_matepair", "vv_dot", BASE + ["-v", "-v", "--dot", "lib.hist"])
        got, err = record(cases, files, bindir, d, "rf_matepair", "fr_forced", BASE + ["--fr", "-v", "lib.hist"], must_pass=False)
        assert "which differs from the detected orientation" in err

        # dups
        r1, r2 = make_pairs(rng, genome, 6000, 400, 40, dup=2500)
        d = pipeline(bindir, work, "dups", contigs, r1, r2)
        add_input(files, d, "dups")
        got, err = record(cases, files, bindir, d, "dups", "v", BASE + ["-v", "lib.hist"])
        m = re.search(r"Duplicate rate of spanning fragments: (\d+)/(\d+)", err)
        assert m and int(m.group(1)) * 10 >= int(m.group(2)) > 0, err
        record(cases, files, bindir, d, "dups", "median", BASE + ["--median", "lib.hist"])

        # wide: a PMF of more than 20,480 entries
        genome = mm.rand_seq(rng, 80150)
        wide = [("0", genome[:40000]), ("1", mm.revcomp(genome[40150:]))]
        r1, r2 = make_pairs(rng, genome, 14000, 22000, 300)
        d = pipeline(bindir, work, "wide", wide, r1, r2)
        add_input(files, d, "wide")
        hist_max = max(int(l.split()[0]) for l in files["wide.lib.hist"].decode().splitlines())
        got, err = record(cases, files, bindir, d, "wide", "v", ["-j1", "-k64", "-l40", "-s1000", "-n10", "-v", "lib.hist"])
        m = re.search(r"min: \d+ max: (\d+)", err)
        assert m and int(m.group(1)) >= 20480 and 2 <= len(estimates(got)) <= 4, (hist_max, err, got)

        # short_frag: mapped with -l20, estimated with -l40
        far_contigs = make_contigs(rng, genome0, 1000, 3000, far=(300, 345))
        r1, r2 = make_pairs(rng, genome0, 30000, 400, 40, dup=8000)
        d = pipeline(bindir, work, "short_frag", far_contigs, r1, r2, l=20)
        add_input(files, d, "short_frag")
        mixed = 0
        for suffix, argv in (("v", BASE + ["-v", "lib.hist"]), ("vv_dot", BASE + ["-v", "-v", "--dot", "lib.hist"]), ("dist", BASE + ["-o", "OUT", "lib.hist"]),
                             ("vv_n5", ["-j1", "-k64", "-l40", "-s1000", "-n5", "-v", "-v", "lib.hist"]),
                             ("vv_n12", ["-j1", "-k64", "-l40", "-s1000", "-n12", "-v", "-v", "lib.hist"]),
                             ("vv_n20", ["-j1", "-k64", "-l40", "-s1000", "-n20", "-v", "-v", "--gfa", "lib.hist"])):
            got, err = record(cases, files, bindir, d, "short_frag", suffix, argv)
            kinds = "".join("f" if "shorter than 2*l" in ln else "p" if "pairs fit the expected" in ln else "" for ln in err.splitlines())
            if suffix in ("v", "vv_dot"):
                assert kinds.count("f") >= 3 and "MLE will be more accurate if l is decreased to" in err, err
            mixed += "p" in kinds and "f" in kinds and kinds.index("p") < kinds.rindex("f")
        assert mixed, "in no run does a fragment warning follow a pairs-fit warning: the order of the two is not exercised"

        # errors
        d = os.path.join(work, "fr_basic")
        open(os.path.join(d, "empty.hist"), "w").close()
        files["errors.empty.hist"] = b""
        st, so, se, _ = run_de(bindir, d, BASE + ["empty.hist"])
        cases.append({"name": "error.empty_hist", "input": "fr_basic", "sam": "fr_basic.lib.sam", "hist": "errors.empty.hist", "argv": BASE + ["empty.hist"],
                      "status": st, "stdout": None, "stdout_text": so.decode(), "stderr": se.decode(), "out_file": None, "out": None})
        assert st == 1 and "is empty" in se.decode()
        lines = files["fr_basic.lib.sam"].decode().splitlines(True)
        head = [l for l in lines if l.startswith("@")]
        body = [l for l in lines if not l.startswith("@")]
        half = len(body) // 2
        files["errors.unsorted.sam"] = "".join(head + body[half:] + body[:half]).encode()
        open(os.path.join(d, "unsorted.sam"), "wb").write(files["errors.unsorted.sam"])
        st, so, se, _ = run_de(bindir, d, BASE + ["lib.hist"], sam="unsorted.sam")
        cases.append({"name": "error.unsorted", "input": "fr_basic", "sam": "errors.unsorted.sam", "hist": "fr_basic.lib.hist", "argv": BASE + ["lib.hist"],
                      "status": st, "stdout": None, "stdout_text": so.decode(), "stderr": se.decode(), "out_file": None, "out": None})
        assert st == 1 and "input must be sorted" in se.decode(), se
        files["errors.single.sam"] = b"@SQ\tSN:0\tLN:5000\n"
        open(os.path.join(d, "single.sam"), "wb").write(files["errors.single.sam"])
        st, so, se, _ = run_de(bindir, d, BASE + ["--dot", "lib.hist"], sam="single.sam")
        cases.append({"name": "error.single_sq", "input": "fr_basic", "sam": "errors.single.sam", "hist": "fr_basic.lib.hist", "argv": BASE + ["--dot", "lib.hist"],
                      "status": st, "stdout": None, "stdout_text": so.decode(), "stderr": se.decode(), "out_file": None, "out": None})
        assert st == 0, se
        for argv in ([], ["lib.hist"], ["-k64", "-s1000", "-n10"], ["-k64", "-s1000", "-n1x", "lib.hist"], BASE + ["--nonesuch", "lib.hist"],
                     BASE + ["a", "b", "c"], ["-k64", "-s100", "-n10", "empty.hist"]):
            st, so, se, _ = run_de(bindir, d, argv, sam="single.sam")
            cases.append({"name": "error.argv " + " ".join(argv), "input": "fr_basic", "sam": "errors.single.sam", "hist": "errors.empty.hist", "argv": argv,
                          "status": st, "stdout": None, "stdout_text": so.decode(), "stderr": se.decode(), "out_file": None, "out": None})

    sizes = dict((n, len(b)) for n, b in files.items())
    mm.OUT = OUT
    mm.write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in cases) + "\n]\n")
    make_rules()
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), os.path.getsize(os.path.join(OUT, "cases.json")), sorted(sizes.items(), key=lambda x: -x[1])[:5])


if __name__ == "__main__":
    main()
