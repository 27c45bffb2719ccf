#!/usr/bin/env python3
"""Regenerates tests/golden/konnector/*: Konnector Bloom filters (`abyss-bloom build -t konnector`, the reference's default type)
and the commands on those files (union, intersect, info, compare, kmers), written by the UNMODIFIED reference.

It compiles Bloom/bloom.cc with the nine Common/DataLayer sources of oracle/Makefile's REFSRC against oracle/shim (plus the Boost
property-map header that bloom.cc reaches through the shim) into a temporary directory, and a small known-answer driver that
links Common/Kmer.cpp and Common/city.cc and prints Bloom::hash(Kmer(window), seed) for every window.  Nothing under oracle/ is
changed.  Run in the build container (needs the reference sources):
    python tests/golden/make_konnector.py [--no-large]
The large cases (large.json: filters past 2^32 bits, records longer than a staging slot) take a few minutes.
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ABYSS_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "konnector")
SHIM = os.path.join(ROOT, "oracle", "shim")
SOURCES = ["Bloom/bloom.cc", "Common/Kmer.cpp", "Common/Sequence.cpp", "Common/Options.cpp", "Common/Uncompress.cpp",
           "Common/Fcontrol.cpp", "Common/SignalHandler.cpp", "Common/Log.cpp", "Common/city.cc", "DataLayer/FastaReader.cpp"]
FLAGS = ["-std=c++11", "-O2", "-fopenmp", "-w", "-include", "getopt.h", "-include", "unistd.h", "-include",
         "boost/property_map/property_map.hpp", "-I" + SHIM, "-I" + REF, "-I" + REF + "/Common", "-I" + REF + "/DataLayer",
         "-I" + REF + "/vendor"]

# the known-answer driver: lines "k seed seq" in, one line of hashes per input line out ("-" for a window that is not all ACGT)
DRIVER = r'''
#include "Common/Kmer.h"
#include "Common/HashFunction.h"
#include <cstdio>
#include <iostream>
#include <string>
int main()
{
	unsigned k; unsigned long long seed; std::string seq;
	while (std::cin >> k >> seed >> seq) {
		Kmer::setLength(k);
		for (size_t i = 0; i + k <= seq.size(); i++) {
			std::string w = seq.substr(i, k);
			if (w.find_first_not_of("ACGTacgt") != std::string::npos) { printf(i ? " -" : "-"); continue; }
			for (auto& c : w) c = toupper(c);
			Kmer key(w);
			unsigned long long h;
			if (key.isCanonical()) h = hashmem(&key, key.bytes(), seed);
			else { Kmer r(key); r.reverseComplement(); h = hashmem(&r, r.bytes(), seed); }
			printf(i ? " %llu" : "%llu", h);
		}
		printf("\n");
	}
	return 0;
}
'''

HASH_KS = [5, 25, 32, 33, 63, 64, 65, 96, 128, 129, 150, 192]
HASH_SEEDS = [0, 7, (1 << 63) + 5]


def compile_reference(tmp):
    objs = []

    def one(src):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["g++"] + FLAGS + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, SOURCES))
    exe = os.path.join(tmp, "abyss-bloom")
    subprocess.run(["g++", "-fopenmp", "-o", exe] + objs + ["-ldl"], check=True)
    drv_src = os.path.join(tmp, "kn_driver.cc")
    open(drv_src, "w").write(DRIVER)
    drv = os.path.join(tmp, "kn_driver")
    keep = [o for o in objs if os.path.basename(o).split(".")[0] in ("Kmer", "city", "Sequence", "Options")]
    subprocess.run(["g++"] + FLAGS + ["-o", drv, drv_src] + keep + ["-ldl"], check=True)
    return exe, drv


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def make_reads(rng):
    """FASTA: a genome sampled with errors, N runs, lower case, reads shorter than k and planted palindromes; FASTQ: 150 bp reads
    with qualities for -q."""
    genome = "".join(rng.choice("ACGT") for _ in range(60000))
    fa, fq = [], []
    for i in range(3000):
        L = rng.choice([20, 40, 64, 100, 150, 150, 150, 200, 250, 300])
        at = rng.randrange(0, len(genome) - L)
        s = list(genome[at:at + L])
        if rng.random() < 0.5:
            s = list(revcomp("".join(s)))
        for j in range(L):
            r = rng.random()
            if r < 0.004:
                s[j] = rng.choice("ACGT")
            elif r < 0.006:
                s[j] = "N"
        if rng.random() < 0.1:
            a = rng.randrange(0, L)
            for j in range(a, min(L, a + rng.randrange(1, 30))):
                s[j] = s[j].lower()
        if rng.random() < 0.05:  # a palindromic stretch: its even k-mers centred on it are their own reverse complement
            h = "".join(rng.choice("ACGT") for _ in range(48))
            p = h + revcomp(h)
            a = rng.randrange(0, max(1, L - len(p)))
            s[a:a + len(p)] = list(p)
            s = s[:L] if len(s) > L else s
        fa.append(">r%d\n%s\n" % (i, "".join(s)))
    for i in range(3000):
        at = rng.randrange(0, len(genome) - 150)
        s = list(genome[at:at + 150])
        q = [chr(33 + rng.choice([2, 2, 3, 10, 20, 30, 35, 40, 40, 40])) for _ in range(150)]
        if rng.random() < 0.02:
            s[rng.randrange(0, 150)] = "N"
        fq.append("@q%d\n%s\n+\n%s\n" % (i, "".join(s), "".join(q)))
    return "".join(fa), "".join(fq)


def hash_vectors(drv, rng):
    seqs = {}
    lines = []
    for k in HASH_KS:
        base = "".join(rng.choice("ACGT") for _ in range(k + 40))
        mixed = list("".join(rng.choice("ACGT") for _ in range(k + 30)))
        mixed[k // 2] = "N"
        for j in range(k + 5, k + 15):
            mixed[j] = mixed[j].lower()
        half = "".join(rng.choice("ACGT") for _ in range(k // 2 + 4))
        pal = half + revcomp(half)  # k even: the middle windows are palindromes
        seqs[k] = [base, "".join(mixed), pal, "A" * (k + 3), "T" * (k + 2)]
        for seed in HASH_SEEDS:
            for s in seqs[k]:
                lines.append("%d %d %s" % (k, seed, s))
    out = subprocess.run([drv], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    vec, n = [], 0
    for k in HASH_KS:
        for seed in HASH_SEEDS:
            for s in seqs[k]:
                hs = [None if x == "-" else int(x) for x in out[n].split()]
                n += 1
                assert len(hs) == len(s) - k + 1
                vec.append({"k": k, "seed": str(seed), "seq": s, "hash": [None if h is None else str(h) for h in hs]})
    return vec


# name, args after `build` (outputs <name>.bloom in the working directory)
BUILDS = [
    ("k25_l1", ["-k25", "-b32K", "-l1", "reads.fa"]),
    ("k25_l2", ["-k25", "-b64K", "-l2", "reads.fa"]),
    ("k25_l3_odd", ["-k25", "-b8002", "-l3", "reads.fa"]),  # 64016 / 3 = 21338 bits a level: not a multiple of 8 or 64
    ("k25_l1_h7", ["-k25", "-b32K", "-h7", "reads.fa"]),
    ("k64_l1_hbig", ["-k64", "-b32K", "-h9223372036854775813", "reads.fa"]),
    ("k25_w1", ["-k25", "-b32K", "-w", "1/4", "reads.fa"]),
    ("k25_w2", ["-k25", "-b32K", "-w", "2/4", "reads.fa"]),
    ("k25_w3", ["-k25", "-b32K", "-w", "3/4", "reads.fa"]),
    ("k25_w4", ["-k25", "-b32K", "-w", "4/4", "reads.fa"]),
    ("k25_l2_L1", ["-k25", "-b64K", "-l2", "-L", "1=k25_l1.bloom", "reads.fa"]),
    ("k64_fq_q3", ["-k64", "-b32K", "-q3", "reads.fq"]),
    ("k96_l2", ["-k96", "-b64K", "-l2", "reads.fa"]),
    ("k150_l1", ["-k150", "-b32K", "reads.fa", "reads.fq"]),
    ("k33_l3_w2", ["-k33", "-b96K", "-l3", "-w", "2/2", "reads.fa"]),
    # every width of the insert kernel (NW = ceil(k / 32)) and its edges in a cascade; odd -b: bits a level neither a power of
    # two nor a multiple of 8
    ("k12_l2", ["-k12", "-b32K", "-l2", "reads.fa"]),
    ("k31_l3_odd", ["-k31", "-b24001", "-l3", "reads.fa"]),  # 64002 bits a level
    ("k32_l2", ["-k32", "-b32K", "-l2", "reads.fa", "reads.fq"]),
    ("k97_l2_odd", ["-k97", "-b24577", "-l2", "reads.fa"]),  # 98308 bits a level
    ("k128_l3", ["-k128", "-b48K", "-l3", "reads.fa", "reads.fq"]),
    ("k160_l2", ["-k160", "-b32K", "-l2", "reads.fa"]),
    ("k161_l3_odd", ["-k161", "-b30001", "-l3", "reads.fa"]),  # 80002 bits a level
    ("k192_l2", ["-k192", "-b64K", "-l2", "reads.fa"]),
]

# name, argv after the program (files refer to the builds above); outputs named out_<name>.bloom are kept
COMMANDS = [
    ("union_windows", ["union", "-k25", "out_union_windows.bloom", "k25_w1.bloom", "k25_w2.bloom", "k25_w3.bloom", "k25_w4.bloom"]),
    ("union_three", ["union", "-k25", "out_union_three.bloom", "k25_l1.bloom", "k25_l2.bloom", "k25_l2_L1.bloom"]),
    ("intersect_two", ["intersect", "-k25", "out_intersect_two.bloom", "k25_l1.bloom", "k25_l2.bloom"]),
    ("intersect_window", ["intersect", "-k25", "out_intersect_window.bloom", "k25_l1.bloom", "k25_w2.bloom"]),
    ("union_window_first", ["union", "-v", "-k25", "out_union_window_first.bloom", "k25_w3.bloom", "k25_l1.bloom"]),
    ("union_size_mismatch", ["union", "-k25", "out_bad1.bloom", "k25_l1.bloom", "k25_l3_odd.bloom"]),
    ("intersect_seed_mismatch", ["intersect", "-k25", "out_bad2.bloom", "k25_l1.bloom", "k25_l1_h7.bloom"]),
    ("info_l1", ["info", "-k25", "k25_l1.bloom"]),
    ("info_l2", ["info", "-k25", "k25_l2.bloom"]),
    ("info_window", ["info", "-k25", "k25_w2.bloom"]),
    ("info_odd", ["info", "-k25", "k25_l3_odd.bloom"]),
    ("info_k64", ["info", "-k64", "k64_l1_hbig.bloom"]),
    ("compare_jaccard", ["compare", "-k25", "k25_l1.bloom", "k25_l2.bloom"]),
    ("compare_forbes", ["compare", "-k25", "-m", "forbes", "k25_l1.bloom", "k25_l1_h7.bloom"]),
    ("compare_czekanowski", ["compare", "-k25", "-m", "czekanowski", "k25_l1.bloom", "k25_l2_L1.bloom"]),
    ("compare_size_mismatch", ["compare", "-k25", "k25_l1.bloom", "k25_w1.bloom"]),
]

# name, argv: the kmers outputs are kept as sha256 and line count
KMERS = [
    ("kmers_fasta", ["kmers", "-k25", "k25_l2.bloom", "reads.fa"]),
    ("kmers_fasta_r", ["kmers", "-k25", "-r", "k25_l2.bloom", "reads.fa"]),
    ("kmers_bed", ["kmers", "-k25", "--bed", "k25_l2.bloom", "reads.fa"]),
    ("kmers_bed_r", ["kmers", "-k25", "-r", "--bed", "k25_l2.bloom", "reads.fa"]),
    ("kmers_raw", ["getKmers", "-k25", "--raw", "k25_l2.bloom", "reads.fa"]),
    ("kmers_raw_r", ["kmers", "-k25", "--raw", "-r", "k25_l2.bloom", "reads.fa"]),
    ("kmers_k64_window", ["kmers", "-k64", "--bed", "k64_l1_hbig.bloom", "reads.fq"]),
    ("kmers_k150", ["kmers", "-k150", "k150_l1.bloom", "reads.fa"]),
    ("kmers_k128_bed", ["kmers", "-k128", "--bed", "k128_l3.bloom", "reads.fa"]),
    ("kmers_k128_raw_r", ["kmers", "-k128", "--raw", "-r", "k128_l3.bloom", "reads.fa"]),
    ("kmers_k192_bed_r", ["kmers", "-k192", "--bed", "-r", "k192_l2.bloom", "reads.fa"]),
    ("kmers_k192_raw", ["kmers", "-k192", "--raw", "k192_l2.bloom", "reads.fa"]),
]

# large.json: name, the cases that must run first (their outputs are inputs), argv; outputs are kept as sha256 and byte count.
# reads.fa and reads.fq are the archive's; long.fa comes from tests/kn_large.py
LARGE = [
    ("build_b2G_l3", [], ["build", "-k64", "-b2G", "-l3", "l3.bloom", "reads.fa"]),  # 5,726,623,061 bits a level: odd, > 2^32
    ("build_b2G_l2", [], ["build", "-k64", "-b2G", "-l2", "l2.bloom", "reads.fa"]),  # 2^33 bits a level
    ("build_b1G_w4", [], ["build", "-k64", "-b1G", "-w", "4/4", "w4.bloom", "reads.fq"]),  # the window starts at bit 6,442,450,944
    ("kmers_b2G_l3_bed", ["build_b2G_l3"], ["kmers", "-k64", "--bed", "l3.bloom", "reads.fa"]),
    ("info_b2G_l3", ["build_b2G_l3"], ["info", "-k64", "l3.bloom"]),
    ("build_long_b64M_l2", [], ["build", "-k64", "-b64M", "-l2", "long.bloom", "long.fa"]),
    ("build_reads_b64M", [], ["build", "-k64", "-b64M", "reads64M.bloom", "reads.fa"]),
    ("kmers_long_bed", ["build_reads_b64M"], ["kmers", "-k64", "--bed", "reads64M.bloom", "long.fa"]),
]


def run(exe, argv, cwd):
    r = subprocess.run([exe] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, OMP_NUM_THREADS="1"))
    return r.returncode, r.stdout, r.stderr


def write_data(files):
    """The reads, the hash vectors and every filter file as one deterministic tar.gz (sorted names, zero times)."""
    import gzip
    import io
    import tarfile
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.USTAR_FORMAT) as tar:
        for name in sorted(files):
            info = tarfile.TarInfo(name)
            info.size, info.mtime, info.mode = len(files[name]), 0, 0o644
            tar.addfile(info, io.BytesIO(files[name]))
    with open(os.path.join(OUT, "data.tar.gz"), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
            z.write(raw.getvalue())


def write_cases(cases):
    """One record a line: reviewable as text."""
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("{\n")
        for i, kind in enumerate(("build", "commands", "kmers")):
            f.write(' "%s": [\n' % kind)
            f.write(",\n".join("  " + json.dumps(r) for r in cases[kind]))
            f.write("\n ]%s\n" % ("," if i < 2 else ""))
        f.write("}\n")


def digest(data):
    """stdout or stderr as text when short, else as sha256, byte count and line count"""
    if len(data) <= 4096:
        return {"text": data.decode()}
    return {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data), "lines": data.count(b"\n")}


def large_cases(exe, files, tmp):
    """large.json: every LARGE case run by the reference, its outputs kept as digests (and deleted once digested)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import kn_large
    work = os.path.join(tmp, "large")
    os.makedirs(work)
    inputs = {}
    for name in ("reads.fa", "reads.fq"):
        open(os.path.join(work, name), "wb").write(files[name])
        inputs[name] = {"sha256": hashlib.sha256(files[name]).hexdigest(), "bytes": len(files[name])}
    sha, size = kn_large.write_long_fasta(os.path.join(work, "long.fa"), files["reads.fa"])
    inputs["long.fa"] = {"sha256": sha, "bytes": size}
    out = []
    for name, needs, argv in LARGE:
        before = set(os.listdir(work))
        st, so, se = run(exe, argv, work)
        assert st == 0, (name, se)
        outputs = {}
        for f in sorted(set(os.listdir(work)) - before):
            sha, size = kn_large.sha256_file(os.path.join(work, f))
            outputs[f] = {"sha256": sha, "bytes": size}
        out.append({"name": name, "needs": needs, "argv": argv, "status": st, "stdout": digest(so), "stderr": digest(se),
                    "outputs": outputs})
        for c in out:  # outputs no later case needs go
            if not any(c["name"] in n for _, n, _ in LARGE[len(out):]):
                for f in c["outputs"]:
                    if os.path.exists(os.path.join(work, f)):
                        os.remove(os.path.join(work, f))
    with open(os.path.join(OUT, "large.json"), "w") as f:
        f.write('{\n "inputs": %s,\n "cases": [\n' % json.dumps(inputs))
        f.write(",\n".join("  " + json.dumps(c) for c in out))
        f.write("\n ]\n}\n")


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference sources are needed (%s)" % REF)
    rng = random.Random(20261015)
    os.makedirs(OUT, exist_ok=True)
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe, drv = compile_reference(tmp)
        fa, fq = make_reads(rng)
        files["reads.fa"], files["reads.fq"] = fa.encode(), fq.encode()
        files["hash_vectors.json"] = json.dumps(hash_vectors(drv, rng)).encode()
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        for name in ("reads.fa", "reads.fq"):
            open(os.path.join(work, name), "wb").write(files[name])
        cases = {"build": [], "commands": [], "kmers": []}
        for name, args in BUILDS:
            st, out, err = run(exe, ["build"] + args_with_output(args, name), work)
            assert st == 0, (name, err)
            files[name + ".bloom"] = open(os.path.join(work, name + ".bloom"), "rb").read()
            cases["build"].append({"name": name, "args": args, "status": st, "stdout": out.decode(), "stderr": err.decode()})
        for name, argv in COMMANDS:
            st, out, err = run(exe, argv, work)
            rec = {"name": name, "argv": argv, "status": st, "stdout": out.decode(), "stderr": err.decode(), "output": None}
            outp = os.path.join(work, "out_%s.bloom" % name)
            if st == 0 and os.path.exists(outp):
                files["out_%s.bloom" % name] = open(outp, "rb").read()
                rec["output"] = "out_%s.bloom" % name
            cases["commands"].append(rec)
        for name, argv in KMERS:
            st, out, err = run(exe, argv, work)
            assert st == 0, (name, err)
            cases["kmers"].append({"name": name, "argv": argv, "status": st, "sha256": hashlib.sha256(out).hexdigest(),
                                   "lines": out.count(b"\n")})
        if "--no-large" not in sys.argv:
            large_cases(exe, files, tmp)
    write_data(files)
    write_cases(cases)
    print("wrote", OUT)


def args_with_output(args, name):
    """`build [options] <OUTPUT> <READS>...`: the output name goes in front of the first read file."""
    i = next(j for j, a in enumerate(args) if a.startswith("reads."))
    return args[:i] + [name + ".bloom"] + args[i:]


if __name__ == "__main__":
    main()
