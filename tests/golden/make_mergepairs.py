#!/usr/bin/env python3
"""Regenerates tests/golden/mergepairs/*: what the UNMODIFIED reference abyss-mergepairs writes.

It compiles Align/mergepairs.cc with Align/smith_waterman.cpp, Common/{Sequence,Options,Uncompress,Fcontrol,SignalHandler,Log}.cpp
and DataLayer/FastaReader.cpp against oracle/shim, with the flags of oracle/Makefile's PIPEFLAGS and -I<reference>/Align, into a
temporary directory.  Nothing under oracle/ is changed.

cases.json + data.tar.gz hold, for each case, the inputs, argv, stdout and stderr (both in the archive) and the status, and of each
of the three PREFIX_*.fastq files its size and SHA-256 (the files themselves would take the set past the size a committed file may have; stdout
holds every merged pair's overlap).  A run the reference ends with an assert or an uncaught exception (a byte reverseComplement
refuses, files of unequal record count, -1 or -2 beyond a read's length) keeps its stderr up to that line and is marked "aborts": the
buffers the reference loses there make its files an accident of its buffering.

    python tests/golden/make_mergepairs.py            the goldens
    python tests/golden/make_mergepairs.py --time     the CPU figure: the reference on 5,000 pairs of 2 x 150 of tools/mp_bench.py
"""
import hashlib
import json
import os
import random
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

REF = mm.REF
OUT = os.path.join(HERE, "mergepairs")
SOURCES = ["Align/mergepairs.cc", "Align/smith_waterman.cpp", "Common/Sequence.cpp", "Common/Options.cpp", "Common/Uncompress.cpp", "Common/Fcontrol.cpp",
           "Common/SignalHandler.cpp", "Common/Log.cpp", "DataLayer/FastaReader.cpp"]


def compile_reference(tmp):
    flags = ["-std=c++11", "-O2", "-fopenmp", "-w", "-DFMBITS=64", "-include", "getopt.h", "-include", "unistd.h", "-I" + mm.SHIM, "-I" + REF, "-I" + REF + "/Common",
             "-I" + REF + "/DataLayer", "-I" + REF + "/FMIndex", "-I" + REF + "/vendor", "-I" + REF + "/Align"]

    def one(src):
        obj = os.path.join(tmp, src.replace("/", "_") + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(REF, src), "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, SOURCES))
    bindir = os.path.join(tmp, "bin")
    os.makedirs(bindir, exist_ok=True)
    subprocess.run(["g++", "-fopenmp", "-o", os.path.join(bindir, "abyss-mergepairs")] + objs + ["-ldl"], check=True)
    return bindir


# ---- inputs built here -------------------------------------------------------------------------------------------------------------

COMP = str.maketrans("ACGTNMRWSYKVHDBacgtnmrwsykvhdb", "TGCANKYWSRMBDHVtgcankywsrmbdhv")


def rc(s):
    return s[::-1].translate(COMP)


def dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def errors(rng, s, rate):
    out = list(s)
    for i, c in enumerate(out):
        if rng.random() < rate:
            out[i] = rng.choice([x for x in "ACGT" if x != c.upper()])
    return "".join(out)


def quals(rng, n, lo=2, hi=40, offset=33):
    """runs of one value, as a sequencer's qualities come (and so that the set stays small once compressed)"""
    out = []
    while len(out) < n:
        out += [chr(offset + rng.choice((lo, 11, 20, 25, 30, 34, 37, hi)))] * rng.randint(1, 12)
    return "".join(out[:n])


def fastq(records):
    """records: (id with comment, sequence, quality)"""
    return "".join("@%s\n%s\n+\n%s\n" % r for r in records).encode()


def fragment_pair(rng, la, lb, frag, rate):
    """reads of la and lb bases from the two ends of a fragment of `frag` bases; a fragment shorter than a read runs into adapter"""
    f = dna(rng, frag)
    one = (f + dna(rng, la))[:la]
    two = rc((dna(rng, lb) + f)[-lb:])
    return errors(rng, one, rate), errors(rng, two, rate)


def pairs_to_files(rng, pairs, tag="r"):
    r1 = [("%s%d/1" % (tag, i), a, quals(rng, len(a))) for i, (a, b) in enumerate(pairs)]
    r2 = [("%s%d/2" % (tag, i), b, quals(rng, len(b))) for i, (a, b) in enumerate(pairs)]
    return fastq(r1), fastq(r2)


def exact_identity(rng, matches, length):
    """a pair whose only gapless overlap of `length` bases holds exactly `matches` matches"""
    core = dna(rng, length)
    other = list(core)
    for p in rng.sample(range(length), length - matches):
        other[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[other[p]]
    a = dna(rng, 60, "AC") + core
    b = "".join(other) + dna(rng, 60, "GT")
    return a, rc(b)


def insert_or_delete(rng, s, n):
    s = list(s)
    for _ in range(n):
        p = rng.randrange(1, max(2, len(s) - 1))
        if rng.random() < 0.5 and len(s) > 2:
            del s[p]
        else:
            s.insert(p, rng.choice("ACGT"))
    return "".join(s)


def run(bindir, d, argv):
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"], OMP_NUM_THREADS="1")
    r = subprocess.run(["abyss-mergepairs"] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return r.returncode, r.stdout, r.stderr


class Recorder:
    def __init__(self, bindir, d):
        self.bindir, self.d, self.files, self.cases = bindir, d, {}, []

    def put(self, name, data):
        data = data if isinstance(data, bytes) else data.encode()
        self.files[name] = data
        open(os.path.join(self.d, name), "wb").write(data)

    def put_pairs(self, stem, rng, pairs):
        a, b = pairs_to_files(rng, pairs, stem)
        self.put(stem + "_1.fq", a)
        self.put(stem + "_2.fq", b)
        return [stem + "_1.fq", stem + "_2.fq"]

    def record(self, name, argv, inputs, prefix="out", dirs=()):
        for suffix in ("_merged.fastq", "_reads_1.fastq", "_reads_2.fastq"):
            if os.path.exists(os.path.join(self.d, prefix + suffix)):
                os.remove(os.path.join(self.d, prefix + suffix))
        for sub in dirs:
            os.makedirs(os.path.join(self.d, sub), exist_ok=True)
        st, so, se = run(self.bindir, self.d, argv)
        rec = {"name": name, "inputs": inputs, "argv": argv, "status": st, "prefix": prefix, "dirs": list(dirs), "stdout": None, "outputs": {}}
        if st < 0:  # an assert or an uncaught exception: the drop-in exits 1 after the same lines and a message of its own
            lines = se.decode().splitlines(True)
            cut = next((i for i, l in enumerate(lines) if "Assertion" in l or "terminate called" in l), len(lines))
            se = "".join(lines[:cut]).encode()
            rec["aborts"] = True
        rec["stderr"] = None
        if se:
            self.files[name + ".stderr"] = se
            rec["stderr"] = name + ".stderr"
        if st == 0:
            if so:
                self.files[name + ".stdout"] = so
                rec["stdout"] = name + ".stdout"
            for suffix in ("_merged.fastq", "_reads_1.fastq", "_reads_2.fastq"):
                p = os.path.join(self.d, prefix + suffix)
                if os.path.exists(p):
                    data = open(p, "rb").read()
                    rec["outputs"][suffix] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        self.cases.append(rec)
        return rec, so.decode(), se.decode()


def time_reference(bindir, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mp_bench
    f1, f2 = mp_bench.write_inputs(tmp, 5000)
    t0 = time.time()
    r = subprocess.run([os.path.join(bindir, "abyss-mergepairs"), "-o", "ref", f1, f2], cwd=tmp, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.time() - t0
    print(json.dumps({"pairs": 5000, "seconds": round(dt, 2), "ms_a_pair": round(dt / 5, 3), "cpus": os.cpu_count(), "stdout_sha256": mp_bench.digest(r.stdout),
                      "stats": r.stderr.decode().strip().splitlines()[-2:]}))


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
        rng = random.Random(20261020)

        # ---- 1. equal reads of 100 and 150, fragments from shorter than a read to twice a read, 1 to 3 % errors
        for L in (100, 150):
            pairs = [fragment_pair(rng, L, L, rng.randint(L // 3, 2 * L), rng.choice((0.01, 0.02, 0.03))) for _ in range(120)]
            ins = R.put_pairs("eq%d" % L, rng, pairs)
            R.record("eq%d.default" % L, ins, ins)
            R.record("eq%d.v" % L, ["-v"] + ins, ins)
            R.record("eq%d.m3_p0.75" % L, ["-m3", "-p0.75"] + ins, ins)

        # ---- 2. unequal lengths from 1 to 150, with and without indels; tiny first reads
        for tag, swap in (("lt", False), ("gt", True)):
            pairs = []
            for n in range(150):
                la, lb = sorted((rng.randint(1, 150), rng.randint(1, 150)))
                if n % 5 == 0:
                    la = rng.randint(1, 4)
                if swap:
                    la, lb = lb, la
                a, b = fragment_pair(rng, la, lb, rng.randint(1, la + lb), 0.02)
                if n % 3 == 0:
                    b = insert_or_delete(rng, b, rng.randint(1, 3))
                pairs.append((a, b))
            ins = R.put_pairs(tag, rng, pairs)
            for m in ("0", "1", "3", "10"):
                for p in ("0", "0.3", "0.9"):
                    R.record("%s.m%s_p%s" % (tag, m, p), ["-m" + m, "-p" + p] + ins, ins)

        # ---- 3. the stripe seams: every pair of these lengths
        seams = (1, 2, 63, 64, 65, 127, 128, 129, 193)
        pairs = []
        for la in seams:
            for lb in seams:
                a, b = fragment_pair(rng, la, lb, rng.randint(max(la, lb), la + lb), 0.02)
                pairs.append((a, b))
        ins = R.put_pairs("seam", rng, pairs)
        R.record("seam.default", ins, ins)
        R.record("seam.m1_p0.5", ["--matches=1", "--identity=0.5"] + ins, ins)
        R.record("seam.m0_p0", ["-m", "0", "-p", "0"] + ins, ins)

        # ---- 4. pairs that do not overlap: the order of ties in the last row decides
        pairs = [(dna(rng, rng.choice((40, 75, 100))), dna(rng, rng.choice((40, 75, 100)))) for _ in range(400)]
        ins = R.put_pairs("apart", rng, pairs)
        R.record("apart.default", ins, ins)
        R.record("apart.m3_p0.3", ["-m3", "-p0.3"] + ins, ins)
        R.record("apart.m1_p0", ["-m1", "-p0"] + ins, ins)

        # ---- 5. lower case, N and IUPAC codes
        pairs = []
        for n in range(120):
            a, b = fragment_pair(rng, 80, 80, rng.randint(60, 150), 0.01)
            a, b = list(a), list(b)
            kind = n % 6
            if kind == 0:  # masked ends
                for i in range(rng.randint(1, 12)):
                    a[i] = a[i].lower()
                for i in range(rng.randint(1, 12)):
                    b[-1 - i] = b[-1 - i].lower()
            elif kind == 1:  # a masked run inside
                at = rng.randint(20, 60)
                for i in range(at, at + 10):
                    a[i] = a[i].lower()
                    b[i] = b[i].lower()
            elif kind == 2:
                for i in rng.sample(range(80), 6):
                    a[i] = rng.choice("Nn")
                for i in rng.sample(range(80), 6):
                    b[i] = rng.choice("Nn")
            elif kind == 3:
                for i in rng.sample(range(80), 12):
                    a[i] = rng.choice("MRWSYKVHDBmrwsykvhdb")
                for i in rng.sample(range(80), 12):
                    b[i] = rng.choice("MRWSYKVHDBmrwsykvhdb")
            elif kind == 4:  # all of one read masked: empty once trimmed
                if n % 12 == 4:
                    a = [c.lower() for c in a]
                else:
                    b = [c.lower() for c in b]
            pairs.append(("".join(a), "".join(b)))
        # the asymmetric pairs: ('R', 'a') matches and ('r', 'A') does not
        for x, y in (("R", "a"), ("r", "A"), ("a", "R"), ("A", "r"), ("N", "a"), ("n", "A"), ("Y", "c"), ("y", "C"), ("M", "m"), ("B", "t")):
            core = dna(rng, 30)
            a = "G" + dna(rng, 20) + core[:15] + x + core[15:] + "G"
            b = "C" + core[:15] + y + core[15:] + dna(rng, 20) + "C"
            pairs.append((a, rc(b)))
        ins = R.put_pairs("codes", rng, pairs)
        R.record("codes.default", ins, ins)
        R.record("codes.no_trim", ["--no-trim-masked"] + ins, ins)
        R.record("codes.trim_m3", ["--no-trim-masked", "--trim-masked", "-m3", "-p0.5"] + ins, ins)
        R.record("codes.no_trim_m1_p1", ["--no-trim-masked", "-m1", "-p1"] + ins, ins)

        # ---- 6. identity exactly at the threshold
        pairs = []
        for m, n in ((9, 10), (18, 20), (1, 2), (3, 4), (27, 30), (45, 50), (10, 20), (15, 20), (17, 20), (19, 20)):
            for _ in range(3):
                pairs.append(exact_identity(rng, m, n))
        ins = R.put_pairs("exact", rng, pairs)
        for p in ("0", "0.3", "0.5", "0.75", "0.9", "1"):
            for m in ("1", "10"):
                R.record("exact.m%s_p%s" % (m, p), ["-m" + m, "-p" + p] + ins, ins)

        # ---- 7. -1, -2, -q, the quality offset, the chastity filter
        pairs = [fragment_pair(rng, 120, 110, rng.randint(80, 200), 0.02) for _ in range(60)]
        r1 = [("c%d" % i, a, quals(rng, len(a), 2, 40)) for i, (a, b) in enumerate(pairs)]
        r2 = [("c%d" % i, b, quals(rng, len(b), 2, 40)) for i, (a, b) in enumerate(pairs)]
        f1 = [("%s 1:%s:0:ACGT" % (n, "Y" if i in (7, 30) else "N"), s, q) for i, (n, s, q) in enumerate(r1)]
        f2 = [("%s 2:%s:0:ACGT" % (n, "Y" if i in (12, 30, 41) else "N"), s, q) for i, (n, s, q) in enumerate(r2)]
        R.put("casava_1.fq", fastq(f1))
        R.put("casava_2.fq", fastq(f2 + [("extra 2:N:0:ACGT", dna(rng, 110), quals(rng, 110))]))
        R.put("casava_2_short.fq", fastq(f2))
        ins = ["casava_1.fq", "casava_2.fq"]
        R.record("casava.default", ins, ins)
        R.record("casava.chastity_v", ["--no-chastity", "--chastity", "-v"] + ins, ins)
        R.record("casava.unequal_after_filter", ["casava_1.fq", "casava_2_short.fq"], ["casava_1.fq", "casava_2_short.fq"])
        R.record("casava.no_chastity_unequal", ["--no-chastity"] + ins, ins)
        R.record("casava.no_chastity", ["--no-chastity", "casava_1.fq", "casava_2_short.fq"], ["casava_1.fq", "casava_2_short.fq"])
        R.record("casava.len1", ["-1", "100", "casava_1.fq", "casava_2.fq"], ins)
        R.record("casava.len2", ["-2", "90", "-1100"] + ins, ins)
        R.record("casava.len1_beyond_the_read", ["-1", "121"] + ins, ins)
        R.record("casava.len2_beyond_the_read", ["-2", "111", "-v"] + ins, ins)
        R.record("casava.long_length1", ["--length1", "90"] + ins, ins)
        R.record("casava.long_length1_eq", ["--length1=90"] + ins, ins)
        R.record("casava.long_length2", ["--length2"] + ins, ins)
        R.record("casava.q10", ["-q10"] + ins, ins)
        R.record("casava.q30_len", ["--trim-quality=30", "-1", "80", "-2", "80", "-m5"] + ins, ins)
        R.record("casava.q41", ["-q41"] + ins, ins)
        ill1 = [(n, s, "".join(chr(ord(c) + 31) for c in q)) for n, s, q in f1]
        ill2 = [(n, s, "".join(chr(ord(c) + 31) for c in q)) for n, s, q in f2 + [("extra 2:N:0:ACGT", dna(rng, 110), quals(rng, 110))]]
        R.put("ill_1.fq", fastq(ill1))
        R.put("ill_2.fq", fastq(ill2))
        ins = ["ill_1.fq", "ill_2.fq"]
        R.record("illumina.q10", ["--illumina-quality", "-q10"] + ins, ins)
        R.record("illumina.standard_q10", ["--illumina-quality", "--standard-quality", "-q10"] + ins, ins)

        # ---- 8. -v, -vvv, -o
        ins = ["eq100_1.fq", "eq100_2.fq"]
        R.record("out.vvv", ["-vvv", "seam_1.fq", "seam_2.fq"], ["seam_1.fq", "seam_2.fq"])
        R.record("out.vvv_m3", ["-v", "--verbose", "-v", "-m3", "-p0.5", "exact_1.fq", "exact_2.fq"], ["exact_1.fq", "exact_2.fq"])
        R.put("apart60_1.fq", b"\n".join(R.files["apart_1.fq"].split(b"\n")[:4 * 60]) + b"\n")
        R.put("apart60_2.fq", b"\n".join(R.files["apart_2.fq"].split(b"\n")[:4 * 60]) + b"\n")
        R.record("out.vvv_apart", ["-vvv", "-m1", "-p0", "apart60_1.fq", "apart60_2.fq"], ["apart60_1.fq", "apart60_2.fq"])
        R.record("out.vvv_codes", ["-vvv", "--no-trim-masked", "-m3", "-p0.5", "codes_1.fq", "codes_2.fq"], ["codes_1.fq", "codes_2.fq"])
        R.record("out.prefix", ["-o", "mine"] + ins, ins, prefix="mine")
        R.record("out.prefix_dir", ["--prefix=sub/dir/x", "-v"] + ins, ins, prefix="sub/dir/x", dirs=["sub/dir"])
        R.record("out.prefix_no_dir", ["-o", "nonesuch/x"] + ins, ins, prefix="nonesuch/x")

        # ---- 9. a byte reverseComplement refuses, in the fourth pair; files of unequal record count; empty files
        pairs = [fragment_pair(rng, 50, 50, 70, 0.01) for _ in range(6)]
        pairs[3] = (pairs[3][0], pairs[3][1][:20] + "X" + pairs[3][1][21:])
        ins = R.put_pairs("badchar", rng, pairs)
        R.record("bad.character", ins, ins)
        pairs[3] = (pairs[3][0][:20] + "X" + pairs[3][0][21:], pairs[4][1])
        ins = R.put_pairs("badchar1", rng, pairs)
        R.record("bad.character_in_read1", ["-m1", "-p0"] + ins, ins)
        pairs = [fragment_pair(rng, 50, 50, 70, 0.01) for _ in range(8)]
        a, b = pairs_to_files(rng, pairs, "u")
        R.put("uneq_1.fq", a)
        R.put("uneq_2.fq", b)
        R.put("uneq_1_less.fq", b"\n".join(a.split(b"\n")[:4 * 6]) + b"\n")
        R.put("uneq_2_less.fq", b"\n".join(b.split(b"\n")[:4 * 7]) + b"\n")
        R.put("empty.fq", b"")
        R.record("unequal.first_longer", ["uneq_1.fq", "uneq_2_less.fq"], ["uneq_1.fq", "uneq_2_less.fq"])
        R.record("unequal.second_longer", ["uneq_1_less.fq", "uneq_2.fq"], ["uneq_1_less.fq", "uneq_2.fq"])
        R.record("unequal.second_longer_by_two", ["-v", "uneq_1_less.fq", "uneq_2.fq"], ["uneq_1_less.fq", "uneq_2.fq"])
        R.record("empty.both", ["empty.fq", "empty.fq"], ["empty.fq"])
        R.record("empty.both_v", ["-v", "empty.fq", "empty.fq"], ["empty.fq"])
        R.record("empty.first", ["empty.fq", "uneq_2.fq"], ["empty.fq", "uneq_2.fq"])
        R.record("empty.second", ["uneq_1.fq", "empty.fq"], ["uneq_1.fq", "empty.fq"])

        # ---- 10. every option error
        for argv in ([], ["--help"], ["--version"], ["a"], ["a", "b", "c"], ["-p0.9x", "a", "b"], ["-px", "a", "b"], ["-m3x", "a", "b"], ["-m", "-1", "a", "b"],
                     ["-q1x", "a", "b"], ["-1", "5x", "a", "b"], ["-2", "x", "a", "b"], ["-ox y", "a", "b"], ["-o", "", "a", "b"], ["--nonesuch", "a", "b"],
                     ["-x", "a", "b"], ["-m"], ["-x"], ["--length1=5x", "a", "b"], ["--identity", "0.5", "--matches"], ["nonesuch_1.fq", "uneq_2.fq"],
                     ["uneq_1.fq", "nonesuch_2.fq"], ["-v", "nonesuch_1.fq", "nonesuch_2.fq"]):
            inputs = [a for a in argv if a in R.files]
            R.record("error.argv " + " ".join(argv), argv, inputs)

        # ---- sections 11 to 13 draw from a generator of their own, so that nothing above changes when they do
        rng = random.Random(20261021)

        # ---- 11. the reads the tool is for: 2 x 250 and 2 x 300, fragments from a third of a read to twice a read, 1 to 3 % errors
        for L in (250, 300):
            pairs = [fragment_pair(rng, L, L, rng.randint(L // 3, 2 * L), rng.choice((0.01, 0.02, 0.03))) for _ in range(60)]
            ins = R.put_pairs("eq%d" % L, rng, pairs)
            R.record("eq%d.default" % L, ins, ins)
            R.record("eq%d.m3_p0.75" % L, ["-m3", "-p0.75"] + ins, ins)

        # ---- 12. the seams up to the kernel's limit of 512 and past it (513 and 600 are the host's): every pair of these lengths
        seams = (1, 64, 255, 256, 257, 320, 449, 511, 512, 513, 600)
        pairs = []
        for la in seams:
            for lb in seams:
                pairs.append(fragment_pair(rng, la, lb, rng.randint(max(la, lb), la + lb), 0.02))
        ins = R.put_pairs("seam512", rng, pairs)
        R.record("seam512.default", ins, ins)
        R.record("seam512.m1_p0.5", ["--matches=1", "--identity=0.5"] + ins, ins)
        R.record("seam512.m0_p0", ["-m", "0", "-p", "0"] + ins, ins)

        # ---- 13. long pairs that do not overlap: the ties of a last row of 300 to 512 columns
        pairs = [(dna(rng, rng.randint(300, 512)), dna(rng, rng.randint(300, 512))) for _ in range(60)]
        ins = R.put_pairs("apart400", rng, pairs)
        R.record("apart400.default", ins, ins)
        R.record("apart400.m1_p0", ["-m1", "-p0"] + ins, ins)

        files, cases = R.files, R.cases
    mm.OUT = OUT
    mm.write_data(files)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in cases) + "\n]\n")
    print("wrote", OUT, os.path.getsize(os.path.join(OUT, "data.tar.gz")), len(cases), "cases")
    for c in cases:
        tail = (files[c["stderr"]].decode() if c["stderr"] else "").strip().splitlines()[-2:]
        print(c["status"], c["name"], "|", " / ".join(tail)[:200])


if __name__ == "__main__":
    main()
