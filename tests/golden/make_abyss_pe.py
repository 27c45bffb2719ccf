"""Regenerates tests/golden/abyss_pe_rules.json: the command lines the UNMODIFIED reference pipeline driver
(bin/abyss-pe, a Makefile) issues for the rules tests/test_abyss_pe_plumbing.py replays -- `%-1.fa`
(bin/abyss-pe:553-555), `%-1.dot` / `%-1.gfa2` (:575-577) and `%-1-rr.fa` in Bloom mode (:581-585).

Each rule is run by make with a recorder first on PATH in place of the binary it calls: the recorder
writes its argv and fails, so nothing else runs.  Kept per rule: make's arguments, the recipe line make
echoed, and the argv the binary received.

Run where the reference tree is (needs /root/reference): python tests/golden/make_abyss_pe.py
"""
import json
import os
import stat
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_PE = "/root/reference/bin/abyss-pe"
OUT = os.path.join(HERE, "abyss_pe_rules.json")

# (rule, binary, files the rule needs, make arguments)
RULES = [
    ("unitigs", "abyss-bloom-dbg", "fastq", ["name=asm", "k=32", "B=100M", "j=1", "in=r1.fq r2.fq", "asm-1.fa"]),
    # the one-letter trap of `name=`: $(t) is the input files, which abyss-pe turns into `-t<files>`
    ("unitigs_name_t", "abyss-bloom-dbg", "fastq", ["name=t", "k=32", "B=100M", "j=1", "in=r1.fq r2.fq", "t-1.fa"]),
    ("adjlist_k32", "AdjList", "k32", ["name=asm", "k=32", "B=100M", "j=1", "in=r1.fq r2.fq", "asm-1.dot"]),
    ("adjlist_k64_ss", "AdjList", "k64", ["name=asm", "k=64", "B=100M", "j=1", "in=r1.fq r2.fq", "SS=--SS", "asm-1.dot"]),
    ("adjlist_k96_gfa2", "AdjList", "k96", ["name=asm", "k=96", "B=100M", "j=1", "in=r1.fq r2.fq", "v=-v", "graph=gfa2", "asm-1.gfa2"]),
    ("rresolver", "abyss-rresolver-short", "rr_k32", ["name=asm", "k=32", "B=8M", "j=2", "in=%(reads)s", "asm-1-rr.fa"]),
]


def run_rule(binary, inputs, make_args):
    with tempfile.TemporaryDirectory() as td:
        reads = ["r1.fq", "r2.fq"]
        if inputs == "fastq":
            for f in reads:
                open(os.path.join(td, f), "w").write("@x\n%s\n+\n%s\n" % ("A" * 50, "I" * 50))
        elif inputs.startswith("k"):
            open(os.path.join(td, "asm-1.fa"), "wb").write(open(os.path.join(HERE, inputs + ".fa"), "rb").read())
        else:
            import rr_util
            reads = rr_util.write_inputs(td, inputs)
            os.rename(os.path.join(td, inputs + "-1.fa"), os.path.join(td, "asm-1.fa"))
            os.rename(os.path.join(td, inputs + "-1.dot"), os.path.join(td, "asm-1.dot"))
        shim = os.path.join(td, "shim")
        os.mkdir(shim)
        rec = os.path.join(td, "argv.txt")
        sh = os.path.join(shim, binary)
        open(sh, "w").write("#!/bin/sh\nprintf '%%s\\n' \"$@\" > %s\nexit 1\n" % rec)
        os.chmod(sh, os.stat(sh).st_mode | stat.S_IXUSR)
        args = [a % {"reads": " ".join(reads)} for a in make_args]
        r = subprocess.run(["make", "-rRf", REF_PE] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, PATH="%s:%s" % (shim, os.environ["PATH"])))
        recipe = [l for l in r.stdout.decode().splitlines() if binary in l]
        assert os.path.exists(rec) and len(recipe) == 1, (r.stdout + r.stderr).decode()
        return {"make_args": args, "recipe": recipe[0], "argv": open(rec).read().split("\n")[:-1]}


def main():
    out = {"_source": "bin/abyss-pe of the reference, run by make with a recorder in place of each binary (tests/golden/make_abyss_pe.py)"}
    for name, binary, inputs, make_args in RULES:
        out[name] = dict(run_rule(binary, inputs, make_args), binary=binary)
    json.dump(out, open(OUT, "w"), indent=1)
    open(OUT, "a").write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
