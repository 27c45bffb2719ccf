#!/usr/bin/env python3
"""Golden vectors for `-g` (outputGraph, BloomDBG/bloom-dbg.h:1171-1242) from the unmodified
reference binary (oracle/_ref/abyss-bloom-dbg, built by `make -C oracle ref`): for the read sets
of the existing golden cases, the SHA-256, size and node / edge counts of the GraphViz file the
reference writes, plus one small file in full (the first 300 reads of k32); the same for the
graph shapes, template widths and growth case of tests/graph_cases.py (seeded reads: with the
generator's arguments, the reference's options and its counter count), and the digest of the
coverage track (-C / -R) it writes for that module's three-record reference.  Needs the reference
binary; the fixtures travel, the reference does not."""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import graph_cases as gc  # noqa: E402
from util import GoldenCase  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "abyss-bloom-dbg")


def run(g, reads, opts, stats=None):
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "reads.fa"), "wb") as f:
            for i, r in enumerate(reads):
                f.write(b">r%d\n%s\n" % (i, r))
        r = subprocess.run([REF] + opts + ["-j1", "-v", "-g", "g.dot", "reads.fa"], cwd=td, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, check=True)
        dot = open(os.path.join(td, "g.dot"), "rb").read()
        err = r.stderr.decode()
        m = re.search(r"processed \d+ reads \(k-mers visited: (\d+), edges visited: (\d+)\)", err)
        if stats is not None:
            stats["counters"] = int(re.search(r"#counters\s+= (\d+)", err).group(1))
        return dot, int(m.group(1)), int(m.group(2))


def entry(dot, nodes, edges):
    return {"sha256": hashlib.sha256(dot).hexdigest(), "bytes": len(dot), "nodes": nodes, "edges": edges}


def seeded(buf, off, opts, gen):
    reads = [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    st = {}
    dot, nodes, edges = run(None, reads, opts, st)
    e = entry(dot, nodes, edges)
    e.update(counters=st["counters"], options=opts, generator=gen)
    return e


def coverage_track():
    g = GoldenCase(gc.COV_READS)
    recs = gc.cov_records(g.opts["k"], gc.cov_text(gc.COV_READS))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "reads.fa"), "wb").write(gc.reads_fasta(g.buf, g.off))
        open(os.path.join(td, "ref.fa"), "wb").write(gc.cov_fasta(recs))
        subprocess.run([REF] + g.meta["options"] + ["-j1", "-C", "cov.wig", "-R", "ref.fa", "reads.fa"], cwd=td,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        wig = open(os.path.join(td, "cov.wig"), "rb").read()
    return {"sha256": hashlib.sha256(wig).hexdigest(), "bytes": len(wig), "solid_runs": wig.count(b" 1\n"),
            "steps": wig.count(b"variableStep"), "options": g.meta["options"], "reads": gc.COV_READS}


def main():
    out = {}
    for name in ("k32", "k64", "k40_mixed", "k48_K16", "k25_h3_kc3_t40"):
        g = GoldenCase(name)
        dot, nodes, edges = run(g, g.reads, g.meta["options"])
        out[name] = {"sha256": hashlib.sha256(dot).hexdigest(), "bytes": len(dot), "nodes": nodes, "edges": edges}
        print(name, out[name])
    g = GoldenCase("k32")
    dot, nodes, edges = run(g, g.reads[:300], g.meta["options"])
    out["k32_first300"] = {"sha256": hashlib.sha256(dot).hexdigest(), "bytes": len(dot), "nodes": nodes, "edges": edges}
    with gzip.GzipFile(os.path.join(HERE, "k32_first300.graph.dot.gz"), "wb", mtime=0) as f:
        f.write(dot)
    for name in gc.SHAPES:
        g = GoldenCase(name)
        out[name] = entry(*run(g, g.reads, g.meta["options"]))
        print(name, out[name])
    for k, K, s in gc.WIDTHS:
        buf, off, gen = gc.seeded_reads(k, s)
        name = gc.width_name(k, K, s)
        out[name] = seeded(buf, off, ["-k%d" % k] + (["-K%d" % K] if K else []) + [gc.SEEDED_COUNTERS_OPT], gen)
        print(name, out[name])
    buf, off = gc.growth_reads()
    out["growth_k40"] = seeded(buf, off, ["-k%d" % gc.GROWTH["k"], gc.GROWTH["opt"]], dict(gc.GROWTH))
    print("growth_k40", out["growth_k40"])
    assert out["growth_k40"]["nodes"] > gc.GROWTH_MIN_NODES
    out["cov_track_k40"] = coverage_track()
    print("cov_track_k40", out["cov_track_k40"])
    json.dump(out, open(os.path.join(HERE, "graph_golden.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
