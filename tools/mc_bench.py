#!/usr/bin/env python3
"""Times MergeContigs' merge on the 92,000-contig set of tools/ov_bench.py (contigs of 200..3000 bp, every other one stored
reverse-complemented, half of the junctions an overlap of 5..62 bases) with generated chain paths: every maximal run of consecutive
contigs joined by an overlap is one path, and the graph holds those edges.  Prints one JSON line: the two kernels from events, the
splice pass's bytes read plus written per second against the HBM peak, the abg_mc_merge call, `MergeContigs` end to end, SHA-256 of
its outputs, and whether tests/hostcheck/mc_check writes the same bytes from the same files.

    python tools/mc_bench.py [--contigs N] [--keep DIR]

write_inputs(dir) is what tests/golden/make_mergecontigs.py --time runs the unmodified reference on."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
K = 64
HBM_BYTES_PER_S = 8e12  # MI355X: 8 TB/s peak


def digest(data):
    return hashlib.sha256(data).hexdigest()[:16]


def build_set(n, seed):
    """(contigs as stored, [(nodes, overlaps)], the ADJ text, the path file text)"""
    import ov_bench
    seqs, dists = ov_bench.simulate(n, seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    stored = [lut[ov_bench.revcomp(s) if i % 2 else s].tobytes() for i, s in enumerate(seqs)]
    name = lambda i, flip=False: "%d%s" % (i, "-" if (i % 2 == 1) != flip else "+")
    right, left = [[] for _ in range(n)], [[] for _ in range(n)]
    paths, run, ovs = [], [0], [0]
    for i, d in enumerate(dists):
        if -(K - 1) < d <= -5:  # an overlap: the edge node(i) -> node(i + 1) and its complement
            e = " [d=%d]" % d
            (left if i % 2 else right)[i].append((name(i + 1, True) if i % 2 else name(i + 1)) + e)
            (right if (i + 1) % 2 else left)[i + 1].append((name(i, True) if (i + 1) % 2 else name(i)) + e)
            run.append(i + 1)
            ovs.append(-d)
        else:
            if len(run) > 1:
                paths.append((run, ovs))
            run, ovs = [i + 1], [0]
    if len(run) > 1:
        paths.append((run, ovs))
    adj = "".join("%d %d %d\t;%s\t;%s\n" % (i, len(s), 30 * len(s), "".join(" " + x for x in right[i]), "".join(" " + x for x in left[i])) for i, s in enumerate(stored))
    text = "".join("%d\t%s\n" % (n + p, " ".join(name(i) for i in run)) for p, (run, _) in enumerate(paths))
    return stored, [([2 * i + (i % 2) for i in run], ovs) for run, ovs in paths], adj, text


def write_inputs(d, n=92_000, seed=7):
    """(FASTA, graph, path file, k) in d"""
    stored, paths, adj, text = build_set(n, seed)
    with open(os.path.join(d, "m.fa"), "wb") as f:
        for i, s in enumerate(stored):
            f.write(b">%d\n%s\n" % (i, s))
    open(os.path.join(d, "m.adj"), "w").write(adj)
    open(os.path.join(d, "m.path"), "w").write(text)
    return "m.fa", "m.adj", "m.path", K


def time_merge(stored, paths, repeat=3):
    from abyss_amd import api
    m = api.PathMerge()
    m.set_contigs(stored)
    m.merge(K, paths)  # warm-up: buffers and code object
    m.profile(True)
    _, bytes0 = m.profile_get("mc_bytes")
    calls = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        seqs, acgt, redone, logs = m.merge(K, paths)
        calls.append(time.perf_counter() - t0)
    junction_ms, splice_ms = m.profile_get("mc_junction")[0] / repeat, m.profile_get("mc_splice")[0] / repeat
    out_bytes = (m.profile_get("mc_bytes")[1] - bytes0) // repeat
    redone_total = m.profile_get("mc_redone")[1]
    m.close()
    moved = 2 * out_bytes  # every output byte is read once and written once (segments and consensus are a few percent more)
    return {"paths": len(paths), "nodes": sum(len(p[0]) for p in paths), "output_bytes": int(out_bytes), "junction_ms": round(junction_ms, 3),
            "splice_ms": round(splice_ms, 3), "splice_bytes_per_s": round(moved / (splice_ms * 1e-3)) if splice_ms else None,
            "splice_share_of_hbm_peak": round(moved / (splice_ms * 1e-3) / HBM_BYTES_PER_S, 4) if splice_ms else None,
            "merge_call_ms": round(1e3 * min(calls), 2), "redone_on_host": int(redone_total)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=92_000)
    ap.add_argument("--keep")
    a = ap.parse_args()
    from abyss_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        stored, paths, _, _ = build_set(a.contigs, 7)
        fa, adj, path, k = write_inputs(d, a.contigs)
        out = {"contigs": a.contigs, "k": k, "merge": time_merge(stored, paths)}
        exe = os.path.join(build.BIN_DIR, "MergeContigs")
        argv = ["-k%d" % k, "-o", "o.fa", "-g", "o.dot", fa, adj, path]
        t0 = time.perf_counter()
        r = subprocess.run([exe] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        out["mergecontigs_seconds"] = round(time.perf_counter() - t0, 3)
        read = lambda f: open(os.path.join(d, f), "rb").read()
        out["fa_sha256"], out["graph_sha256"], out["stderr"] = digest(read("o.fa")), digest(read("o.dot")), r.stderr.decode().splitlines()
        # the same run by the host check (the serial text of abg_mc.h), byte for byte; the digests are what
        # tests/golden/make_mergecontigs.py --time prints for the unmodified reference on the same files
        build.build_hostcheck()
        t0 = time.perf_counter()
        h = subprocess.run([build.MC_CHECK, "run", "-k%d" % k, "-o", "h.fa", "-g", "h.dot", fa, adj, path], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        out["mc_check_seconds"] = round(time.perf_counter() - t0, 3)
        out["equals_host_check"] = read("h.fa") == read("o.fa") and read("h.dot") == read("o.dot") and h.stderr == r.stderr
        print(json.dumps(out), flush=True)
        if not out["equals_host_check"]:
            sys.exit("MergeContigs and the host check differ")


if __name__ == "__main__":
    main()
