#!/usr/bin/env python3
"""Times Overlap's search at the shape of BASELINE.json configs[1]: 92,000 contigs along a genome, every junction a candidate from
both of its contigs.  Prints one JSON line: the search kernel from events, the abg_ov_find call, the bytes a search must read at
least and what that costs at HBM speed, and `Overlap` end to end at default verbosity.  --worst adds the low-complexity case: two
100 kb contigs whose junction is a period-3 repeat, where no lane leaves early.

    python tools/ov_bench.py [--contigs N] [--seed S] [--worst] [--keep DIR]

write_inputs(dir, n, seed) is what tests/golden/make_overlap.py --time runs the unmodified reference on."""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 64
HBM_BYTES_PER_S = 8e12  # MI355X: 8 TB/s peak


def revcomp(a):
    return (3 - a)[::-1]


def simulate(n, seed):
    """contigs of 200..3000 bp as 2-bit codes; junction i joins contig i and i + 1: an overlap of 5..K-2 bases (half of them), a gap
    of 1..200 (a third) or nothing in common at d <= 0.  Every other contig is stored reverse-complemented."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(200, 3001, n)
    kinds = rng.integers(0, 6, n - 1)
    seqs, dists = [], []
    prev = rng.integers(0, 4, lens[0], dtype=np.uint8)
    seqs.append(prev)
    for i in range(1, n):
        body = rng.integers(0, 4, lens[i], dtype=np.uint8)
        kd = kinds[i - 1]
        if kd < 3:
            ov = int(rng.integers(5, K - 1))
            body[:ov] = prev[-ov:]
            dists.append(-ov)
        elif kd < 5:
            dists.append(int(rng.integers(1, 201)))
        else:
            dists.append(-int(rng.integers(0, 4)))
        seqs.append(body)
        prev = body
    return seqs, dists


def write_inputs(d, n, seed):
    """c.fa, c.adj (no edges: every end is blunt), c.dist; returns (contigs as stored, pairs as 2 * id + sense)"""
    seqs, dists = simulate(n, seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    stored = [revcomp(s) if i % 2 else s for i, s in enumerate(seqs)]
    with open(os.path.join(d, "c.fa"), "wb") as f:
        for i, s in enumerate(stored):
            f.write(b">%d\n" % i)
            f.write(lut[s].tobytes())
            f.write(b"\n")
    with open(os.path.join(d, "c.adj"), "w") as f:
        for i, s in enumerate(stored):
            f.write("%d %d %d\t;\t;\n" % (i, len(s), 30 * len(s)))
    node = lambda i, flip=False: "%d%s" % (i, "-" if (i % 2 == 1) != flip else "+")
    right = [[] for _ in range(n)]
    left = [[] for _ in range(n)]
    pairs = []
    for i, dd in enumerate(dists):
        a, b = i, i + 1
        e = ",%d,20,3.0" % dd
        # seen from a and from b, as DistanceEst writes both
        for ref in (a, b):
            t, h = (node(a), node(b))
            if t != "%d+" % ref and h != "%d+" % ref:
                t, h = node(b, True), node(a, True)
            (right if t == "%d+" % ref else left)[ref].append((h if t == "%d+" % ref else t) + e)
        pairs.append((2 * a + (a % 2), 2 * b + (b % 2)))
    with open(os.path.join(d, "c.dist"), "w") as f:
        for i in range(n):
            f.write("%d %s ; %s\n" % (i, " ".join(right[i]), " ".join(left[i])))
    return [lut[s].tobytes() for s in stored], pairs


def time_find(contigs, pairs, repeat=3, all=False):
    from abyss_amd import api
    co = api.ContigOverlap()
    co.set_contigs(contigs)
    p = np.asarray(pairs, dtype=np.uint32)
    co.find(p, all=all)  # warm-up: buffers and code object
    co.profile(True)
    calls = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        top, n = co.find(p, all=all)
        calls.append(time.perf_counter() - t0)
    if all:
        n = np.diff(n.astype(np.int64))
    ms, launches = co.profile_get("ov_search")
    _, nbytes = co.profile_get("ov_search_bytes")
    co.close()
    kernel_ms = ms / repeat
    bound_ms = nbytes / repeat / HBM_BYTES_PER_S * 1e3
    return {"pairs": len(p), "kernel_ms": round(kernel_ms, 4), "launches": launches // repeat, "find_call_ms": round(1e3 * min(calls), 3),
            "min_bytes": nbytes // repeat, "hbm_bound_ms": round(bound_ms, 5), "kernel_over_bound": round(kernel_ms / bound_ms, 1) if bound_ms else None,
            "with_match": int((n > 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=92_000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--keep")
    a = ap.parse_args()
    from abyss_amd import build
    out = {"contigs": a.contigs}
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        contigs, pairs = write_inputs(d, a.contigs, a.seed)
        both = pairs + [(h ^ 1, t ^ 1) for t, h in pairs]  # every junction in both directions
        out["search"] = time_find(contigs, both)
        exe = os.path.join(build.BIN_DIR, "Overlap")
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-k%d" % K, "-g", "o.adj", "-o", "o.fa", "c.fa", "c.adj", "c.dist"], cwd=d, stdout=subprocess.PIPE, check=True)
        out["overlap_seconds"] = round(time.perf_counter() - t0, 3)
        out["summary"] = r.stdout.decode().split("\n")[:7]
    if a.worst:
        unit = "ACG"
        rep = (unit * 40000)[:100_000 - 1]
        t = ("T" + rep).encode()
        h = (rep + "T").encode()
        out["worst_period3_100kb_top"] = time_find([t, h], [(0, 2)], repeat=1)          # stops at the third match, in the first step
        out["worst_period3_100kb_all"] = time_find([t, h], [(0, 2)], repeat=1, all=True)  # every l is compared, a third of them to the end
    print(json.dumps(out))


if __name__ == "__main__":
    main()
