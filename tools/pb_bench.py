#!/usr/bin/env python3
"""Times PopBubbles' alignment on two generated inputs:

  snp   about 92,000 contigs: a chain of 30,600 flanks of 300 bp with a SNP bubble between every two neighbours (two branches of
        2k - 1 bases, 1 x 1 cells once trimmed), every other branch stored reverse-complemented
  long  256 bubbles whose branches are 1 to 9 kb: the second branch is the first with 2 % substitutions and a few short indels

Prints one JSON line an input: the two kernels from events, cell updates a second, the flag bytes written a second against the HBM
peak, the abg_pb_align call, `PopBubbles` end to end, SHA-256 of its stdout and -g file and, with --host-check, whether
tests/hostcheck/pb_check writes the same bytes from the same files.

    python tools/pb_bench.py [--inputs snp,long] [--keep DIR] [--host-check]

write_inputs(dir, which) is what tests/golden/make_popbubbles.py --time runs the unmodified reference on."""
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
K = 64
HBM_BYTES_PER_S = 8e12  # MI355X: 8 TB/s peak
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def digest(data):
    return hashlib.sha256(data).hexdigest()[:16]


def rc(s):
    return s.translate(COMP)[::-1]


def build_set(which, seed=7):
    """(contigs [(name, bytes)], ADJ text, the pairs of trimmed branches the alignment sees)"""
    rng = np.random.default_rng(seed)
    dna = lambda n: LUT[rng.integers(0, 4, n)].tobytes()
    n = 30_600 if which == "snp" else 256
    flanks = [dna(300) for _ in range(n + 1)]
    contigs, lines, pairs = [], [], []
    name = lambda i: "f%d" % i
    for i in range(n):
        if which == "snp":
            a = dna(1)
            b = LUT[(b"ACGT".index(a) + 1 + int(rng.integers(0, 3))) % 4:][:1].tobytes()
        else:
            length = int(rng.integers(1000, 9001))
            a = dna(length)
            m = np.frombuffer(a, dtype=np.uint8).copy()
            at = rng.choice(length, length // 50, replace=False)
            m[at] = LUT[rng.integers(0, 4, len(at))]
            b = m.tobytes()
            for _ in range(4):  # two deletions and two insertions of 1..40 bases
                p, w = int(rng.integers(50, len(b) - 50)), int(rng.integers(1, 41))
                b = b[:p] + b[p + w:] if _ % 2 else b[:p] + dna(w) + b[p:]
        pairs.append((a, b))
        left, right = flanks[i], flanks[i + 1]
        for j, mid in enumerate((a, b)):
            seq = left[-(K - 1):] + mid + right[:K - 1]
            flip = (i + j) % 2 == 1
            contigs.append(("b%d_%d" % (i, j), rc(seq) if flip else seq, flip))
    out = []
    for i in range(n + 1):
        right = "" if i == n else "".join(" b%d_%d%s" % (i, j, "-" if contigs[2 * i + j][2] else "+") for j in range(2))
        left = "" if i == 0 else "".join(" b%d_%d%s" % (i - 1, j, "-" if contigs[2 * (i - 1) + j][2] else "+") for j in range(2))
        out.append("%s %d %d\t;%s\t;%s\n" % (name(i), 300, 30 * 300, right, left))
    for i in range(n):
        for j in range(2):
            nm, seq, flip = contigs[2 * i + j]
            # the branch as read forwards goes from flank i to flank i + 1; stored reverse-complemented, its + vertex goes back
            out.append("%s %d %d\t;%s\t;%s\n" % (nm, len(seq), (20 + 10 * j) * len(seq), " %s-" % name(i) if flip else " %s+" % name(i + 1),
                                                " %s-" % name(i + 1) if flip else " %s+" % name(i)))
    records = [(name(i), f) for i, f in enumerate(flanks)] + [(nm, seq) for nm, seq, _ in contigs]
    return records, "".join(out), pairs


def write_inputs(d, which):
    """(FASTA, graph, k) in d"""
    records, adj, _ = build_set(which)
    with open(os.path.join(d, which + ".fa"), "wb") as f:
        for nm, seq in records:
            f.write(b">%s\n%s\n" % (nm.encode(), seq))
    open(os.path.join(d, which + ".adj"), "w").write(adj)
    return which + ".fa", which + ".adj", K


def time_align(pairs, repeat=3):
    from abyss_amd import api
    al = api.BubbleAlign()
    al.align(pairs)  # warm-up: buffers and code object
    al.profile_reset()
    calls = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        matches, size, redone = al.align(pairs)
        calls.append(time.perf_counter() - t0)
    lane_ms, wave_ms = al.profile_get("pb_lane")[0] / repeat, al.profile_get("pb_wave")[0] / repeat
    cells, launches, redone_total = al.profile_get("pb_cells")[1] // repeat, al.profile_get("pb_launches")[1] // repeat, al.profile_get("pb_redone")[1]
    al.close()
    kernel_s = (lane_ms + wave_ms) * 1e-3
    return {"pairs": len(pairs), "cells": int(cells), "launches": int(launches), "lane_ms": round(lane_ms, 3), "wave_ms": round(wave_ms, 3),
            "cell_updates_per_s": round(cells / kernel_s) if kernel_s else None,
            "flag_bytes_per_s_share_of_hbm_peak": round(cells / kernel_s / HBM_BYTES_PER_S, 5) if kernel_s else None,  # a byte a cell
            "align_call_ms": round(1e3 * min(calls), 2), "redone_on_host": int(redone_total), "matches_sum": int(matches.sum()), "size_sum": int(size.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="snp,long")
    ap.add_argument("--keep")
    ap.add_argument("--host-check", action="store_true")
    a = ap.parse_args()
    from abyss_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        for which in a.inputs.split(","):
            records, _, pairs = build_set(which)
            fa, adj, k = write_inputs(d, which)
            out = {"input": which, "contigs": len(records), "k": k, "align": time_align(pairs)}
            exe = os.path.join(build.BIN_DIR, "PopBubbles")
            argv = ["-k%d" % k, "-g", which + ".out.adj", fa, adj]
            t0 = time.perf_counter()
            r = subprocess.run([exe] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            out["popbubbles_seconds"] = round(time.perf_counter() - t0, 3)
            read = lambda f: open(os.path.join(d, f), "rb").read()
            out["stdout_sha256"], out["graph_sha256"], out["popped"] = digest(r.stdout), digest(read(which + ".out.adj")), r.stdout.count(b"\n")
            if a.host_check:  # the same run over the serial text of abg_pb.h, byte for byte
                build.build_hostcheck()
                t0 = time.perf_counter()
                h = subprocess.run([build.PB_CHECK, "run", "-k%d" % k, "-g", which + ".host.adj", fa, adj], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
                out["pb_check_seconds"] = round(time.perf_counter() - t0, 3)
                out["equals_host_check"] = h.stdout == r.stdout and read(which + ".host.adj") == read(which + ".out.adj")
            print(json.dumps(out), flush=True)
            if a.host_check and not out["equals_host_check"]:
                sys.exit("PopBubbles and the host check differ")


if __name__ == "__main__":
    main()
