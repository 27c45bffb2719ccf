#!/usr/bin/env python3
"""Times SimpleGraph's search on two inputs.  `contigs`: the 92,000-contig files of tools/ov_bench.py run through our Overlap, so the
graph and the estimates are what the stage before writes at the shape of BASELINE.json configs[1]; nearly every search there takes a
handful of steps.  `bubbles`: ladders of bubbles, a few percent of them 17 rungs long with an estimate no path can meet, so that
those searches run to the cost cap of 100,000 visits beside thousands that take a few dozen.  Prints one JSON line per input: the
search kernel from events, the abg_sg_search call, the share of the kernel's wave steps taken with fewer than half the lanes busy,
the dependent-load chain the longest search must walk, and `SimpleGraph` end to end at default verbosity.

    python tools/sg_bench.py [--input contigs|bubbles|both] [--contigs N] [--ladders N] [--keep DIR]

write_inputs(dir, variant) is what tests/golden/make_simplegraph.py --time runs the unmodified reference on."""
import argparse
import hashlib
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
K_BUBBLES = 32
LOAD_LATENCY_NS = 85.0  # one dependent global load that hits L2 on MI355X: about 200 cycles at 2.4 GHz (a search's own graph is small)
LOADS_A_STEP = 4        # the serial loads of a step that pushes: the edge's target, two probes of the constraint list, the new vertex's edges


def _overlap(d, k, n, seed):
    """c.fa, c.adj, c.dist of ov_bench -> o.adj through our Overlap (the GPU binary, or the host check where there is no device)"""
    import ov_bench
    from abyss_amd import build
    ov_bench.write_inputs(d, n, seed)
    argv = ["-k%d" % k, "-g", "o.adj", "-o", "o.fa", "c.fa", "c.adj", "c.dist"]
    r = subprocess.run([os.path.join(build.BIN_DIR, "Overlap")] + argv, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if r.returncode == 0:
        return "Overlap"
    if b"no HIP device available" not in r.stderr:  # only the lack of a device sends the input through the host check
        sys.exit("Overlap failed: " + r.stderr.decode()[-500:])
    build.build_hostcheck()
    subprocess.run([build.OV_CHECK, "run"] + argv, cwd=d, stdout=subprocess.DEVNULL, check=True)
    return "ov_check"


def _ladders(d, n, hard_percent=3):
    """b.adj, b.dist: n ladders (s -> {a, b} -> s -> ...), rungs of 50 and 51 between spines of 100; ladder i has 3 rungs, or 17 and an
    estimate to a contig off the ladder when i falls in the hard share"""
    D = -(K_BUBBLES - 1)
    adj, dist = [], []
    for i in range(n):
        hard = i % 100 < hard_percent
        rungs = 17 if hard else 3
        p = "L%d" % i
        s = lambda r: "%ss%d" % (p, r)
        for r in range(rungs + 1):
            out = " %sa%d+ %sb%d+" % (p, r + 1, p, r + 1) if r < rungs else ""
            inn = " %sa%d+ %sb%d+" % (p, r, p, r) if r > 0 else ""
            adj.append("%s 100 1000\t;%s\t;%s\n" % (s(r), out, inn))
            if r < rungs:
                for b, l in (("a", 50), ("b", 51)):
                    adj.append("%s%s%d %d %d\t; %s+\t; %s+\n" % (p, b, r + 1, l, 10 * l, s(r + 1), s(r)))
        short = rungs * (D + 50) + (rungs - 1) * (D + 100) + D
        ests = [" %s+,%d,12,1.0" % (s(1), D + 50 + D), " %s+,%d,15,2.0" % (s(rungs), short + rungs // 2)]
        if hard:
            adj.append("%sx 80 800\t;\t;\n" % p)
            ests.append(" %sx+,3000,9,5.0" % p)
        dist.append("%s%s ;\n" % (s(0), "".join(ests)))
    open(os.path.join(d, "b.adj"), "w").write("".join(adj))
    open(os.path.join(d, "b.dist"), "w").write("".join(dist))


def digest(data):
    return hashlib.sha256(data).hexdigest()[:16]


def write_inputs(d, variant, contigs=92_000, ladders=20_000, seed=7):
    """(graph file, estimate file, k) in d"""
    if variant == "contigs":
        print(json.dumps({"overlap_run_by": _overlap(d, 64, contigs, seed)}), flush=True)
        return "o.adj", "c.dist", 64
    _ladders(d, ladders)
    return "b.adj", "b.dist", K_BUBBLES


def load(d, adj, dist, k, distance_error=6):
    """the pass of simplegraph_core.h in Python: (CSR graph, searches as api.PathSearch takes them)"""
    lines = [l for l in open(os.path.join(d, adj)).read().splitlines() if l.strip()]
    ids = {l.split(None, 1)[0]: i for i, l in enumerate(lines)}
    out = [[] for _ in range(2 * len(lines))]
    lengths = np.zeros(2 * len(lines), dtype=np.uint32)
    edge = re.compile(r"(\S+)([+-])(?:\s*\[d=(-?\d+)\])?")
    for i, l in enumerate(lines):
        head, right, left = l.split(";")
        lengths[2 * i] = lengths[2 * i + 1] = int(head.split()[1])
        for sense, part in ((0, right), (1, left)):
            for m in edge.finditer(part):
                v = 2 * ids[m.group(1)] + (m.group(2) == "-")
                out[2 * i + sense].append((v ^ sense, int(m.group(3)) if m.group(3) else -(k - 1)))
    off = np.zeros(len(out) + 1, dtype=np.uint64)
    np.cumsum([len(o) for o in out], out=off[1:])
    graph = (off, lengths, np.array([v for o in out for v, _ in o], dtype=np.uint32), np.array([x for o in out for _, x in o], dtype=np.int32))
    searches = []
    for l in open(os.path.join(d, dist)).read().splitlines():
        if not l.strip():
            continue
        name, rest = l.split(None, 1) if len(l.split(None, 1)) > 1 else (l.strip(), ";")
        sides = rest.split(";")
        ref = ids[name]
        for direction in (1, 0):  # the anterior side first, its vertices flipped
            cons = []
            for e in sides[direction].split():
                v, dd, _, sd = e.split(",")
                vertex = (2 * ids[v[:-1]] + (v[-1] == "-")) ^ direction
                cons.append((vertex, int(dd) + int(math.ceil(np.float32(3) * np.float32(sd) + np.float32(distance_error)))))
            if cons:
                searches.append((2 * ref + direction, cons))
    return graph, searches


def time_search(graph, searches, repeat=3):
    from abyss_amd import api
    ps = api.PathSearch()
    ps.set_graph(*graph)
    visited, redone, paths = ps.search(searches)  # warm-up: buffers and code object
    ps.profile(True)  # events only: the kernel as every run has it
    calls = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        ps.search(searches)
        calls.append(time.perf_counter() - t0)
    ms, launches = ps.profile_get("sg_search")
    ps.profile(True, count_steps=True)  # one more call in which the kernel counts its wave steps (two ballots a step: not timed)
    ps.search(searches)
    ms2, _ = ps.profile_get("sg_search")
    _, steps = ps.profile_get("sg_steps")
    _, thin = ps.profile_get("sg_thin_steps")
    ps.close()
    longest = int(visited.max()) if len(visited) else 0
    chain_ms = longest * LOADS_A_STEP * LOAD_LATENCY_NS * 1e-6
    kernel_ms = ms / repeat
    return {"searches": len(searches), "kernel_ms": round(kernel_ms, 3), "launches": launches // repeat, "search_call_ms": round(1e3 * min(calls), 2),
            "wave_steps": steps, "thin_share": round(thin / steps, 4) if steps else None, "longest_search_visits": longest,
            "at_cost_cap": int((visited >= 100000).sum()), "redone_on_host": int(redone.sum()), "paths": sum(len(p) for p in paths),
            "kernel_ms_while_counting": round(ms2 - ms, 3), "latency_bound_ms": round(chain_ms, 2), "kernel_over_bound": round(kernel_ms / chain_ms, 2) if chain_ms else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="both", choices=["contigs", "bubbles", "both"])
    ap.add_argument("--contigs", type=int, default=92_000)
    ap.add_argument("--ladders", type=int, default=20_000)
    ap.add_argument("--keep")
    a = ap.parse_args()
    from abyss_amd import build
    for variant in (["contigs", "bubbles"] if a.input == "both" else [a.input]):
        with tempfile.TemporaryDirectory() as tmp:
            d = a.keep or tmp
            os.makedirs(d, exist_ok=True)
            adj, dist, k = write_inputs(d, variant, a.contigs, a.ladders)
            out = {"input": variant, "k": k}
            t0 = time.perf_counter()
            graph, searches = load(d, adj, dist, k)
            out["python_load_seconds"] = round(time.perf_counter() - t0, 2)
            out["vertices"], out["edges"] = len(graph[1]), len(graph[2])
            out["search"] = time_search(graph, searches)
            exe = os.path.join(build.BIN_DIR, "SimpleGraph")
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-k%d" % k, "-o", "o.path", adj, dist], cwd=d, stdout=subprocess.PIPE, check=True)
            out["simplegraph_seconds"] = round(time.perf_counter() - t0, 3)
            out["summary"] = r.stdout.decode().split("\n")[3:11]
            # the same run by the host check (the search body run serially), byte for byte; the digests are what
            # tests/golden/make_simplegraph.py --time prints for the unmodified reference on the same files
            paths = open(os.path.join(d, "o.path"), "rb").read()
            build.build_hostcheck()
            h = subprocess.run([build.SG_CHECK, "run", "-k%d" % k, "-o", "h.path", adj, dist], cwd=d, stdout=subprocess.PIPE, check=True)
            out["equals_host_check"] = h.stdout == r.stdout and open(os.path.join(d, "h.path"), "rb").read() == paths
            out["path_lines"], out["path_sha256"], out["stdout_sha256"] = paths.count(b"\n"), digest(paths), digest(r.stdout)
            if not out["equals_host_check"]:
                print(json.dumps(out), flush=True)
                sys.exit("SimpleGraph and the host check differ on " + variant)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
