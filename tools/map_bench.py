#!/usr/bin/env python3
"""map_bench.py -- reads/s of the FM-index read mapping (abg_fm_*, abyss_amd/bin/abyss-map) on one MI355X.

The target is built with the library: a synthetic genome (abyss_amd.synth, as bench.py's configs[1] at --genome-mbp 30: 50x of
2x150 bp reads with 0.5 % substitution errors) is assembled into unitigs by api.BloomDBG (k=64, H=4), and the unitigs, one FASTA
record each, are the text.  --reads of those reads are mapped with -l40 (abyss-pe's default l).

Timed: abg_fm_build and abg_fm_map_seqs through the profile API (events around the kernels, the reads already in host memory in
the ABI's block form; the search steps come from the same API), and abyss-map end to end, process start to last SAM record, the
median of --runs runs spaced 3 s apart (notes/README.md).  One JSON line on stdout.
    python tools/map_bench.py [--genome-mbp 30] [--reads 2000000] [--runs 3] [--sweep 2,4,8,16,32] > profiles/<name>.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abyss_amd import api, build, synth  # noqa: E402

IC_GATHER_BYTES_PER_S = 8.6e12  # MI355X, uniformly random rows of a 38 MB table served by the Infinity Cache


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=30.0)
    ap.add_argument("--coverage", type=float, default=50.0)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--min-len", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sweep", default="", help="waves a CU to time the search kernel at, e.g. 2,4,8,16,32 (abg_fm_tune)")
    a = ap.parse_args()
    k = 64
    genome = int(a.genome_mbp * 1e6)
    t0 = time.time()
    m1, m2 = synth.make_read_set(genome, a.coverage)
    ascii_reads = synth.codes_to_ascii(np.concatenate([m1, m2]))
    del m1, m2
    buf, off = api.matrix_to_seqs(ascii_reads)
    g = api.BloomDBG(k, bloom_bytes=int(min(2 << 30, max(1 << 26, genome * 64))))
    g.load(buf, off)
    _, contigs = g.assemble(buf, off)
    g.close()
    target = b"".join(b">%d\n%s\n" % (i, c.seq) for i, c in enumerate(c for c in contigs if not c.redundant))
    n_unitigs = target.count(b">")
    del contigs
    n_reads = min(a.reads, len(off) - 1)
    read_len = int(off[1] - off[0])
    rbuf, roff = buf[:int(off[n_reads])], off[:n_reads + 1]
    setup_s = time.time() - t0

    fm = api.FMIndex()
    fm.profile(True)
    t0 = time.time()
    fm.build(target)
    build_wall = time.time() - t0
    sa_ms, occ_ms = fm.profile_get("fm_sa")[0], fm.profile_get("fm_occ")[0]
    fm.profile(False)
    fm.map(rbuf[:int(roff[10000])], roff[:10001], a.min_len)  # warm-up: buffers sized, memo cleared
    fm.map(rbuf, roff, a.min_len)
    fm.profile(True)
    t0 = time.time()
    hits = fm.map(rbuf, roff, a.min_len)
    map_wall = time.time() - t0
    map_ms = fm.profile_get("fm_map")[0]
    steps = fm.profile_get("fm_map_steps")[1]
    sweep = []
    for waves in [int(w) for w in a.sweep.split(",") if w]:  # kernel time of the same call at other lane counts, each after a warm-up call
        fm.tune(waves)
        fm.profile(False)
        fm.map(rbuf, roff, a.min_len)
        fm.profile(True)
        before = fm.profile_get("fm_map")[0]
        fm.map(rbuf, roff, a.min_len)
        ms = fm.profile_get("fm_map")[0] - before
        sweep.append({"waves_per_cu": waves, "kernel_ms": round(ms, 3), "reads_per_s_kernel": round(n_reads / (ms / 1e3))})
    fm.close()
    span = hits["qend"].astype(np.int64) - hits["qstart"]
    mapped = int(((hits["u"] > hits["l"]).any(axis=1)).sum())
    sectors_per_s = 2 * steps / (map_ms / 1e3)
    out = {
        "what": "FM-index read mapping, one MI355X: abg_fm_build / abg_fm_map_seqs (kernel time, profile API) and abyss-map end to end",
        "genome_bp": genome, "coverage": a.coverage, "k": k, "unitigs": n_unitigs, "target_bytes": len(target),
        "occ_table_bytes": (len(target) + 1) // 128 * 64 + 64, "reads": n_reads, "read_length": read_len, "min_len": a.min_len,
        "setup_s": round(setup_s, 2),
        "build": {"wall_s": round(build_wall, 4), "fm_sa_ms": round(sa_ms, 3), "fm_occ_ms": round(occ_ms, 3)},
        "map": {"kernel_ms": round(map_ms, 3), "call_wall_s": round(map_wall, 4), "reads_per_s_kernel": round(n_reads / (map_ms / 1e3)),
                "reads_per_s_call": round(n_reads / map_wall), "steps": int(steps), "steps_per_read": round(steps / n_reads, 1),
                "sectors_per_s": round(sectors_per_s), "gather_bytes_per_s": round(sectors_per_s * 64),
                "fraction_of_infinity_cache_gather_rate": round(sectors_per_s * 64 / IC_GATHER_BYTES_PER_S, 4),
                "mapped": mapped, "full_length": int((span.max(axis=1) == read_len).sum())},
    }
    if sweep:
        out["wave_sweep"] = sweep
    if a.runs > 0:
        build.build_cli()
        with tempfile.TemporaryDirectory() as td:
            open(os.path.join(td, "target.fa"), "wb").write(target)
            with open(os.path.join(td, "reads.fa"), "wb") as f:
                rows = ascii_reads[:n_reads]
                ids = np.char.add(np.char.add(">r", np.arange(n_reads).astype(str)), "\n").astype("S")
                for i in range(0, n_reads, 200000):
                    f.write(b"".join(h + r.tobytes() + b"\n" for h, r in zip(ids[i:i + 200000], rows[i:i + 200000])))
            times = []
            for r in range(a.runs):
                if r:
                    time.sleep(3)
                t0 = time.time()
                p = subprocess.run([os.path.join(build.BIN_DIR, "abyss-map"), "-j16", "-l%d" % a.min_len, "reads.fa", "target.fa"], cwd=td,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
                times.append(time.time() - t0)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr.decode())
                    return 1
            med = statistics.median(times)
            out["end_to_end"] = {"what": "abyss_amd/bin/abyss-map -j16 -l%d reads.fa target.fa, process start to last record, FASTA on local disk" % a.min_len,
                                 "seconds": [round(t, 3) for t in times], "median_s": round(med, 3), "reads_per_s": round(n_reads / med),
                                 "sam_records": p.stdout.count(b"\n") - 2 - n_unitigs}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
