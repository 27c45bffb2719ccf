#!/usr/bin/env python3
"""Times abyss-mergepairs' alignment on N generated pairs of 2 x 150 bp: fragments of 100 to 450 bp (a third of them too long to
overlap), 1 % substitutions, qualities 2 to 40.

Prints one JSON line: the kernel from events (abg_mp_profile_get), cell updates a second, the shares of pairs whose last row the
host sorted, that went out again, and that the host aligned; the abg_mp_align call; `abyss-mergepairs` end to end with the
SHA-256 of its stdout and of its three files and, with --host-check, whether tests/hostcheck/mp_check writes the same bytes from
the same files.

    python tools/mp_bench.py [--pairs 1000000] [--keep DIR] [--host-check] [--skip-binary]

write_inputs(dir, n) is what tests/golden/make_mergepairs.py --time runs the unmodified reference on."""
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
READ = 150
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
SUFFIXES = ("_merged.fastq", "_reads_1.fastq", "_reads_2.fastq")


def digest(data):
    return hashlib.sha256(data).hexdigest()[:16]


def build_pairs(n, seed=11):
    """(reads 1, reads 2) as (n, 150) arrays of bytes, read 2 as the file holds it"""
    rng = np.random.default_rng(seed)
    frag = rng.integers(100, 451, n)
    genome = LUT[rng.integers(0, 4, (n, 450 + READ))]  # the fragment, then what the sequencer reads past its end
    one = genome[:, :READ].copy()
    two = np.empty((n, READ), dtype=np.uint8)
    for f in np.unique(frag):  # read 2: the last 150 bases of the fragment (adapter where it is shorter), reverse-complemented
        rows = np.nonzero(frag == f)[0]
        if f >= READ:
            seg = genome[rows, f - READ:f]
        else:
            seg = np.concatenate([LUT[rng.integers(0, 4, (len(rows), READ - f))], genome[rows, :f]], axis=1)
            one[rows, f:] = LUT[rng.integers(0, 4, (len(rows), READ - f))]
        two[rows] = COMP[seg[:, ::-1]]
    for reads in (one, two):
        hit = rng.random(reads.shape) < 0.01
        reads[hit] = LUT[rng.integers(0, 4, int(hit.sum()))]
    return one, two


def write_inputs(d, n):
    one, two = build_pairs(n)
    rng = np.random.default_rng(12)
    names = []
    for which, reads in (("1", one), ("2", two)):
        qual = (33 + rng.integers(2, 41, reads.shape)).astype(np.uint8)
        name = "mp_%d_%s.fq" % (n, which)
        with open(os.path.join(d, name), "wb") as f:
            for at in range(0, n, 100000):
                f.write(b"".join(b"@p%d/%s\n%s\n+\n%s\n" % (i, which.encode(), reads[i].tobytes(), qual[i].tobytes()) for i in range(at, min(n, at + 100000))))
        names.append(name)
    return names


def time_align(n, repeat=3):
    from abyss_amd import api
    one, two = build_pairs(n)
    pairs = [(one[i].tobytes(), two[i].tobytes()) for i in range(n)]
    al = api.PairMerge()
    al.align(pairs[:min(n, 70000)])  # warm-up: buffers and code object
    al.profile_reset()
    calls = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        rec = al.align(pairs)
        calls.append(time.perf_counter() - t0)
    wave_ms = al.profile_get("mp_wave")[0] / repeat
    get = lambda name: al.profile_get(name)[1] // repeat
    cells, launches, spilled, host, again = get("mp_cells"), get("mp_launches"), get("mp_spilled"), get("mp_host"), get("mp_relaunched")
    al.close()
    return {"pairs": n, "cells": int(cells), "launches": int(launches), "wave_ms": round(wave_ms, 3), "cell_updates_per_s": round(cells / (wave_ms * 1e-3)) if wave_ms else None,
            "kernel_us_a_pair": round(1e3 * wave_ms / n, 4), "spilled_share": round(spilled / n, 5), "relaunched_share": round(again / n, 5), "host_share": round(host / n, 5),
            "align_call_ms": round(1e3 * min(calls), 2), "merged": int((rec[:, 3] == 1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--keep")
    ap.add_argument("--host-check", action="store_true")
    ap.add_argument("--skip-binary", action="store_true")
    a = ap.parse_args()
    from abyss_amd import build
    out = {"pairs": a.pairs, "read_length": READ, "align": time_align(a.pairs)}
    if not a.skip_binary:
        with tempfile.TemporaryDirectory() as tmp:
            d = a.keep or tmp
            os.makedirs(d, exist_ok=True)
            f1, f2 = write_inputs(d, a.pairs)
            read = lambda prefix: b"".join(open(os.path.join(d, prefix + s), "rb").read() for s in SUFFIXES)
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(build.BIN_DIR, "abyss-mergepairs"), "-o", "gpu", f1, f2], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            out["mergepairs_seconds"] = round(time.perf_counter() - t0, 3)
            out["stdout_sha256"], out["files_sha256"], out["stats"] = digest(r.stdout), digest(read("gpu")), r.stderr.decode().strip().splitlines()[-2:]
            if a.host_check:  # the same run over the serial text of abg_mp.h, byte for byte
                build.build_hostcheck()
                t0 = time.perf_counter()
                h = subprocess.run([build.MP_CHECK, "run", "-o", "host", f1, f2], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
                out["mp_check_seconds"] = round(time.perf_counter() - t0, 3)
                out["host_stdout_sha256"], out["host_files_sha256"] = digest(h.stdout), digest(read("host"))
                out["equals_host_check"] = h.stdout == r.stdout and h.stderr == r.stderr and read("host") == read("gpu")
    print(json.dumps(out), flush=True)
    if out.get("equals_host_check") is False:
        sys.exit("abyss-mergepairs and the host check differ")


if __name__ == "__main__":
    main()
