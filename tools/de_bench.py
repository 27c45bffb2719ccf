#!/usr/bin/env python3
"""de_bench.py -- the rates of DistanceEst's maximum-likelihood estimate (abg_de_*, abyss_amd/bin/DistanceEst) on one MI355X.

Synthetic, at the size of bench.py's configs[1]: the contig pairs that --contigs unitigs (92,000) give with -s1000 and a 400 +- 40 bp
FR library, both directions of every junction, --pairs read pairs a junction; and a wide library (insert 22,000 +- 1,500, a PMF too
long for LDS) with --wide-jobs pairs.  Timed: the scan kernel through the profile API (terms = PMF entries x thetas, per second),
the whole abg_de_estimate call (host preparation, scan, tail), and the binary end to end on a SAM file of --records records
(process start to exit, the median of --runs runs).  One JSON line on stdout.
    python tools/de_bench.py [--contigs 92000] [--records 10000000] [--runs 3] > profiles/<name>.json
write_sam() also makes the input of `tests/golden/make_distanceest.py --time`, the CPU figure.
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

K, L, READ = 64, 40, 100


def normal_hist(mean, sd, n, seed):
    rng = np.random.default_rng(seed)
    v = np.rint(rng.normal(mean, sd, n)).astype(np.int64)
    return np.bincount(v[v > 0])


def write_hist(path, hist):
    with open(path, "w") as f:
        for v in np.nonzero(hist)[0]:
            f.write("%d\t%d\n" % (v, hist[v]))


def pmf_of(hist):
    """Common/PMF.h over the histogram as it is (dense enough that the clean-up chain leaves it alone but for its far tails)"""
    nz = np.nonzero(hist)[0]
    h = hist[:nz[-1] + 1].astype(np.float64)
    count = h.sum()
    minp = 1.0 / count
    return np.where(h > 0, h / count, minp), minp, float((np.arange(len(h)) * h).sum() / count)


def contig_lengths(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1000, 4000, n)  # every one a seed contig: the job count is the point


def write_sam(path, hist_path, records, contigs, seed):
    """a sorted SAM of `records` records: every junction of `contigs` contigs spanned by FR pairs of a 400 +- 40 bp library, each
    pair one record in either contig's group; the histogram beside it"""
    rng = np.random.default_rng(seed)
    lens = contig_lengths(contigs, seed)
    write_hist(hist_path, normal_hist(400, 40, 2_000_000, seed + 1))
    per = max(1, records // (2 * (contigs - 1)))
    gaps = np.where(rng.random(contigs - 1) < 0.5, -(K - 1), rng.integers(1, 120, contigs - 1))
    with open(path, "w") as f:
        f.write("".join("@SQ\tSN:%d\tLN:%d\n" % (i, n) for i, n in enumerate(lens)))
        left = None  # the records of junction (i - 1, i) that belong to contig i
        for i in range(contigs):
            out = left or []
            if i + 1 < contigs:
                frag = np.maximum(2 * READ + 1 + max(int(gaps[i]), 0), np.rint(rng.normal(400, 40, per)).astype(np.int64))
                span = frag - gaps[i]                      # the provisional fragment: bases in i plus bases in i + 1
                u = rng.integers(READ, span - READ + 1)    # bases of the fragment in contig i
                pos = lens[i] - u                          # forward read in i, 0-based
                mend = span - u                            # end of the reverse read in i + 1
                mpos = mend - READ
                out += ["p%d_%d/1\t97\t%d\t%d\t60\t%dM\t%d\t%d\t%d\t*\t*\n" % (i, j, i, pos[j] + 1, READ, i + 1, mpos[j] + 1, mend[j] - pos[j])
                        for j in range(per)]
                left = ["p%d_%d/2\t145\t%d\t%d\t60\t%dM\t%d\t%d\t%d\t*\t*\n" % (i, j, i + 1, mpos[j] + 1, READ, i, pos[j] + 1, pos[j] - mend[j])
                        for j in range(per)]
            f.write("".join(out))
    return 2 * per * (contigs - 1)


def job_set(contigs, pairs, mean, sd, max_dist, seed, lo=1000, hi=4000):
    """(pairs, samples, offsets) of api.DistanceMLE.estimate: both directions of every junction"""
    from abyss_amd import api
    rng = np.random.default_rng(seed)
    n = 2 * (contigs - 1)
    lens = rng.integers(lo, hi, contigs)
    gaps = np.repeat(np.where(rng.random(contigs - 1) < 0.5, -(K - 1), rng.integers(1, 120, contigs - 1)), 2)
    p = np.zeros(n, dtype=api.DE_PAIR)
    p["first"], p["last"], p["l"], p["rf"] = -(K - 1), max_dist, L, 0
    p["len0"] = np.repeat(lens[:-1], 2)
    p["len1"] = np.repeat(lens[1:], 2)
    samples = np.maximum(2 * L, np.rint(rng.normal(mean, sd, n * pairs)).astype(np.int64) - np.repeat(gaps, pairs)).astype(np.int32)
    return p, samples, np.arange(n + 1, dtype=np.uint64) * pairs


def time_estimate(m, pairs, samples, offsets, npmf, runs):
    m.estimate(pairs[:64], samples[:int(offsets[64])], offsets[:65])  # warm-up: buffers, code object
    walls, kernel, terms = [], [], 0
    for _ in range(runs):
        m.profile(True)
        ms0, _ = m.profile_get("de_scan")
        _, t0 = m.profile_get("de_scan_terms")
        w = time.time()
        m.estimate(pairs, samples, offsets)
        walls.append(time.time() - w)
        ms1, _ = m.profile_get("de_scan")
        _, t1 = m.profile_get("de_scan_terms")
        m.profile(False)
        kernel.append((ms1 - ms0) / 1e3)
        terms = t1 - t0
        time.sleep(1)
    k, w = statistics.median(kernel), statistics.median(walls)
    return {"jobs": len(pairs), "pmf_entries": npmf, "terms": int(terms), "scan_kernel_s": round(k, 4), "terms_per_s": round(terms / k, 0),
            "estimate_call_s": round(w, 4), "jobs_per_s": round(len(pairs) / w, 0)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=92000)
    ap.add_argument("--pairs", type=int, default=54)
    ap.add_argument("--wide-jobs", type=int, default=64)
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from abyss_amd import api, build
    out = {"contigs": a.contigs}
    m = api.DistanceMLE()
    pmf, minp, mean = pmf_of(normal_hist(400, 40, 2_000_000, 8))
    m.set_pmf(pmf, minp, mean)
    out["pe_400_40"] = time_estimate(m, *job_set(a.contigs, a.pairs, 400, 40, len(pmf) - 1, 3), len(pmf), a.runs)
    for block in (64, 128):  # the one knob: thetas a workgroup
        m.tune(block)
        out["pe_400_40"]["scan_kernel_s_block%d" % block] = time_estimate(m, *job_set(a.contigs, a.pairs, 400, 40, len(pmf) - 1, 3), len(pmf), 1)["scan_kernel_s"]
    m.tune(0)
    pmf, minp, mean = pmf_of(normal_hist(22000, 1500, 40_000_000, 9))
    m.set_pmf(pmf, minp, mean)
    out["wide_22000_1500"] = time_estimate(m, *job_set(a.wide_jobs // 2 + 1, 200, 22000, 1500, len(pmf) - 1, 4, 40000, 60000), len(pmf), a.runs)
    m.close()

    build.build_cli()
    exe = os.path.join(build.BIN_DIR, "DistanceEst")
    with tempfile.TemporaryDirectory() as td:
        sam, hist = os.path.join(td, "big.sam"), os.path.join(td, "big.hist")
        t0 = time.time()
        n = write_sam(sam, hist, a.records, a.contigs, 7)
        out["end_to_end"] = {"records": n, "sam_bytes": os.path.getsize(sam), "make_sam_s": round(time.time() - t0, 1)}
        for label, extra in (("mle_j16", ["-j16"]), ("mle_j1", ["-j1"]), ("median_j16", ["-j16", "--median"])):
            walls = []
            for _ in range(a.runs):
                with open(sam, "rb") as f:
                    t0 = time.time()
                    subprocess.run([exe, "-k%d" % K, "-l%d" % L, "-s1000", "-n10", "-o", os.path.join(td, "o.dist"), hist] + extra, stdin=f, check=True)
                    walls.append(time.time() - t0)
                time.sleep(1)
            out["end_to_end"][label + "_s"] = round(statistics.median(walls), 3)
        out["end_to_end"]["records_per_s_mle_j16"] = round(n / out["end_to_end"]["mle_j16_s"], 0)
        out["end_to_end"]["estimates"] = sum(l.count(",") // 3 for l in open(os.path.join(td, "o.dist")))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
