"""Shared by the DistanceEst tests: the goldens of tests/golden/distanceest (made by tests/golden/make_distanceest.py from the
unmodified reference), job files of tests/hostcheck/de_check, the small shapes of the scan tests and a plain-Python restatement of
the scan (DistanceEst/MLE.cpp:84-98, 125-129) that owes nothing to abg_de.h."""
import functools
import json
import math
import os
import random
import re
import struct
import subprocess

import numpy as np

import golden_archive

HERE = os.path.dirname(os.path.abspath(__file__))
JOB = np.dtype([("first", "<i4"), ("last", "<i4"), ("len0", "<u4"), ("len1", "<u4")])
PAIR = np.dtype([("first", "<i4"), ("last", "<i4"), ("len0", "<u4"), ("len1", "<u4"), ("l", "<u4"), ("rf", "<u4")])

_files, golden, cases = golden_archive.bind("distanceest")


def rules():
    return json.load(open(os.path.join(HERE, "golden", "distanceest_rules.json")))


def is_mle(case):
    return "--mean" not in case["argv"] and "--median" not in case["argv"]


def needs_device(case):
    """whether abyss_amd/bin/DistanceEst reaches the estimator on this case: an MLE run that gets as far as a contig pair"""
    return is_mle(case) and not case["name"].startswith("error.") or case["name"] == "error.unsorted"


def run_case(prefix, case, tmp, env=None, argv=None):
    """runs `prefix + argv` in tmp as the generator ran the reference: (status, stdout, stderr, -o file or None)"""
    tmp = str(tmp)
    with open(os.path.join(tmp, case["hist"].split(".", 1)[1]), "wb") as f:
        f.write(golden(case["hist"]))
    e = dict(os.environ)
    e.pop("COLUMNS", None)
    e.update(env or {})
    r = subprocess.run(list(prefix) + list(argv if argv is not None else case["argv"]), cwd=tmp, input=golden(case["sam"]), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=e, timeout=120)
    written = None
    if case["out_file"]:
        p = os.path.join(tmp, case["out_file"])
        if os.path.exists(p):
            written = open(p, "rb").read()
            os.remove(p)
    return r.returncode, r.stdout, r.stderr.decode(), written


def check_case(case, got):
    """every byte of stdout, the -o file, stderr and the status against what the reference wrote"""
    status, out, err, written = got
    assert status == case["status"], err
    want_out = golden(case["stdout"]) if case["stdout"] else case["stdout_text"].encode()
    assert out == want_out
    assert written == (golden(case["out"]) if case["out"] else None)
    # (getopt's own message names argv[0], which the reference was run as through PATH)
    assert [re.sub(r"^\S*/(DistanceEst|de_check): ", "DistanceEst: ", ln) for ln in err.splitlines()] == case["stderr"].splitlines()


# ---- job files (tests/hostcheck/de_check.cc)

def write_jobs(path, pmf, minp, mean, jobs, values, counts, offsets):
    with open(path, "wb") as f:
        f.write(struct.pack("<Qdd", len(pmf), minp, mean))
        f.write(np.asarray(pmf, dtype="<f8").tobytes())
        f.write(struct.pack("<Q", len(jobs)))
        f.write(np.asarray(jobs, dtype=JOB).tobytes())
        f.write(np.asarray(offsets, dtype="<u8").tobytes())
        f.write(np.asarray(values, dtype="<i4").tobytes())
        f.write(np.asarray(counts, dtype="<u4").tobytes())


def read_jobs(path):
    """a job file, with what `de_check dump` appends where it is there"""
    b = open(path, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(b, dtype=dtype, count=n, offset=at)
        at += a.nbytes
        return a
    npmf, minp, mean = struct.unpack_from("<Qdd", b, 0)
    at = 24
    out = {"minp": minp, "mean": mean, "pmf": take("<f8", npmf)}
    nj = int(take("<u8", 1)[0])
    out["jobs"] = take(JOB, nj)
    out["offsets"] = take("<u8", nj + 1)
    out["values"] = take("<i4", int(out["offsets"][nj]))
    out["counts"] = take("<u4", int(out["offsets"][nj]))
    if at < len(b):
        out["pairs"] = take(PAIR, nj)
        out["sample_offsets"] = take("<u8", nj + 1)
        out["samples"] = take("<i4", int(out["sample_offsets"][nj]))
        out["labels"] = open(path + ".labels").read().splitlines()
    assert at == len(b)
    return out


def thetas(jobs):
    return [max(0, int(j["last"]) - int(j["first"]) + 1) for j in jobs]


def read_scan(path, jobs):
    """(c, L, n) as de_check scan wrote them, job after job"""
    b = open(path, "rb").read()
    c, like, n, at = [], [], [], 0
    for t in thetas(jobs):
        c.append(np.frombuffer(b, "<f8", t, at))
        like.append(np.frombuffer(b, "<f8", t, at + 8 * t))
        n.append(np.frombuffer(b, "<u4", t, at + 16 * t))
        at += 20 * t
    assert at == len(b)
    cat = lambda x, d: np.concatenate(x) if x else np.zeros(0, d)  # noqa: E731
    return cat(c, "<f8"), cat(like, "<f8"), cat(n, "<u4")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32),
                                                 b.view(np.uint64 if b.dtype.itemsize == 8 else np.uint32))


# ---- the scan restated: plain float loops in the reference's order

def py_scan(pmf, minp, jobs, values, counts, offsets):
    pmf = [float(p) for p in pmf]
    npmf = len(pmf)
    logp = [math.log(p) for p in pmf]
    logminp = math.log(minp)
    c_out, l_out, n_out = [], [], []
    for j, job in enumerate(jobs):
        first, last, x1, x2 = int(job["first"]), int(job["last"]), int(job["len0"]), int(job["len1"])
        x3 = x1 + x2
        sv = [int(v) for v in values[int(offsets[j]):int(offsets[j + 1])]]
        sc = [int(v) for v in counts[int(offsets[j]):int(offsets[j + 1])]]
        for theta in range(first, last + 1):
            c = 0.0
            for i in range(npmf):
                x = i - theta
                num = 1 if x <= 0 else x if x < x1 else x1 if x < x2 else x3 - x if x < x3 else 1
                c += pmf[i] * (num / x1)
            like, n = 0.0, 0
            for x, k in zip(sv, sc):
                i = x + theta
                if 0 <= i < npmf:
                    p, lp = pmf[i], logp[i]
                else:
                    p, lp = minp, logminp
                like += k * lp
                if p > minp:
                    n += k
            c_out.append(c)
            l_out.append(like)
            n_out.append(n)
    return np.array(c_out, dtype=np.float64), np.array(l_out, dtype=np.float64), np.array(n_out, dtype=np.uint32)


def make_pmf(rng, size):
    """as Common/PMF.h makes one: n / count, or 1 / count where n is 0"""
    n = [rng.choice([0, 0, 1, 2, 3, 7, 50]) for _ in range(size)]
    n[rng.randrange(size)] = 9
    count = sum(n)
    minp = 1.0 / count
    pmf = [k / count if k else minp for k in n]
    mean = sum(i * k for i, k in enumerate(n)) / count
    return pmf, minp, mean


def make_samples(rng, n, lo, hi, max_count):
    vals = sorted(rng.sample(range(lo, hi), n))
    return vals, [rng.randrange(1, max_count + 1) for _ in vals]


def small_shapes():
    """[(name, pmf, minp, mean, jobs, values, counts, offsets)]: every PMF size of 1, 2, 63, 64, 65, 257, 1000 and every theta count
    of 1, 63, 64, 65, 257 (the first to need a second workgroup of 256) and 1025, with the corners named beside each job"""
    rng = random.Random(20261018)
    groups = []

    def group(name, size, specs):
        pmf, minp, mean = make_pmf(rng, size)
        jobs, values, counts, offsets = [], [], [], [0]
        for first, nth, len0, len1, (v, k) in specs:
            jobs.append((first, first + nth - 1, len0, len1))
            values += v
            counts += k
            offsets.append(len(values))
        groups.append((name, pmf, minp, mean, np.array(jobs, dtype=JOB), np.array(values, dtype=np.int32), np.array(counts, dtype=np.uint32),
                       np.array(offsets, dtype=np.uint64)))
    S = lambda n, lo, hi, mc=5: make_samples(rng, n, lo, hi, mc)  # noqa: E731
    group("pmf1000", 1000, [
        (-10, 1, 1, 1, S(1, 100, 900)),                    # one theta, x1 = 1, len0 == len1, one sample
        (-40, 65, 997, 2000, S(1, 100, 900)),              # an inexact quotient; one sample
        (-100, 257, 123457, 200000, S(300, 0, 1200, 100000)),  # x1 beyond the PMF: the flat top is never reached; 300 samples, large counts
    ])
    group("pmf257", 257, [
        (-600, 1025, 3, 5, S(40, 0, 500)),                 # x3 = 8 inside the theta range: the far side; x + theta < 0 for some samples
        (-5000, 64, 7, 7, S(20, 0, 400)),                  # x + theta < 0 for all
        (5000, 63, 7, 90, S(20, 0, 400)),                  # x + theta > maxValue for all
        (0, 0, 3, 3, S(3, 0, 10)),                         # an empty range
    ])
    group("pmf64", 64, [(-30, n, x1, x1 + d, S(5, 0, 80)) for n, x1, d in
                        ((1025, 7, 40), (257, 3, 0), (65, 997, 1), (64, 1, 0), (63, 123457, 5), (1, 7, 7))])
    for size in (1, 2, 63, 65):
        group("pmf%d" % size, size, [(-size - 3, n, x1, x1 + size, S(4, 0, size + 9)) for n, x1 in ((1, 3), (63, 1), (64, 7), (65, 997), (257, 123457))])
    group("mixed200", 63, [(rng.randrange(-90, 30), rng.randrange(0, 90), x1, x1 + rng.randrange(0, 50), S(rng.randrange(1, 12), 0, 90, 1000))
                           for x1 in (rng.choice([1, 3, 7, 997, 123457]) for _ in range(200))])
    return groups


def parse_dot(stdout, stderr):
    """{"a+ b-": (d, n)} of every estimate of a --dot -v -v run, printed or only warned about (those the estimator never saw, with
    d = INT_MIN, left out)"""
    out = {}
    for m in re.finditer(r'^"([^"]+)" -> "([^"]+)" \[d=(-?\d+) e=[0-9.]+ n=(\d+)\]$', stdout, re.M):
        out[m.group(1) + " " + m.group(2)] = (int(m.group(3)), int(m.group(4)))
    for m in re.finditer(r'^warning: "([^"]+)" -> "([^"]+)" \[d=(-?\d+)\] (\d+) of \d+ pairs', stderr, re.M):
        if int(m.group(3)) != -2 ** 31:
            out[m.group(1) + " " + m.group(2)] = (int(m.group(3)), int(m.group(4)))
    return out
