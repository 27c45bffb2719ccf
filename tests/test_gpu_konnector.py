"""Konnector Bloom filters on the GPU (abg_kn.hip through api.KonnectorBloom and abyss_amd/bin/abyss-bloom) against the
reference's own outputs (tests/golden/konnector, made by tests/golden/make_konnector.py: cases.json and, for filters past 2^32
bits and records longer than a staging slot, large.json), the host restatement (tests/hostcheck/kn_check) and plain Python
restatements of the index and the cascade."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from abyss_amd import api, build, synth
import kn_large
from kn_golden import cases, filter_header, golden, hash_vectors, large, workdir

pytestmark = pytest.mark.gpu


def abyss_bloom():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-bloom")


def kn_check():
    build.build_hostcheck()
    return build.KN_CHECK


def run(argv, cwd, timeout=300, env=None):
    return subprocess.run([abyss_bloom()] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                          env=None if env is None else dict(os.environ, **env))


def test_hash_seq_known_answers():
    vec = hash_vectors()
    bits = 1000003
    filters = {}
    try:
        for v in vec:
            key = (v["k"], int(v["seed"]))
            if key not in filters:
                filters[key] = api.KonnectorBloom(v["k"], bits, seed=int(v["seed"]))
            h, i, ok = filters[key].hash_seq(v["seq"].encode())
            want = v["hash"]
            assert [bool(x) for x in ok] == [w is not None for w in want], key
            assert [int(x) for x, w in zip(h, want) if w is not None] == [int(w) for w in want if w is not None], key
            assert [int(x) for x, w in zip(i, want) if w is not None] == [int(w) % bits for w in want if w is not None], key
    finally:
        for f in filters.values():
            f.close()


@pytest.mark.parametrize("name", [c["name"] for c in cases()["build"]])
def test_build_matches_reference(tmp_path, name):
    c = next(c for c in cases()["build"] if c["name"] == name)
    wd = workdir(tmp_path)
    i = next(j for j, a in enumerate(c["args"]) if a.startswith("reads."))
    out = "gpu_%s.bloom" % name
    r = run(["build"] + c["args"][:i] + [out] + c["args"][i:], wd)
    assert r.returncode == c["status"], r.stderr
    assert r.stderr.decode() == c["stderr"]
    assert open(os.path.join(wd, out), "rb").read() == golden(name + ".bloom")


@pytest.mark.parametrize("name", [c["name"] for c in cases()["kmers"]])
def test_kmers_match_reference(tmp_path, name):
    c = next(c for c in cases()["kmers"] if c["name"] == name)
    r = run(c["argv"], workdir(tmp_path))
    assert r.returncode == c["status"], r.stderr
    assert r.stdout.count(b"\n") == c["lines"]
    assert hashlib.sha256(r.stdout).hexdigest() == c["sha256"]


@pytest.fixture(scope="module")
def synth_reads(tmp_path_factory):
    """400 k pairs of 150 bp (120 M bases: several upload chunks of the binary and of the library)."""
    d = tmp_path_factory.mktemp("kn_synth")
    m1, m2 = synth.make_read_set(600000, 200.0)
    assert len(m1) == 400000
    synth.write_fastq(str(d / "r1.fq"), m1, "r", 1)
    synth.write_fastq(str(d / "r2.fq"), m2, "r", 2)
    return str(d)


def test_synth_threads_agree_with_the_serial_restatement(synth_reads):
    wd = synth_reads
    outs = []
    for j in (1, 16):
        r = run(["build", "-k64", "-b8M", "-l2", "-j%d" % j, "j%d.bloom" % j, "r1.fq", "r2.fq"], wd, timeout=600)
        assert r.returncode == 0, r.stderr
        outs.append(open(os.path.join(wd, "j%d.bloom" % j), "rb").read())
    assert outs[0] == outs[1]
    bits = 8 * 8 * (1 << 20) // 2
    subprocess.run([kn_check(), "build", "64", "0", "2", str(bits), "0", str(bits - 1), "host.bloom", "r1.fq", "r2.fq"],
                   cwd=wd, check=True, timeout=900)
    assert open(os.path.join(wd, "host.bloom"), "rb").read() == outs[0]


def test_union_of_gpu_windows_is_the_plain_filter(tmp_path):
    wd = workdir(tmp_path)
    for w in range(1, 5):
        r = run(["build", "-k32", "-b128K", "-l2", "-h3", "-w", "%d/4" % w, "w%d.bloom" % w, "reads.fa", "reads.fq"], wd)
        assert r.returncode == 0, r.stderr
    r = run(["build", "-k32", "-b128K", "-l2", "-h3", "plain.bloom", "reads.fa", "reads.fq"], wd)
    assert r.returncode == 0, r.stderr
    r = run(["union", "-k32", "u.bloom", "w1.bloom", "w2.bloom", "w3.bloom", "w4.bloom"], wd)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(wd, "u.bloom"), "rb").read() == open(os.path.join(wd, "plain.bloom"), "rb").read()


@pytest.mark.parametrize("fmt,inverse", [("fasta", False), ("bed", True), ("raw", False), ("raw", True)])
def test_prebuilt_filter_kmers_match_the_restatement(tmp_path, fmt, inverse):
    wd = workdir(tmp_path)
    r = run(["build", "-k40", "-b24K", "-l2", "-h11", "pre.bloom", "reads.fq"], wd)
    assert r.returncode == 0, r.stderr
    argv = ["kmers", "-k40", "--" + fmt] + (["-r"] if inverse else []) + ["pre.bloom", "reads.fa"]
    got = run(argv, wd)
    assert got.returncode == 0, got.stderr
    want = subprocess.run([kn_check(), "kmers", "40", "pre.bloom", "reads.fa", fmt] + (["inverse"] if inverse else []), cwd=wd,
                          stdout=subprocess.PIPE, check=True).stdout
    assert len(want) > 0
    assert got.stdout == want


def test_api_cascade_and_popcount():
    """KonnectorBloom: the levels of a cascade from the API equal the host restatement's, popcount included."""
    buf = golden("reads.fa")
    seqs = [l for l in buf.split(b"\n") if l and not l.startswith(b">")]
    b, off = api.concat_seqs(seqs)
    f = api.KonnectorBloom(25, 50000, levels=3, seed=5)
    try:
        f.load(b, off)
        pops = f.popcount()
        lv = [f.level(i) for i in range(3)]
        assert pops == [int(np.unpackbits(x).sum()) for x in lv]
        assert pops[0] > pops[1] > pops[2] > 0
        flags = f.contains(b, off)
        assert flags.sum() > 0
    finally:
        f.close()


# ---- the index space: mod64 on the device for every kind of filter size ---------------------------------------------------

MOD_BITS = [3, 64, 1000003, (1 << 32) - 1, 1 << 32, (1 << 32) + 15, 5726623061, 1 << 33, 38177487104, 1 << 40, (1 << 63) + 12345,
            (1 << 64) - 59]


def test_hash_seq_index_for_every_filter_size(monkeypatch):
    """index = hash % bits on the device (abg::mod64: a mask for powers of two, a multiply-high otherwise) for sizes past 2^32
    and up to 2^64 - 59, against Python's integers.  A window of at most 4096 bits keeps each filter tiny."""
    monkeypatch.setenv("ABG_KN_SLOT_BYTES", "65536")
    by_key = {}
    for v in hash_vectors():
        by_key.setdefault((v["k"], int(v["seed"])), []).append(v)
    for bits in MOD_BITS:
        for (k, seed), vs in sorted(by_key.items()):
            f = api.KonnectorBloom(k, bits, seed=seed, start=0, end=min(bits - 1, 4095))
            try:
                for v in vs:
                    h, i, ok = f.hash_seq(v["seq"].encode())
                    want = [int(w) for w in v["hash"] if w is not None]
                    assert [int(x) for x in h[ok]] == want, (bits, k, seed)
                    assert [int(x) for x in i[ok]] == [w % bits for w in want], (bits, k, seed)
            finally:
                f.close()


# ---- bit placement at high offsets: a window past 2^32 of a 5,726,623,061-bit cascade --------------------------------------

def restated_levels(hashes, bits, start, end, levels):
    """CascadingBloomFilterWindow::insert, restated: index = hash % bits; inside [start, end] local bit i sets byte i // 8,
    bit 7 - i % 8 of the first level where it is clear.  Returns {byte: value} for each level."""
    have = [set() for _ in range(levels)]
    for h in hashes:
        idx = h % bits
        if start <= idx <= end:
            for lv in have:
                if idx - start not in lv:
                    lv.add(idx - start)
                    break
    out = []
    for lv in have:
        d = {}
        for i in lv:
            d[i // 8] = d.get(i // 8, 0) | (1 << (7 - i % 8))
        out.append(d)
    return out


@pytest.mark.parametrize("k,seed_i", [(5, 0), (33, 1), (96, 2), (128, 0), (150, 1), (192, 2)])
def test_bit_placement_past_2_32(k, seed_i):
    bits, levels = 5726623061, 3
    start, end = bits - (1 << 31), bits - 1
    vec = hash_vectors()
    seed = int(sorted({v["seed"] for v in vec}, key=int)[seed_i])
    vs = [v for v in vec if v["k"] == k and int(v["seed"]) == seed]
    assert len(vs) == 5
    seqs = [v["seq"].encode() for v in vs] + [vs[0]["seq"].encode()]  # the first twice: its windows reach level 2
    hashes = [int(w) for v in vs + [vs[0]] for w in v["hash"] if w is not None]
    want = restated_levels(hashes, bits, start, end, levels)
    assert want[0] and want[1] and sum(len(w) for w in want) > 0
    b, off = api.concat_seqs(seqs)
    f = api.KonnectorBloom(k, bits, levels=levels, seed=seed, start=start, end=end)
    try:
        f.load(b, off)
        for lv in range(levels):
            got = f.level(lv)
            assert got.size == (1 << 28)
            nz = np.flatnonzero(got)
            assert [int(x) for x in nz] == sorted(want[lv]), lv
            assert [int(got[x]) for x in nz] == [want[lv][x] for x in sorted(want[lv])], lv
        assert f.popcount() == [sum(bin(x).count("1") for x in w.values()) for w in want]
        flags = f.contains(b, off)
        at = 0
        for v in vs + [vs[0]]:  # level 0 holds exactly the in-window indices of the windows loaded
            exp = [w is not None and start <= int(w) % bits <= end for w in v["hash"]]
            assert [bool(x) for x in flags[at:at + len(exp)]] == exp
            assert not flags[at + len(exp):at + len(v["seq"])].any()
            at += len(v["seq"])
    finally:
        f.close()


# ---- large cases: digests of the reference's outputs (tests/golden/konnector/large.json) -----------------------------------

@pytest.fixture(scope="module")
def large_dir(tmp_path_factory):
    """reads.fa, reads.fq and long.fa (tests/kn_large.py), each checked against large.json's digest."""
    d = str(tmp_path_factory.mktemp("kn_large"))
    inputs = large()["inputs"]
    for name in ("reads.fa", "reads.fq"):
        open(os.path.join(d, name), "wb").write(golden(name))
    kn_large.write_long_fasta(os.path.join(d, "long.fa"), golden("reads.fa"))
    for name, want in inputs.items():
        assert kn_large.sha256_file(os.path.join(d, name)) == (want["sha256"], want["bytes"]), name
    return d


def check_stream(got, want):
    if "text" in want:
        assert got.decode() == want["text"]
    else:
        assert (hashlib.sha256(got).hexdigest(), len(got), got.count(b"\n")) == (want["sha256"], want["bytes"], want["lines"])


def large_params():
    out = []
    for c in large()["cases"]:
        out.append(pytest.param(c["name"], None, id=c["name"]))
        if any(a == "long.fa" for a in c["argv"]):  # the long records again through 64 KiB slots: ~2,300 pieces
            out.append(pytest.param(c["name"], "65536", id=c["name"] + "-slot64K"))
    return out


@pytest.mark.parametrize("name,slot", large_params())
def test_large_case_digests(large_dir, name, slot):
    by_name = {c["name"]: c for c in large()["cases"]}
    c = by_name[name]
    env = {} if slot is None else {"ABG_KN_SLOT_BYTES": slot}
    made = []
    try:
        for n in c["needs"]:
            r = run(by_name[n]["argv"], large_dir, env=env)
            assert r.returncode == 0, r.stderr
            made += list(by_name[n]["outputs"])
        made += list(c["outputs"])
        r = run(c["argv"], large_dir, env=env)
        assert r.returncode == c["status"], r.stderr
        check_stream(r.stdout, c["stdout"])
        check_stream(r.stderr, c["stderr"])
        for out, want in c["outputs"].items():
            got = kn_large.sha256_file(os.path.join(large_dir, out))
            os.remove(os.path.join(large_dir, out))
            assert got == (want["sha256"], want["bytes"]), out
    finally:
        for out in made:
            if os.path.exists(os.path.join(large_dir, out)):
                os.remove(os.path.join(large_dir, out))


# ---- slot-size invariance: staging slots of 1, 4 and 64 KiB give the reference's bytes ---------------------------------------

SLOTS = ["1024", "4096", "65536"]


@pytest.mark.parametrize("slot", SLOTS)
def test_small_slots_build_goldens(tmp_path, slot):
    wd = workdir(tmp_path)
    for c in cases()["build"]:
        i = next(j for j, a in enumerate(c["args"]) if a.startswith("reads."))
        out = "slot_%s.bloom" % c["name"]
        r = run(["build"] + c["args"][:i] + [out] + c["args"][i:], wd, env={"ABG_KN_SLOT_BYTES": slot})
        assert r.returncode == c["status"], (c["name"], r.stderr)
        assert r.stderr.decode() == c["stderr"], c["name"]
        assert open(os.path.join(wd, out), "rb").read() == golden(c["name"] + ".bloom"), c["name"]


@pytest.mark.parametrize("slot", SLOTS)
@pytest.mark.parametrize("name", ["kmers_bed", "kmers_k192_bed_r"])
def test_small_slots_kmers_goldens(tmp_path, slot, name):
    c = next(c for c in cases()["kmers"] if c["name"] == name)
    r = run(c["argv"], workdir(tmp_path), env={"ABG_KN_SLOT_BYTES": slot})
    assert r.returncode == c["status"], r.stderr
    assert r.stdout.count(b"\n") == c["lines"]
    assert hashlib.sha256(r.stdout).hexdigest() == c["sha256"]


def joined_reads(per):
    """reads.fa's records as the reader hands them over (masked, lower-case ends trimmed: FastaReader trimMasked) joined by
    'N' into sequences of `per` records: the same windows as the records, in sequences longer than a small slot (so they are
    cut into pieces)."""
    recs = [re.sub(rb"^[a-z]+|[a-z]+$", b"", r) for r in kn_large.fasta_records(golden("reads.fa"))]
    return api.concat_seqs([b"N".join(recs[i:i + per]) for i in range(0, len(recs), per)])


# build goldens of reads.fa alone without -w, -L or -q: the API restates them from the joined records
API_BUILDS = ["k25_l2", "k25_l3_odd", "k64_l1_hbig", "k96_l2", "k12_l2", "k31_l3_odd", "k97_l2_odd", "k160_l2", "k161_l3_odd",
              "k192_l2"]


@pytest.mark.parametrize("slot", SLOTS)
def test_small_slots_api_load_and_contains(monkeypatch, slot):
    monkeypatch.setenv("ABG_KN_SLOT_BYTES", slot)
    b, off = joined_reads(1000)
    assert int(np.diff(off).min()) > 100000
    for name in API_BUILDS:
        c = next(c for c in cases()["build"] if c["name"] == name)
        (k, bits, start, end, seed), want = filter_header(golden(name + ".bloom"))
        levels = next((int(a[2:]) for a in c["args"] if a.startswith("-l")), 1)
        f = api.KonnectorBloom(k, bits, levels=levels, seed=seed, start=start, end=end)
        try:
            f.load(b, off)
            assert f.level(levels - 1).tobytes() == want, name
            assert f.popcount() == [int(x) for x in re.findall(r"Bloom popcount \(bits\): (\d+)", c["stderr"])], name
        finally:
            f.close()
    # a filter of reads.fa holds every window of them: the flags are exactly the all-ACGT windows, in the caller's positions
    for name in ("k25_l1", "k64_l1_hbig"):
        (k, bits, start, end, seed), data = filter_header(golden(name + ".bloom"))
        f = api.KonnectorBloom(k, bits, seed=seed, start=start, end=end)
        try:
            f.set_level(0, np.frombuffer(data, dtype=np.uint8))
            flags = f.contains(b, off)
            acgt = np.isin(np.frombuffer(b, dtype=np.uint8), np.frombuffer(b"ACGTacgt", dtype=np.uint8))
            want = np.zeros(len(b), dtype=bool)
            for s, e in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
                full = np.convolve(acgt[s:e], np.ones(k, dtype=np.int64), mode="valid") == k
                want[s:s + len(full)] = full
            assert want.sum() > 100000
            assert np.array_equal(flags.astype(bool), want), name
            assert not f.contains(b, off, inverse=True).any(), name
        finally:
            f.close()
