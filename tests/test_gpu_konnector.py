"""Konnector Bloom filters on the GPU (abg_kn.hip through api.KonnectorBloom and abyss_amd/bin/abyss-bloom) against the
reference's own outputs (tests/golden/konnector, made by tests/golden/make_konnector.py) and the host restatement
(tests/hostcheck/kn_check)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from abyss_amd import api, build, synth
from kn_golden import cases, golden, hash_vectors, workdir

pytestmark = pytest.mark.gpu


def abyss_bloom():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-bloom")


def kn_check():
    build.build_hostcheck()
    return build.KN_CHECK


def run(argv, cwd, timeout=300):
    return subprocess.run([abyss_bloom()] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


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
