"""Konnector Bloom filters on the host (no GPU): the ABG_HD logic of abyss_amd/csrc/abg_kn.h (packing, canonical choice,
CityHash64WithSeed) against known-answer vectors of the reference's own Kmer + city.cc, and the file commands of
`abyss-bloom` (union, intersect, info, compare: host-side streaming that never starts the HIP runtime) against the
reference's outputs (tests/golden/konnector, made by tests/golden/make_konnector.py)."""
import hashlib
import os
import subprocess

import pytest

from abyss_amd import build
import kn_large
from kn_golden import cases, golden, hash_vectors, large, workdir


def abyss_bloom():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "abyss-bloom")


def kn_check():
    build.build_hostcheck()
    return build.KN_CHECK


def test_hash_vectors_host():
    vec = hash_vectors()
    lines = "".join("%d %s %s\n" % (v["k"], v["seed"], v["seq"]) for v in vec)
    out = subprocess.run([kn_check(), "hash"], input=lines, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(out) == len(vec)
    for v, line in zip(vec, out):
        want = ["-" if h is None else h for h in v["hash"]]
        assert line.split() == want, (v["k"], v["seed"], v["seq"])


@pytest.mark.parametrize("name", [c["name"] for c in cases()["commands"]])
def test_file_command_matches_reference(tmp_path, name):
    c = next(c for c in cases()["commands"] if c["name"] == name)
    wd = workdir(tmp_path)
    r = subprocess.run([abyss_bloom()] + c["argv"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == c["status"], r.stderr
    assert r.stdout.decode() == c["stdout"]
    assert r.stderr.decode() == c["stderr"]
    if c["output"]:
        assert open(os.path.join(wd, c["output"]), "rb").read() == golden(c["output"])


def _data(path):
    raw = open(path, "rb").read()
    i = 0
    for _ in range(4):
        i = raw.index(b"\n", i) + 1
    head = raw[:i].split(b"\n")
    full, start, end = (int(x) for x in head[2].split(b"\t"))
    return full, start, end, raw[i:]


def test_compare_counts_exact_bytes_on_odd_sizes(tmp_path):
    """A size that is not a multiple of 262,144 bits (21,338, the -l3 case): the four counts cover exactly ceil(bits / 8)
    bytes, and 1/1 is the popcount of the AND (the reference would count stale buffer bytes here)."""
    wd = workdir(tmp_path)
    # a second filter of the same size: the odd filter ANDed with a shifted copy of itself
    full, start, end, a = _data(os.path.join(wd, "k25_l3_odd.bloom"))
    b = bytes(a[(i + 1) % len(a)] for i in range(len(a)))
    header = open(os.path.join(wd, "k25_l3_odd.bloom"), "rb").read()[:-len(a)]
    open(os.path.join(wd, "other.bloom"), "wb").write(header + b)
    r = subprocess.run([abyss_bloom(), "compare", "-k25", "k25_l3_odd.bloom", "other.bloom"], cwd=wd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1
    counts = dict(line.split(": ") for line in r.stdout.splitlines())
    n11, n10, n01, n00 = (int(counts[x]) for x in ("1/1", "1/0", "0/1", "0/0"))
    nbytes = (end - start + 1 + 7) // 8
    assert n11 + n10 + n01 + n00 == 8 * nbytes
    assert n11 == sum(bin(x & y).count("1") for x, y in zip(a, b))
    assert n10 == sum(bin(x & ~y & 0xFF).count("1") for x, y in zip(a, b))
    assert "Jaccard similarity: " in r.stdout


def test_graph_and_trim_are_refused(tmp_path):
    for cmd in ("graph", "trim"):
        r = subprocess.run([abyss_bloom(), cmd, "-k25", "x.bloom"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 1 and "not provided by this build" in r.stderr
    r = subprocess.run([abyss_bloom(), "frobnicate"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "unrecognized command" in r.stderr


def test_build_checks_its_options_before_any_device_work(tmp_path):
    """The reference's option errors for -t konnector come before the HIP runtime is touched."""
    wd = workdir(tmp_path)
    r = subprocess.run([abyss_bloom(), "build", "-k25", "-b32K", "-L", "1=k25_l1.bloom", "o.bloom", "reads.fa"], cwd=wd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "-L can only be used with cascading bloom filters (-l >= 2)" in r.stderr
    r = subprocess.run([abyss_bloom(), "build", "-k25", "-b1001", "-l2", "-w", "1/3", "o.bloom", "reads.fa"], cwd=wd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "(b / l) % w == 0 must be true" in r.stderr
    r = subprocess.run([abyss_bloom(), "build", "-k25", "-t", "bogus", "o.bloom", "reads.fa"], cwd=wd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "unrecognized argument to `-t'" in r.stderr


def test_host_restatement_builds_the_reference_files(tmp_path):
    """kn_check fills the cascade one k-mer at a time: the plain, cascading and window cases byte-equal to the reference."""
    wd = workdir(tmp_path)
    for name, k, seed, levels, bits, start, end, reads in [
            ("k25_l1", 25, 0, 1, 262144, 0, 262143, ["reads.fa"]),
            ("k25_l2", 25, 0, 2, 262144, 0, 262143, ["reads.fa"]),
            ("k25_w3", 25, 0, 1, 262144, 131072, 196607, ["reads.fa"]),
            ("k96_l2", 96, 0, 2, 262144, 0, 262143, ["reads.fa"]),
            ("k150_l1", 150, 0, 1, 262144, 0, 262143, ["reads.fa", "reads.fq"])]:
        out = os.path.join(wd, "h_%s.bloom" % name)
        subprocess.run([kn_check(), "build", str(k), str(seed), str(levels), str(bits), str(start), str(end), out] + reads,
                       cwd=wd, check=True)
        assert open(out, "rb").read() == golden(name + ".bloom"), name


def test_large_inputs_regenerate(tmp_path):
    """The large GPU cases regenerate long.fa (tests/kn_large.py) on the machine that runs them: its bytes must still be the ones
    the reference ran on (large.json), and the archive's reads too."""
    inputs = large()["inputs"]
    assert set(inputs) == {"reads.fa", "reads.fq", "long.fa"}
    for name in ("reads.fa", "reads.fq"):
        data = golden(name)
        assert (hashlib.sha256(data).hexdigest(), len(data)) == (inputs[name]["sha256"], inputs[name]["bytes"]), name
    path = str(tmp_path / "long.fa")
    got = kn_large.write_long_fasta(path, golden("reads.fa"))
    assert got == (inputs["long.fa"]["sha256"], inputs["long.fa"]["bytes"])
    assert kn_large.sha256_file(path) == got
    with open(path, "rb") as f:
        head = f.read(8)
    assert head == b">long0\n" + head[7:8] and head[7:8] in b"ACGTN"
    assert got[1] == sum(kn_large.LONG_LENGTHS) + 2 * (len(">long0") + 2)
