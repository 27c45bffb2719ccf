"""abyss-map, abyss-index and api.FMIndex on the GPU against what the unmodified reference wrote (tests/golden/map) and against
tests/hostcheck/fm_check, which runs the same search bodies serially."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abyss_amd import _lib, api, build
import map_golden as mg
from test_map_host import expected_sam, stale_dir, stderr_lines, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bins():
    build.build_cli()
    return {p: os.path.join(build.BIN_DIR, p) for p in ("abyss-map", "abyss-index")}


@pytest.fixture(scope="module")
def fm_check():
    build.build_hostcheck()
    return build.FM_CHECK


@pytest.fixture(scope="module")
def fm():
    f = api.FMIndex()
    yield f
    f.close()


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def read_seqs(data):
    """the sequences of a two-line FASTA or four-line FASTQ file, case folded as FastaReader::FOLD_CASE does"""
    lines = data.split(b"\n")
    step = 4 if data[:1] == b"@" else 2
    return [lines[i + 1].upper() for i in range(0, len(lines) - 1, step)]


INDEXED = [c for c in mg.cases()["index"] if c["fm"] and c["argv"] == [c["target"]]] + \
    [c for c in mg.cases()["index"] if c["name"] == "numeric_s1"]


@pytest.mark.parametrize("case", INDEXED, ids=lambda c: c["name"])
def test_export_equals_the_reference_index(case, fm):
    """SA (at the file's sample period) and the whole BWT, decoded from the reference's .fm"""
    text = mg.input_bytes(case["target"])
    fm.build(text)
    assert fm.size() == len(text)
    sa, bwt = fm.export()
    period, want_sa, want_bwt = mg.parse_fm(mg.golden(case["fm"]))
    assert sa[0] == len(text) and np.array_equal(np.sort(sa), np.arange(len(text) + 1, dtype=np.uint32))
    assert np.array_equal(sa[::period].astype(np.uint64), want_sa)
    assert np.array_equal(bwt, want_bwt)


@pytest.mark.parametrize("case", mg.cases()["index"], ids=lambda c: c["name"])
def test_index_files_equal_the_reference(case, bins, tmp_path):
    write_inputs(tmp_path, [case["target"]])
    r = run([bins["abyss-index"]] + case["argv"], tmp_path)
    assert r.returncode == 0, r.stderr
    for ext in ("fm", "fai"):
        p = tmp_path / (case["target"] + "." + ext)
        if case.get(ext + "_sha256") is None:
            assert not p.exists()
            continue
        got = p.read_bytes()
        assert mg.sha256(got) == case[ext + "_sha256"], ext
        if case[ext]:
            assert got == mg.golden(case[ext])


@pytest.mark.parametrize("case", mg.cases()["map"], ids=lambda c: c["name"])
def test_sam_equals_the_reference(case, bins, tmp_path):
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    r = run([bins["abyss-map"]] + case["argv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_sam(case, [bins["abyss-map"]])
    assert stderr_lines(r.stderr.decode()) == stderr_lines(case["stderr"])  # (with -v: the counters)


def test_sam_in_small_blocks_and_on_many_threads(bins, tmp_path, monkeypatch):
    """blocks of 7 reads (the next one parsed while one is mapped) and -j16 formatting: the same bytes"""
    case = next(c for c in mg.cases()["map"] if c["name"] == "letters_l30_ss")
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    monkeypatch.setenv("ABG_MAP_BLOCK_READS", "7")
    argv = ["-j16"] + case["argv"][1:]
    r = run([bins["abyss-map"]] + argv, tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_sam(dict(case, argv=argv), [bins["abyss-map"]])
    assert stderr_lines(r.stderr.decode()) == stderr_lines(case["stderr"])


def test_sam_with_index_files_present_and_stale(bins, tmp_path):
    case = next(c for c in mg.cases()["map"] if c["name"] == "numeric_l1_ss")
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    for ext in (".fm", ".fai"):
        (tmp_path / (case["target"] + ext)).write_bytes(mg.golden(case["target"] + ext))
    r = run([bins["abyss-map"]] + case["argv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_sam(case, [bins["abyss-map"]])
    assert "Building" not in r.stderr.decode()
    for stale in (c for c in mg.cases()["errors"] if c["stale"]):
        d = tmp_path / stale["name"]
        d.mkdir()
        stale_dir(stale, d)
        r = run([bins["abyss-map"]] + stale["argv"], d)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == stale["stderr"]


RAW = [("letters.fa", "reads1.fa", 30, False, True), ("letters.fa", "reads2.fq", 30, True, True), ("letters.fa", "reads1.fa", 2000, False, True),
       ("numeric.fa", "nreads1.fa", 1, False, True), ("numeric.fa", "nreads2.fq", 5, False, False), ("numeric.fa", "nreads1.fa", 0, True, True),
       ("edge128.fa", "nreads1.fa", 3, False, True), ("no_t.fa", "treads.fa", 20, False, True),
       # the table build at the block edges: reads of the targets themselves, so that ranks in the first and last block decide matches
       # (a text of 127 bytes has 128 rows and a last block without a symbol); the SAM cases on the same files tie them to the reference
       ("edge127.fa", "ereads127.fa", 5, False, True), ("edge128.fa", "ereads128.fa", 8, True, True), ("edge129.fa", "ereads129.fa", 6, False, False)]


@pytest.mark.parametrize("target,reads,k,ss,rc", RAW, ids=lambda v: str(v))
def test_raw_matches_equal_the_serial_bodies(target, reads, k, ss, rc, fm, fm_check, tmp_path):
    """both strands' (l, u, qstart, qend, num) and SA[l], reads of 1 to 3000 bases in one call"""
    write_inputs(tmp_path, [target, reads])
    flags = (0 if rc else 1) | (2 if ss else 0)
    r = run([fm_check, "hits", str(k), str(flags), target, reads], tmp_path)
    assert r.returncode == 0, r.stderr
    want = np.array([[int(x) for x in ln.split()] for ln in r.stdout.decode().splitlines()], dtype=np.uint32).reshape(-1, 2, 6)
    seqs = read_seqs(mg.golden(reads))
    assert len(seqs) == len(want)
    fm.build(mg.golden(target))
    buf, off = api.concat_seqs(seqs)
    got = fm.map(buf, off, k, ss=ss, rc=rc)
    for j, name in enumerate(api.FM_HIT.names):
        assert np.array_equal(got[name], want[:, :, j]), name


def test_one_call_of_many_reads_equals_its_blocks(fm):
    """50,000 reads against the 2 Mbp target: one call (the ticket runs far past the lanes) against five calls of 10,000, and the
    perfect reads against where they were cut"""
    fm.build(mg.big_target())
    seqs = read_seqs(mg.big_reads(50000, 150))
    buf, off = api.concat_seqs(seqs)
    whole = fm.map(buf, off, 30)
    parts = []
    for a in range(0, 50000, 10000):
        b, o = api.concat_seqs(seqs[a:a + 10000])
        parts.append(fm.map(b, o, 30))
    assert np.array_equal(whole, np.concatenate(parts))
    span = whole["qend"].astype(np.int64) - whole["qstart"]
    best = span.max(axis=1)
    clean = np.array([j % 7 != 3 and j % 31 != 5 for j in range(50000)])
    assert (best[clean] == 150).all() and (best[~clean] < 150).all() and (best >= 75).all()
    text = mg.big_target()
    for j in range(0, 50000, 997):  # the located text is the read (forward reads on the forward strand)
        h = whole[j, 0] if span[j, 0] >= span[j, 1] else whole[j, 1]
        s = seqs[j] if span[j, 0] >= span[j, 1] else mg.revcomp(seqs[j])
        assert text[int(h["pos"]):int(h["pos"]) + int(h["qend"] - h["qstart"])] == s[int(h["qstart"]):int(h["qend"])]


def test_the_wave_count_changes_no_match(fm):
    """abg_fm_tune: one and two waves a CU (fewer lanes than the 50,000 reads, so the ticket hands out the rest) and thirty-two (as
    many lanes as reads, the memo re-sized) give the default's matches"""
    fm.build(mg.big_target())
    buf, off = api.concat_seqs(read_seqs(mg.big_reads(50000, 150)))
    want = fm.map(buf, off, 30)
    try:
        for waves in (1, 2, 32):
            fm.tune(waves)
            assert np.array_equal(fm.map(buf, off, 30), want), waves
    finally:
        fm.tune(0)


def test_refused_sizes_and_calls(fm):
    with pytest.raises(api.AbyssAmdError):
        fm.build(b"")
    # 2^32 - 1 bytes or more: refused on the size alone, before a byte is read (so four bytes stand in for the text); the index
    # that was there stays
    fm.build(b">0\nACGT\n")
    small = C.create_string_buffer(b"ACGT")
    for n in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
        assert fm._lib.abg_fm_build(fm._h, C.cast(small, C.c_void_p), n) == _lib.ABG_EINVAL
        assert b"smaller than 4294967295 bytes" in fm._lib.abg_fm_last_error(fm._h)
    assert fm.size() == 8
    with pytest.raises(api.AbyssAmdError):
        fm.tune(33)
    f = api.FMIndex()
    with pytest.raises(api.AbyssAmdError) as e:
        f.map(b"ACGT", np.array([0, 4]), 1)
    assert "no index" in str(e.value)
    f.close()
    fm.build(b">0\nACGT\n")
    assert fm.map(b"", np.array([0]), 1).shape == (0, 2)
    empty = fm.map(b"ACGT", np.array([0, 0, 4]), 1)  # an empty sequence: the start value, no match
    assert empty[0, 0]["l"] == empty[0, 0]["u"] == 0 and empty[1, 0]["qend"] - empty[1, 0]["qstart"] == 4
    fm.profile(True)
    fm.build(mg.golden("numeric.fa"))
    assert fm.profile_get("fm_sa")[1] == 1 and fm.profile_get("fm_occ")[1] == 1
    fm.profile(False)
