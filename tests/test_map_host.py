"""abyss-map and abyss-index without a GPU: tests/hostcheck/fm_check runs the serial bodies of abyss_amd/csrc/abg_fm.h (table, search,
locate) over a host-sorted suffix array and prints through map_core.h; every byte is compared with what the unmodified reference
wrote (tests/golden/map, tests/golden/make_map.py).  The binaries' option and argument errors come before any device work."""
import os
import re
import subprocess

import pytest

from abyss_amd import api, build
import map_golden as mg


@pytest.fixture(scope="module")
def fm_check():
    build.build_hostcheck()
    return build.FM_CHECK


@pytest.fixture(scope="module")
def bins():
    build.build_cli()
    return {p: os.path.join(build.BIN_DIR, p) for p in ("abyss-map", "abyss-index")}


def write_inputs(d, names):
    for name in names:
        with open(os.path.join(str(d), name), "wb") as f:
            f.write(mg.input_bytes(name))


def expected_sam(case, argv0):
    """the golden SAM with its CL: the command actually run"""
    lines = mg.golden(case["sam"]).split(b"\n")
    assert lines[1].startswith(b"@PG\t") and b"\tCL:" in lines[1]
    lines[1] = lines[1][:lines[1].index(b"\tCL:") + 4] + " ".join(argv0 + case["argv"]).encode()
    return b"\n".join(lines)


def stderr_lines(text):
    """without the reference's memory figures, which the drop-in leaves out; the percentages to three digits: the reference prints
    them with setprecision(3) only where its memory line came before them, which depends on how much memory it took"""
    return [re.sub(r"\(([0-9.]+)%\)", lambda m: "(%.3g%%)" % float(m.group(1)), ln) for ln in text.splitlines() if not ln.startswith("Using ")]


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


@pytest.mark.parametrize("case", mg.cases()["index"], ids=lambda c: c["name"])
def test_index_files_equal_the_reference(case, fm_check, tmp_path):
    write_inputs(tmp_path, [case["target"]])
    r = run([fm_check, "index"] + case["argv"], tmp_path)
    assert r.returncode == case["status"], r.stderr
    for ext in ("fm", "fai"):
        p = tmp_path / (case["target"] + "." + ext)
        if case.get(ext + "_sha256") is None:
            assert not p.exists()
            continue
        got = p.read_bytes()
        assert mg.sha256(got) == case[ext + "_sha256"], ext
        if case[ext]:
            assert got == mg.golden(case[ext])
    want = [ln for ln in stderr_lines(case["stderr"]) if not ln.startswith("Read ") or "contigs" in ln]
    assert [ln for ln in r.stderr.decode().splitlines() if not ln.startswith("Read ") or "contigs" in ln] == want


@pytest.mark.parametrize("case", mg.cases()["map"], ids=lambda c: c["name"])
def test_sam_equals_the_reference(case, fm_check, tmp_path):
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    r = run([fm_check, "map"] + case["argv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_sam(case, ["abyss-map"])
    assert stderr_lines(r.stderr.decode()) == stderr_lines(case["stderr"])


def test_sam_in_small_blocks_and_on_many_threads(fm_check, tmp_path, monkeypatch):
    """blocks of 7 reads (the next one parsed while one is mapped) and -j16 formatting: the same bytes"""
    case = next(c for c in mg.cases()["map"] if c["name"] == "letters_l30_ss")
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    argv = ["-j16"] + case["argv"][1:]
    for block in ("7", "80"):
        monkeypatch.setenv("ABG_MAP_BLOCK_READS", block)
        r = run([fm_check, "map"] + argv, tmp_path)
        assert r.returncode == 0, r.stderr
        assert r.stdout == expected_sam(dict(case, argv=argv), ["abyss-map"])
        assert stderr_lines(r.stderr.decode()) == stderr_lines(case["stderr"])


def test_sam_with_index_files_present(fm_check, tmp_path):
    case = next(c for c in mg.cases()["map"] if c["name"] == "numeric_l1_ss")
    write_inputs(tmp_path, [case["target"]] + case["queries"])
    for ext in (".fm", ".fai"):
        (tmp_path / (case["target"] + ext)).write_bytes(mg.golden(case["target"] + ext))
    r = run([fm_check, "map"] + case["argv"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_sam(case, ["abyss-map"])
    err = r.stderr.decode()
    assert "Building" not in err and "Reading `numeric.fa.fm'..." in err and "Reading `numeric.fa.fai'..." in err
    want = [ln for ln in stderr_lines(case["stderr"]) if ln.startswith(("Mapped", "Made", "Read "))]
    assert [ln for ln in stderr_lines(err) if ln.startswith(("Mapped", "Made", "Read "))] == want


def stale_dir(case, d):
    write_inputs(d, ["numeric.fa", "nreads1.fa"])
    fm, fai = mg.golden("numeric.fa.fm"), mg.golden("numeric.fa.fai")
    if case["stale"] == "fm":
        fm = mg.golden("no_t.fa.fm")
    elif case["stale"] == "fai":
        fai = mg.golden("no_t.fa.fai")
    else:
        fm = fm.replace(b"FM 64 1", b"FM 32 1", 1)
    (d / "numeric.fa.fm").write_bytes(fm)
    (d / "numeric.fa.fai").write_bytes(fai)


@pytest.mark.parametrize("case", [c for c in mg.cases()["errors"] if c["stale"]], ids=lambda c: c["name"])
def test_stale_index_files_are_reported(case, fm_check, bins, tmp_path):
    """the version check and the two staleness checks: the reference's message and status, from fm_check and from the binary (which
    makes them before it asks for a device)"""
    stale_dir(case, tmp_path)
    for cmd in ([fm_check, "map"], [bins["abyss-map"]]):
        r = run(cmd + case["argv"], tmp_path)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode() == case["stderr"]


@pytest.mark.parametrize("case", [c for c in mg.cases()["errors"] if not c["stale"] and c["name"] != "id_at"], ids=lambda c: c["name"])
def test_argument_errors_equal_the_reference(case, bins, tmp_path):
    r = run([bins[case["prog"]]] + case["argv"], tmp_path)
    assert (r.returncode, r.stdout.decode()) == (case["status"], case["stdout"])
    assert r.stderr.decode().replace(bins[case["prog"]], case["prog"]) == case["stderr"]


def test_read_errors_equal_the_reference(fm_check, tmp_path):
    case = next(c for c in mg.cases()["errors"] if c["name"] == "id_at")
    write_inputs(tmp_path, ["numeric.fa", "at.fa"])
    r = run([fm_check, "map"] + case["argv"], tmp_path)
    assert r.returncode == case["status"] == 1
    assert r.stdout.split(b"\n")[2:] == case["stdout"].encode().split(b"\n")[2:]  # the record before the bad one is printed
    assert [ln for ln in r.stderr.decode().splitlines() if not ln.startswith("Building")] == \
        [ln for ln in case["stderr"].splitlines() if not ln.startswith("Building")]
    (tmp_path / "empty.fa").write_text(">a\nACGTAC\n>e\n\n")
    r = run([fm_check, "map", "-l5", "empty.fa", "numeric.fa"], tmp_path)
    assert r.returncode == 1 and b"is empty" in r.stderr


REFUSED = [("abyss-map", ["-d", "a", "b"]), ("abyss-map", ["--dup", "a", "b"]), ("abyss-map", ["-a", "XYZ", "a", "b"]),
           ("abyss-map", ["--alpha", "a", "b"]), ("abyss-map", ["--protein", "a", "b"]), ("abyss-index", ["--bwt2fm", "a"]),
           ("abyss-index", ["-d", "a"]), ("abyss-index", ["--decompress", "a"]), ("abyss-index", ["--alpha", "a"]),
           ("abyss-index", ["--protein", "a"]), ("abyss-index", ["-aXYZ", "a"])]


@pytest.mark.parametrize("prog,argv", REFUSED, ids=lambda v: v if isinstance(v, str) else " ".join(v))
def test_unsupported_options_are_refused(prog, argv, bins, tmp_path):
    r = run([bins[prog]] + argv, tmp_path)
    assert r.returncode == 1 and r.stdout == b"" and b"is not supported" in r.stderr


def test_header_match_is_an_error_not_an_abort(fm_check, tmp_path):
    """-l no larger than a run of ACGT letters in an id: the reference fails an assertion, the drop-in says why and exits 1"""
    write_inputs(tmp_path, ["letters.fa"])
    (tmp_path / "q.fa").write_text(">q\nGATTACA\n")
    r = run([fm_check, "map", "-l5", "--no-rc", "q.fa", "letters.fa"], tmp_path)
    assert r.returncode == 1 and b"lies in a header line" in r.stderr


def test_multi_line_target_is_an_error_not_an_abort(fm_check, bins, tmp_path):
    """a record whose sequence runs over two lines: FastaIndex::index fails an assertion, the drop-in says why and exits 1 (the binary
    too: the target is indexed before a device is asked for)"""
    (tmp_path / "t.fa").write_text(">0\nACGTACGTAC\nGGGTTTAAAC\n>1\nACGT\n")
    (tmp_path / "q.fa").write_text(">q\nACGTACG\n")
    for cmd in ([fm_check, "map"], [bins["abyss-map"]]):
        r = run(cmd + ["-l5", "q.fa", "t.fa"], tmp_path)
        assert r.returncode == 1 and r.stdout == b"" and b"t.fa" in r.stderr and b"expected `>' at the start of a record" in r.stderr
    r = run([bins["abyss-index"], "--fai", "t.fa"], tmp_path)
    assert r.returncode == 1 and b"expected `>' at the start of a record" in r.stderr and not (tmp_path / "t.fa.fai").exists()


def test_abyss_pe_command_lines_are_accepted(bins, tmp_path):
    """bin/abyss-pe: `abyss-map $v -j$j -l$l $(ALIGNER_OPTIONS) $(MAP_OPTIONS) reads... target` and `abyss-index $v FILE`; the parsers take
    them and get as far as opening the files"""
    r = run([bins["abyss-map"], "-v", "-j8", "-l40", "--order", "missing_1.fq", "missing_2.fq", "missing-3.fa"], tmp_path)
    assert r.returncode == 1 and b"missing-3.fa" in r.stderr and b"invalid option" not in r.stderr and b"--help" not in r.stderr
    r = run([bins["abyss-map"], "-j2", "-l40", "--SS", "--db=x.sqlite", "--library=a", "--strain=b", "--species=c", "m_1.fq", "m-3.fa"], tmp_path)
    assert r.returncode == 1 and b"m-3.fa" in r.stderr and b"invalid option" not in r.stderr and b"--help" not in r.stderr
    r = run([bins["abyss-index"], "-v", "missing-3.fa"], tmp_path)
    assert r.returncode == 1 and b"missing-3.fa" in r.stderr and b"--help" not in r.stderr
    for p in ("abyss-map", "abyss-index"):
        r = run([bins[p], "--help"], tmp_path)
        assert r.returncode == 0 and r.stdout.startswith(b"Usage: " + p.encode())
        r = run([bins[p], "--version"], tmp_path)
        assert r.returncode == 0 and r.stdout.startswith(p.encode() + b" (ABySS")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


@pytest.mark.skipif(_have_gpu(), reason="a GPU is present")
def test_fm_index_has_no_cpu_fallback(bins, tmp_path):
    """abg_fm_create -> ABG_ENODEV without a GPU, and both binaries say so and exit 1 once they need the index"""
    with pytest.raises(api.AbyssAmdError) as e:
        api.FMIndex()
    assert "(-2)" in str(e.value) and "no HIP device" in str(e.value)
    write_inputs(tmp_path, ["numeric.fa", "nreads1.fa"])
    r = run([bins["abyss-map"], "-l5", "nreads1.fa", "numeric.fa"], tmp_path)
    assert r.returncode == 1 and r.stdout == b"" and b"no HIP device" in r.stderr
    r = run([bins["abyss-index"], "numeric.fa"], tmp_path)
    assert r.returncode == 1 and b"no HIP device" in r.stderr and not (tmp_path / "numeric.fa.fm").exists()
    assert (tmp_path / "numeric.fa.fai").read_bytes() == mg.golden("numeric.fa.fai")  # (--both writes the .fai first, as the reference)
