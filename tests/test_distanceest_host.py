"""DistanceEst without a GPU: tests/hostcheck/de_check runs distanceest_core.h over the serial bodies of abyss_amd/csrc/abg_de.h, and
every byte is compared with what the unmodified reference wrote at -j1 (tests/golden/distanceest, tests/golden/make_distanceest.py).
The binary itself runs where it needs no device: --mean, --median, the option and input errors, the abyss-pe rule lines.  The scan's
serial bodies are compared bit for bit with a plain-Python restatement of the reference's loops."""
import os
import subprocess

import pytest

from abyss_amd import build
import distanceest_golden as dg


@pytest.fixture(scope="module")
def de_check():
    build.build_hostcheck()
    return build.DE_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "DistanceEst")


@pytest.mark.parametrize("case", dg.cases(), ids=lambda c: c["name"])
def test_de_check_writes_what_the_reference_wrote(case, de_check, tmp_path):
    dg.check_case(case, dg.run_case([de_check, "run"], case, tmp_path))


# AMD_LOG_LEVEL=4 makes the HIP runtime log every API call, its own start-up included, to stderr, which check_case compares byte for
# byte: a run that passes with it made no HIP call at all (test_mle_without_a_device_says_so shows the log where one is made).
NO_HIP = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "AMD_LOG_LEVEL": "4"}


@pytest.mark.parametrize("case", [c for c in dg.cases() if not dg.needs_device(c)], ids=lambda c: c["name"])
def test_binary_without_a_device(case, binary, tmp_path):
    """--mean, --median and the errors that come before any contig pair never start the HIP runtime"""
    dg.check_case(case, dg.run_case([binary], case, tmp_path, env=NO_HIP))


def test_threads_change_no_byte(de_check, tmp_path):
    for name in ("fr_basic.dist", "fr_basic.median_dot", "rf_matepair.gfa2"):
        case = next(c for c in dg.cases() if c["name"] == name)
        argv = ["-j16" if a == "-j1" else a for a in case["argv"]]
        dg.check_case(case, dg.run_case([de_check, "run"], case, tmp_path, argv=argv))


@pytest.mark.parametrize("block", ["64", "1000", "5003", "20000"])
@pytest.mark.parametrize("name", ["fr_basic.dist", "rf_matepair.vv_dot", "short_frag.vv_n12", "error.unsorted"])
def test_small_input_blocks_change_no_byte(name, block, de_check, tmp_path):
    """ABG_DE_BLOCK_BYTES: the input in blocks of a few records (64 bytes: less than a line, so a block grows until it holds one),
    every block cut at a line end, refilled many times and parsed in pieces on -j16 threads"""
    case = next(c for c in dg.cases() if c["name"] == name)
    assert len(dg.golden(case["sam"])) > 3 * int(block)
    argv = ["-j16" if a == "-j1" else a for a in case["argv"]]
    dg.check_case(case, dg.run_case([de_check, "run"], case, tmp_path, argv=argv, env={"ABG_DE_BLOCK_BYTES": block}))


def test_mle_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in dg.cases() if c["name"] == "fr_basic.stdout")
    status, out, err, _ = dg.run_case([binary], case, tmp_path, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert status == 1 and out == b""
    assert err.splitlines() == ["DistanceEst: error: no HIP device available (abyss_amd has no CPU fallback)"]
    # ... and with the runtime's log on, the one HIP call it made shows: what test_binary_without_a_device would trip over
    status, out, err, _ = dg.run_case([binary], case, tmp_path, env=NO_HIP)
    assert status == 1 and len(err.splitlines()) > 1 and "hipGetDeviceCount" in err


@pytest.mark.parametrize("name", [k for k in dg.rules() if not k.startswith("_")])
def test_abyss_pe_rule_lines_parse(name, binary, tmp_path):
    """the command lines bin/abyss-pe issues for its -3.dist and -6.dist.dot rules: accepted, and the -o file is the rule's target"""
    rule = dg.rules()[name]
    argv = rule["argv"]
    hist = argv[-1]
    (tmp_path / hist).write_bytes(dg.golden("fr_basic.lib.hist"))
    r = subprocess.run([binary] + argv, cwd=str(tmp_path), input=b"@SQ\tSN:0\tLN:5000\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr
    target = rule["make_args"][-1]
    assert argv[argv.index("-o") + 1] == target
    want = b"digraph dist {\ngraph [k=%s s=%s n=%s]\n" % tuple(next(a[2:] for a in argv if a.startswith(o)).encode() for o in ("-k", "-s", "-n")) \
        if "--dot" in argv else b""
    assert (tmp_path / target).read_bytes() == want
    assert (b"Mate orientation" in r.stderr) == ("-v" in argv)


@pytest.fixture(scope="module")
def restated():
    """the Python restatement of every small shape, computed once"""
    return {g[0]: dg.py_scan(g[1], g[2], g[4], g[5], g[6], g[7]) for g in dg.small_shapes()}


@pytest.mark.parametrize("group", dg.small_shapes(), ids=lambda g: g[0])
def test_serial_scan_is_the_reference_arithmetic(group, restated, de_check, tmp_path):
    name, pmf, minp, mean, jobs, values, counts, offsets = group
    jf, of = str(tmp_path / "jobs"), str(tmp_path / "scan")
    dg.write_jobs(jf, pmf, minp, mean, jobs, values, counts, offsets)
    subprocess.run([de_check, "scan", jf, of], check=True, timeout=60)
    c, like, n = dg.read_scan(of, jobs)
    wc, wl, wn = restated[name]
    assert dg.same_bits(c, wc) and dg.same_bits(like, wl) and dg.same_bits(n, wn)
    assert len(c) == sum(dg.thetas(jobs))


def test_small_shapes_cover_what_they_claim():
    groups = dg.small_shapes()
    assert {len(g[1]) for g in groups} >= {1, 2, 63, 64, 65, 257, 1000}
    assert {t for g in groups for t in dg.thetas(g[4])} >= {0, 1, 63, 64, 65, 257, 1025}
    assert {int(j["len0"]) for g in groups for j in g[4]} >= {1, 3, 7, 997, 123457}
    assert any(len(g[4]) == 200 for g in groups)
    assert max(int(k) for g in groups for k in g[6]) > 50000 and any(int(o[i + 1] - o[i]) == 300 for g in groups for o in [g[7]] for i in range(len(o) - 1))
