"""MergeContigs on the host.  tests/hostcheck/mc_check runs the same mergecontigs_core.h as abyss_amd/bin/MergeContigs over the serial
text of abg_mc.h: it must write every golden case byte for byte (tests/golden/mergecontigs, from the unmodified reference).  The
plain-Python restatement must give the sequences and warnings the reference wrote, and flag the paths of the redo family only.  The
binary must write, with no device in sight, every case that has no path of two or more nodes."""
import os
import shlex
import subprocess

import pytest

from abyss_amd import build
import mergecontigs_golden as mcg

NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "AMD_LOG_LEVEL": "4"}


@pytest.fixture(scope="module")
def mc_check():
    build.build_hostcheck()
    return build.MC_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "MergeContigs")


@pytest.mark.parametrize("case", mcg.cases(), ids=lambda c: c["name"])
def test_mc_check_writes_what_the_reference_wrote(case, mc_check, tmp_path):
    mcg.check_case(case, mcg.run_case([mc_check, "run"], case, tmp_path))


def test_the_goldens_reach_every_family():
    by_name = {c["name"]: c for c in mcg.cases()}
    assert {c["family"] for c in mcg.cases()} == set(range(1, 9))
    out = mcg.golden(by_name["exact.k64"]["out"]).decode()
    headers = [l for l in out.splitlines() if l.startswith(">p")]
    assert [h.split()[3].count(",") for h in headers] == [1, 2, 2, 2] and ",...," in headers[2] and ",...," in headers[3] and ",...," not in headers[1]
    redo = by_name["redo.vvv"]["stderr"]
    assert "(good)" in redo and "(too low)" in redo and redo.count("warning: the head of") >= 2 and "(too few)" in by_name["redo.toofew_vvv"]["stderr"]
    assert "Consider increasing" in by_name["files.coverage_advice"]["stderr"] and "inf" in by_name["files.coverage_inf"]["stderr"]
    assert "n:200" in by_name["files.v"]["stderr"] and "V=" in by_name["files.adj_g_default_v"]["stderr"]
    formats = {c["name"].split("_to")[1] for c in mcg.cases() if "_to" in c["name"]}
    assert formats == {"adj", "dot", "gv", "dot-meancov", "gfa", "gfa1", "gfa2", "sam"}
    assert sum(1 for c in mcg.cases() if c.get("aborts")) >= 8 and sum(1 for c in mcg.cases() if c.get("refused")) == 1
    assert sum(1 for c in mcg.cases() if mcg.needs_device(c)) >= 40 and sum(1 for c in mcg.cases() if mcg.needs_device(c) is False) >= 4


MERGING = [c for c in mcg.cases() if mcg.needs_device(c) and c["out"] and "-" not in c["argv"] and not any(a.endswith(".dot") for a in c["argv"])]


@pytest.mark.parametrize("case", MERGING, ids=lambda c: c["name"])
def test_restatement_gives_what_the_reference_wrote(case):
    """the sequences of the -o file and the warnings of stderr; and it flags a path in the redo family and the non-subset case only"""
    k, contigs, paths = mcg.case_paths(case)
    verbose = sum(a.count("v") if a.startswith("-v") else a == "--verbose" for a in case["argv"])
    fasta = dict((n, s) for n, s in mcg.read_fasta(mcg.golden(case["out"])))
    args = [a for a in case["argv"] if a in case["inputs"]]
    names = mcg.read_adj(mcg.golden(args[1]), k)[0] if len(args) == 3 else [n for n, _ in mcg.read_fasta(mcg.golden(args[0]))]
    name = lambda u: "%dN" % -u if u < 0 else names[u >> 1] + "+-"[u & 1]
    flagged, log = 0, ""
    for pid, nodes, ov in paths:
        seq, f, text = mcg.py_merge_path(contigs, k, nodes, ov, verbose, name)
        assert seq == fasta[pid], pid
        flagged += f
        log += text
    assert log == "" or log in case["stderr"]
    assert ("warning: the head of" in log) == ("warning: the head of" in case["stderr"])
    expects_redo = case["family"] == 5 or case["name"] == "consensus.nonsubset"
    assert (flagged > 0) == expects_redo, flagged


NO_MERGE = [c for c in mcg.cases() if mcg.needs_device(c) is False]


@pytest.mark.parametrize("case", NO_MERGE, ids=lambda c: c["name"])
def test_binary_without_a_device_writes_the_cases_that_merge_nothing(case, binary, tmp_path):
    """the HIP runtime is never started: AMD_LOG_LEVEL=4 would make it talk on stderr, which is compared"""
    mcg.check_case(case, mcg.run_case([binary], case, tmp_path, env=NO_DEVICE))


def test_refused_graph_formats_and_ignored_options(binary, tmp_path):
    case = next(c for c in mcg.cases() if c["name"] == "files.nopaths")
    for name in case["inputs"]:
        (tmp_path / name).write_bytes(mcg.golden(name))
    env = dict(os.environ, **NO_DEVICE)
    (tmp_path / "g.gfa").write_bytes(b"H\tVN:Z:1.0\n")
    r = subprocess.run([binary, "-k32", "-o", "o.fa", case["inputs"][0], "g.gfa", "none.path"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)
    assert r.returncode == 1 and b"GraphViz (--dot) or ADJ format only" in r.stderr
    r = subprocess.run([binary, "--db=x.db", "--library=l", "--strain=s", "--species=p"] + case["argv"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=60)
    assert r.returncode == 0 and (tmp_path / "out.fa").read_bytes() == mcg.golden(case["out"]) and not os.path.exists(tmp_path / "x.db")


def test_abyss_pe_rule_lines_parse(binary, tmp_path):
    """the command lines `make -n` of the unmodified bin/abyss-pe prints for the -2.fa, -3.fa and -6.fa rules: every option is one this
    program takes and the -o file is the rule's target; with no such files the run stops at the first input, not at an option"""
    rules = {name: rule for name, rule in mcg.rules().items() if not name.startswith("_")}
    assert set(rules) == {"contigs", "contigs_adj_v", "pe_contigs"}
    for name, rule in rules.items():
        assert rule["recipes"][-1]["target"] == rule["make_args"][-1]
        for recipe in rule["recipes"]:
            argv = recipe["argv"]
            assert "MergeContigs" in shlex.split(recipe["recipe"]) and argv[argv.index("-o") + 1] == recipe["target"]
            assert ("-v" in argv) == ("v=-v" in rule["make_args"]) and (argv[-3] == "-") == recipe["stdin"]
            r = subprocess.run([binary] + argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **NO_DEVICE), timeout=60, input=b"")
            assert r.returncode == 1 and argv[-2] in r.stderr.decode() and "option" not in r.stderr.decode(), r.stderr
