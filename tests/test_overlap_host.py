"""Overlap on the host.  tests/hostcheck/ov_check runs the same overlap_core.h as abyss_amd/bin/Overlap over the search body of
abg_ov.h executed serially: it must write every golden case byte for byte (tests/golden/overlap, from the unmodified reference), and
its search must equal the plain-Python restatement on the small shapes.  The binary itself must write, with no device in sight,
every case in which no pair reaches findOverlap, and say so and exit 1 where one does."""
import os
import shlex
import subprocess

import pytest

from abyss_amd import build
import overlap_golden as og

NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "AMD_LOG_LEVEL": "4"}


@pytest.fixture(scope="module")
def ov_check():
    build.build_hostcheck()
    return build.OV_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "Overlap")


@pytest.mark.parametrize("case", og.cases(), ids=lambda c: c["name"])
def test_ov_check_writes_what_the_reference_wrote(case, ov_check, tmp_path):
    prefix = [ov_check, "run"]
    og.check_case(case, og.run_case(prefix, case, tmp_path), prefix)


NO_SEARCH = [c for c in og.cases() if not og.needs_device(c)]


def test_the_goldens_cover_both_kinds_of_run():
    assert len(NO_SEARCH) >= 10 and len(og.cases()) - len(NO_SEARCH) >= 20
    assert any(c["status"] == 0 and c["out_fa"] and og.golden(c["out_fa"]) for c in NO_SEARCH)  # a run that scaffolds without a search


@pytest.mark.parametrize("case", NO_SEARCH, ids=lambda c: c["name"])
def test_binary_without_a_device_writes_the_cases_that_need_no_search(case, binary, tmp_path):
    """the HIP runtime is never started: AMD_LOG_LEVEL=4 would make it talk on stderr, which is compared"""
    got = og.run_case([binary], case, tmp_path, env=NO_DEVICE)
    og.check_case(case, got, [binary])


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in og.cases() if c["name"] == "main.default")
    e = dict(NO_DEVICE)
    e.pop("AMD_LOG_LEVEL")
    status, out, err, fa, g = og.run_case([binary], case, tmp_path, env=e)
    assert status == 1 and out == b"" and g is None
    assert err.splitlines()[-1] == "Overlap: error: no HIP device available (abyss_amd has no CPU fallback)"


def test_where_the_reference_asserts_the_binary_names_the_input(binary, tmp_path):
    case = next(c for c in og.cases() if c["name"] == "nosearch.default")
    for name in case["inputs"]:
        (tmp_path / name).write_bytes(og.golden(name))
    (tmp_path / "empty.fa").write_bytes(b"")
    (tmp_path / "far.dist").write_bytes(b"0 1-,100000,20,3.0 ;\n")
    (tmp_path / "self.dot").write_bytes(b'digraph dist {\n"0+" -> "0-" [d=-3 e=1.0 n=5]\n}\n')
    for argv, what in ((["empty.fa", "nosearch.adj", "nosearch.dist"], "empty.fa"), (["nosearch.fa", "nosearch.adj", "far.dist"], "far.dist"),
                       (["nosearch.fa", "nosearch.adj", "self.dot"], "self.dot")):
        r = subprocess.run([binary, "-k32", "-o", "o.fa"] + argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **NO_DEVICE),
                           timeout=60)
        assert r.returncode == 1 and what in r.stderr.decode(), (argv, r.stderr)


def test_abyss_pe_rule_lines_parse(binary, tmp_path):
    """the command lines `make -n` of the unmodified bin/abyss-pe prints for the -4.fa rule: every option is one this program takes, and
    the -o and -g files are the rule's two targets"""
    rules = og.rules()
    assert len(rules) >= 4
    for name, rule in rules.items():
        if name.startswith("_"):
            continue
        argv = rule["argv"]
        assert shlex.split(rule["recipe"])[1:] == argv
        assert [argv[argv.index("-o") + 1], argv[argv.index("-g") + 1]] == rule["targets"]
        assert ("--SS" in argv) == ("SS=--SS" in rule["make_args"]) and ("-v" in argv) == ("v=-v" in rule["make_args"])
        # the inputs do not exist: the options parse and the program stops at the first file, not at an option
        r = subprocess.run([binary] + argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **NO_DEVICE), timeout=60)
        assert r.returncode == 1 and "asm-3.fa" in r.stderr.decode() and "option" not in r.stderr.decode(), r.stderr


@pytest.mark.parametrize("group", og.small_shapes(), ids=lambda g: g.name)
def test_small_shapes_are_what_they_claim(group):
    og.check_claims(group)


def test_small_shapes_cover_the_list():
    groups = {g.name: g for g in og.small_shapes()}
    lengths = groups["lengths"]
    mins = set(min(len(lengths.oriented(t)), len(lengths.oriented(h))) for t, h in lengths.pairs)
    assert set(og.MIN_LENGTHS) <= mins
    ratios = [len(lengths.oriented(t)) / len(lengths.oriented(h)) for t, h in lengths.pairs]
    assert max(ratios) > 1000 and min(ratios) < 0.001  # |t| >> |h| and |h| >> |t|
    for g in groups.values():
        if not g.name.startswith("placement"):
            assert set((t & 1, h & 1) for t, h in g.pairs) == {(0, 0), (0, 1), (1, 0), (1, 1)}, g.name
    found = {l: f for l, f in zip(groups["sets"].labels, groups["sets"].expected())}
    assert found["no_match"] == [] and found["single_1"] == [1] and found["two_steps_128_64_1"] == [128, 64, 1]
    assert found["ends_64"] == [64, 1] and found["ends_65"] == [65, 1]
    assert any(len(f) == 2 for f in found.values()) and any(len(f) > 3 for f in found.values())
    assert found["homopolymer_130_70"] == list(range(70, 0, -1))
    assert {"period_2_90", "period_3_100", "period_7_150"} <= set(found)
    assert any(c.islower() for g in groups.values() for s in g.contigs for c in s)
    assert any(c in "NMRWSYKVHDB" for s in groups["bytes"].contigs for c in s)
    assert {"placement_late_t", "placement_long_l", "placement_early_t"} <= set(groups)


@pytest.mark.parametrize("group", og.small_shapes(), ids=lambda g: g.name)
def test_ov_check_find_equals_the_restatement(group, ov_check, tmp_path):
    pf, rf = str(tmp_path / "pairs"), str(tmp_path / "results")
    og.write_pairs(pf, group.folded(), group.pairs)
    subprocess.run([ov_check, "find", pf, rf], check=True, timeout=120)
    got = og.read_results(rf, len(group.pairs))
    for (top, ntop, found), want, label in zip(got, group.expected(), group.labels):
        assert found == want, label
        assert ntop == min(3, len(want)) and top == (want[:3] + [0, 0, 0])[:3], label
