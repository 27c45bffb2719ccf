"""SimpleGraph on the host.  tests/hostcheck/sg_check runs the same simplegraph_core.h as abyss_amd/bin/SimpleGraph over the search
body of abg_sg.h executed serially: it must write every golden case byte for byte (tests/golden/simplegraph, from the unmodified
reference), and its search must equal the plain-Python restatement of the recursive search on the small shapes.  The restatement
itself must give the paths the reference printed under -v.  The binary must write, with no device in sight, every case in which
nothing is searched, and say so and exit 1 where something is."""
import os
import shlex
import subprocess

import pytest

from abyss_amd import build
import simplegraph_golden as sgg

NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "AMD_LOG_LEVEL": "4"}


@pytest.fixture(scope="module")
def sg_check():
    build.build_hostcheck()
    return build.SG_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "SimpleGraph")


@pytest.mark.parametrize("case", sgg.cases(), ids=lambda c: c["name"])
def test_sg_check_writes_what_the_reference_wrote(case, sg_check, tmp_path):
    sgg.check_case(case, sgg.run_case([sg_check, "run"], case, tmp_path))


def _summary(case):
    text = sgg.golden(case["stdout"]).decode()
    return {l.split(": ")[0]: int(l.split(": ")[1]) for l in text.splitlines() if ": " in l and l.split(": ")[1].isdigit()}


def test_the_goldens_reach_every_outcome():
    by_name = {c["name"]: c for c in sgg.cases()}
    s = _summary(by_name["main.default"])
    assert (s["Total paths attempted"], s["Unique path"], s["No possible paths"]) == (41, 36, 5)
    reached = {}
    for c in sgg.cases():
        if c["stdout"] and c["status"] == 0:
            for key, n in _summary(c).items():
                reached[key] = max(reached.get(key, 0), n)
    for key in ("Seed too short", "Seeds with no edges", "Edges removed", "Unique path", "No possible paths", "No valid paths", "Repetitive",
                "Multiple valid paths", "Too many solutions", "Too complex"):
        assert reached[key] > 0, key
    assert _summary(by_name["ladder8.cost_exact"])["Too complex"] == 1 and _summary(by_name["ladder8.cost_above"])["Too complex"] == 0
    # the ambiguous node spans the longest way between the spines: n rungs of 51 and n - 1 spines of 100, every junction an overlap
    # of k - 1 = 31, plus k - 1 by the convention of the path files
    for n in (3, 7):
        gap = 51 * n + 100 * (n - 1) - 31 * 2 * n + 31
        for fmt in ("adj", "dot"):
            assert b"s0\ts0+ %dN s%d+\n" % (gap, n) == sgg.golden(by_name["ladder%d.%s_default" % (n, fmt)]["out"])
    assert b"s0\ts0+ 198N s3+\n" == sgg.golden(by_name["ladder3.adj_default"]["out"])
    for inp in ("main", "samesense", "ambig"):  # our previous stage's graphs in both formats, to the same paths
        assert sgg.golden(by_name[inp + ".dot"]["out"]) == sgg.golden(by_name[inp + ".default"]["out"])
    assert any(b"Consider increasing" in sgg.golden(c["stdout"]) for c in sgg.cases() if c["stdout"])
    assert sum(1 for c in sgg.cases() if not sgg.needs_device(c)) >= 10 and sum(1 for c in sgg.cases() if sgg.needs_device(c)) >= 40


VERBOSE_ADJ = [c for c in sgg.cases() if c["status"] == 0 and sgg.needs_device(c) and c["inputs"][0].endswith(".adj")
               and any(a in ("-v", "-vv", "--verbose") for a in c["argv"])]


@pytest.mark.parametrize("case", VERBOSE_ADJ, ids=lambda c: c["name"])
def test_restatement_gives_the_paths_the_reference_printed(case):
    k = int(next(a for a in case["argv"] if a.startswith("-k"))[2:])
    cost = next((int(a.split("=")[1]) for a in case["argv"] if a.startswith("--max-cost=")), sgg.MAX_COST)
    g, names = sgg.parse_adj(sgg.golden(case["inputs"][0]), k)
    ids = {n: i for i, n in enumerate(names)}
    vertex = lambda s: 2 * ids[s[:-1]] + (s[-1] == "-")
    name = lambda v: names[v >> 1] + "+-"[v & 1]
    blocks = sgg.verbose_blocks(sgg.golden(case["stdout"]))
    assert blocks
    for origin, cons, paths, sol in blocks:
        visited, found = sgg.py_search(g, vertex(origin), [(vertex(v), b) for v, b in cons], max_cost=cost)
        assert [" ".join(name(v) for v in p) for p in found] == paths, origin
        assert ("(too complex)" in sol) == (visited >= cost) and ("(too many solutions)" in sol) == (len(found) > sgg.MAX_PATHS), origin


NO_SEARCH = [c for c in sgg.cases() if not sgg.needs_device(c)]


@pytest.mark.parametrize("case", NO_SEARCH, ids=lambda c: c["name"])
def test_binary_without_a_device_writes_the_cases_that_need_no_search(case, binary, tmp_path):
    """the HIP runtime is never started: AMD_LOG_LEVEL=4 would make it talk on stderr, which is compared"""
    sgg.check_case(case, sgg.run_case([binary], case, tmp_path, env=NO_DEVICE))


def test_binary_without_a_device_says_so(binary, tmp_path):
    case = next(c for c in sgg.cases() if c["name"] == "main.default")
    e = dict(NO_DEVICE)
    e.pop("AMD_LOG_LEVEL")
    status, out, err, path = sgg.run_case([binary], case, tmp_path, env=e)
    assert status == 1 and out == b""
    assert err.splitlines()[-1] == "SimpleGraph: error: no HIP device available (abyss_amd has no CPU fallback)"


def test_refused_graph_formats_and_ignored_options(binary, tmp_path):
    case = next(c for c in sgg.cases() if c["name"] == "nosearch.empty")
    for name in case["inputs"]:
        (tmp_path / name).write_bytes(sgg.golden(name))
    env = dict(os.environ, **NO_DEVICE)
    (tmp_path / "g.gfa").write_bytes(b"H\tVN:Z:1.0\n")
    r = subprocess.run([binary, "-k32", "-o", "o.path", "g.gfa", "empty.dist"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)
    assert r.returncode == 1 and b"GraphViz (--dot) or ADJ format only" in r.stderr
    r = subprocess.run([binary, "--db=x.db", "--library=l", "--strain=s", "--species=p", "-j7"] + case["argv"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=60)
    assert r.returncode == 0 and r.stdout == sgg.golden(case["stdout"]) and not os.path.exists(tmp_path / "x.db")


def test_abyss_pe_rule_lines_parse(binary, tmp_path):
    """the command lines `make -n` of the unmodified bin/abyss-pe prints for the -4.path1 rule: every option is one this program takes,
    the -o file is the rule's target and the two arguments are its prerequisites"""
    rules = {name: rule for name, rule in sgg.rules().items() if not name.startswith("_")}
    assert set(rules) == {"plain", "v", "adj_options"}
    for name, rule in rules.items():
        argv = rule["argv"]
        assert shlex.split(rule["recipe"])[-len(argv):] == argv
        assert argv[argv.index("-o") + 1] == rule["target"] and argv[-2:] == rule["inputs"]
        assert ("-v" in argv) == ("v=-v" in rule["make_args"])
        r = subprocess.run([binary] + argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **NO_DEVICE), timeout=60)
        assert r.returncode == 1 and rule["inputs"][0] in r.stderr.decode() and "option" not in r.stderr.decode(), r.stderr


SHAPES = sgg.small_shapes() + [sgg.wave_shape(n) for n in (1, 65)]


@pytest.mark.parametrize("shape", sgg.small_shapes(), ids=lambda s: s.name)
def test_small_shapes_are_what_they_claim(shape):
    for (visited, paths), (npaths, nvisited) in zip(shape.expected(), shape.claim):
        assert npaths is None or len(paths) == npaths, shape.name
        assert nvisited is None or visited == nvisited, shape.name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s.name)
def test_tie_order_of_equal_bounds_changes_nothing(shape):
    """the claim of abg_sg.h that lets it drop the bound-sorted copy: the restatement keeps the copy, and gives the same answer with
    the equal bounds in the other order"""
    assert [sgg.py_search(shape.graph, o, c, shape.max_cost, reverse_ties=True) for o, c in shape.searches] == shape.expected()


def test_the_hard_search_runs_to_the_cost():
    shape = sgg.wave_shape(65)
    assert sorted(v for v, _ in shape.expected())[-1] == sgg.MAX_COST and sum(1 for v, _ in shape.expected() if v >= sgg.MAX_COST) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s.name)
def test_sg_check_search_equals_the_restatement(shape, sg_check, tmp_path):
    sf, rf = str(tmp_path / "searches"), str(tmp_path / "results")
    sgg.write_searches(sf, shape.graph, shape.searches, max_cost=shape.max_cost)
    subprocess.run([sg_check, "search", sf, rf], check=True, timeout=120)
    assert read_equal(sgg.read_results(rf, len(shape.searches)), shape.expected())


def read_equal(got, want):
    for i, ((gv, gp), (wv, wp)) in enumerate(zip(got, want)):
        assert gv == wv and gp == wp, i
    return len(got) == len(want)
