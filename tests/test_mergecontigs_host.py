"""MergeContigs on the host.  tests/hostcheck/mc_check runs the same mergecontigs_core.h as abyss_amd/bin/MergeContigs over the serial
text of abg_mc.h: it must write every golden case byte for byte (tests/golden/mergecontigs, from the unmodified reference).  The
plain-Python restatement must give the sequences and warnings the reference wrote, and flag the paths of the redo family only.  The
binary must write, with no device in sight, every case that has no path of two or more nodes.

`mc_check splice` runs the product's mc_layout, a serial copy of the junction walk over the ring, and a byte-by-byte splice from the
segments alone: on every generated set of the device tests (mergecontigs_golden.dirty_sets) it must give the restatement's sequences,
flags and ACGT counts.  The conditions those device tests rest on are asserted here for the restatement alone: it flags the planned
paths and no other, most sequences hold bytes that are not ACGT, all four kinds of segment and a two-part gap are laid out, a node
that is all window is followed by another junction, and marks, conflicts and gaps sit where they are planned."""
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


# ---- the generated sets of the device tests (mergecontigs_golden.dirty_sets), on the host

def acgt(s):
    return sum(s.count(c) for c in b"ACGTacgt")


def run_splice(mc_check, name, d):
    """`mc_check splice` on a set: ([(sequence, flag, count)], [segments of each kind], two-part gaps)"""
    s = mcg.dirty_sets()[name]
    mcg.dump_paths(d / "paths.txt", s["k"], s["contigs"], s["paths"])
    r = subprocess.run([mc_check, "splice", "paths.txt"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    words = lines[-1].split()
    assert words[:2] == ["#", "segments"] and len(lines) == len(s["paths"]) + 1
    return [(seq.encode(), int(flag), int(count)) for seq, flag, count in (l.split() for l in lines[:-1])], [int(w) for w in words[2:6]], int(words[-1])


@pytest.mark.parametrize("name", mcg.DIRTY_SETS)
def test_splice_over_the_layout_equals_the_restatement(name, mc_check, tmp_path):
    """mc_layout's segments, the ring walk and a byte-by-byte splice give py_merge_path's sequences, flags and ACGT counts; a path the
    ring cannot hold is the host's from the start (flag 2)"""
    s = mcg.dirty_sets()[name]
    got, kinds, two_part = run_splice(mc_check, name, tmp_path)
    for i, (seq, flagged, _) in enumerate(mcg.expected(name)):
        assert got[i] == (seq, 2 if i in s["host"] else int(flagged), acgt(seq)), i


def test_splice_refuses_a_dump_it_cannot_read(mc_check, tmp_path):
    (tmp_path / "paths.txt").write_text("25 1 1\nACGT\n2 0 0 2 3\n")
    r = subprocess.run([mc_check, "splice", "paths.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"no such contig" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("name", mcg.DIRTY_SETS)
def test_restatement_flags_the_planned_paths_only(name):
    s = mcg.dirty_sets()[name]
    assert [i for i, (_, flagged, _) in enumerate(mcg.expected(name)) if flagged] == s["flagged"]
    assert bool(s["flagged"]) == (name == "dirty.breaks" or name.startswith("conflict."))
    assert s["host"] == [i for i, (_, ov) in enumerate(s["paths"]) if max(ov) > 1024] and bool(s["host"]) == name.startswith("ring.")


def test_dirty_paths_hold_what_the_device_tests_need(mc_check, tmp_path):
    """the conditions of the main clean set: most sequences hold bytes that are not ACGT, every kind of segment is laid out, a node
    that is all window is followed by another junction, overlaps differ within a path, gaps of every planned size occur"""
    s, want = mcg.dirty_sets()["dirty"], mcg.expected("dirty")
    k = s["k"]
    assert len(s["paths"]) == 257 and all(2 <= len(nodes) <= 8 for nodes, _ in s["paths"])
    assert 2 * sum(acgt(seq) < len(seq) for seq, _, _ in want) >= len(want)
    got, kinds, two_part = run_splice(mc_check, "dirty", tmp_path)
    assert all(n > 0 for n in kinds), kinds
    length = lambda u: len(s["contigs"][u >> 1])
    assert any(u >= 0 and length(u) == o for nodes, ov in s["paths"] for u, o in list(zip(nodes, ov))[1:-1])
    assert any(len(set(ov[1:])) > 1 for _, ov in s["paths"])
    assert any(u & 1 for nodes, _ in s["paths"] for u in nodes if u >= 0) and any(not u & 1 for nodes, _ in s["paths"] for u in nodes if u >= 0)
    gaps = {-u for nodes, _ in s["paths"] for u in nodes if u < 0}
    assert {1, k - 2, k - 1, k, k + 1} <= gaps and max(gaps) > k + 1
    for nodes, ov in s["paths"]:
        assert nodes[0] >= 0 and nodes[-1] >= 0 and not any(u < 0 and v < 0 for u, v in zip(nodes, nodes[1:]))
        assert all(o == k - 1 for u, v, o in zip(nodes, nodes[1:], ov[1:]) if u < 0 or v < 0) and all(1 <= o <= 90 for o in ov[1:])
    text = b"".join(s["contigs"])
    assert all(text.count(c) for c in b"acgtNnRYMKSWBDHVrymkswbdhv")


def test_a_two_part_gap_is_laid_out(mc_check, tmp_path):
    """joined by k - 1 on both sides a gap never is (mergecontigs_golden._short_gap_set says why): the set with shorter joins lays out
    the N run and the n run of a gap side by side, and the restatement has them in its sequences"""
    got, kinds, two_part = run_splice(mc_check, "gaps.short", tmp_path)
    assert two_part > 0 and kinds[3] > two_part
    assert any(b"Nn" in seq for seq, _, _ in mcg.expected("gaps.short"))
    for name in ("dirty", "gaps"):
        assert run_splice(mc_check, name, tmp_path)[2] == 0


def test_marks_and_conflicts_sit_where_they_are_planned(mc_check, tmp_path):
    """the window set: the restatement has a lower-case base, a code or a plain base (the N gave way) at the marked position and
    upper-case ACGT everywhere else; the conflict sets: all of CONFLICTS occur, at CONFLICT_AT; the gap set: the gap's first own byte
    is at the planned offset of a 16-byte chunk; the seams set: three segments and more begin in a 16-byte chunk, on average"""
    s, want = mcg.dirty_sets()["window"], mcg.expected("window")
    seen = set()
    for p, at, kind in s["marks"]:
        seq = want[p][0]
        w = s["paths"][p][1][1]
        seen.add((kind, w, at - (len(s["contigs"][s["paths"][p][0][0] >> 1]) - w)))
        c = seq[at:at + 1]
        assert (c in b"acgt" if kind == "lower" else c in b"RYMKSWBDHV" if kind == "code" else c in b"ACGT") and len(c) == 1, (p, c)
        assert acgt(seq[:at] + seq[at + 1:]) == len(seq) - 1 and (seq[:at] + seq[at + 1:]).isupper()
    assert seen == {(kind, w, q) for kind in ("lower", "code", "N") for w in mcg.WINDOW_OVERLAPS for q in mcg.window_positions(w)}
    assert [mcg.window_positions(w) for w in (63, 129)] == [[0, 62], [0, 62, 63, 64, 128]]
    seen = set()
    for which in range(mcg.CONFLICT_SETS):
        c = mcg.dirty_sets()["conflict.%d" % which]
        assert len(c["paths"]) == 130 and sorted(c["breaks"]) == list(mcg.CONFLICT_AT) and all(len(nodes) == 4 for nodes, _ in c["paths"])
        seen |= {(c["paths"][p][1][place], q, place) for p, (place, q) in c["breaks"].items()}
    assert seen == set(mcg.CONFLICTS) and len(seen) == 3 * 19
    s, want = mcg.dirty_sets()["gaps"], mcg.expected("gaps")
    at = 0
    for (nodes, ov), (seq, _, _), (gap_at, target) in zip(s["paths"], want, s["gap_at"]):
        assert gap_at == at + len(s["contigs"][nodes[0] >> 1]) and gap_at % 16 == target and -nodes[1] in mcg.GAP_SIZES
        at += len(seq)
    assert sorted((-nodes[1], t) for (nodes, _), (_, t) in zip(s["paths"], s["gap_at"])) == sorted((n, t) for n in mcg.GAP_SIZES for t in (0, 1, 15))
    assert any(acgt(seq) < len(seq) - seq.count(b"N") - seq.count(b"n") < len(seq) for seq, _, _ in want)
    s = mcg.dirty_sets()["seams"]
    assert len(s["paths"]) == 64 and all(len(nodes) == 8 and all(1 <= o <= 3 for o in ov[1:]) for nodes, ov in s["paths"])
    assert all(1 <= len(c) <= 5 for c in s["contigs"])
    got, kinds, two_part = run_splice(mc_check, "seams", tmp_path)
    assert sum(kinds) >= 3 * (sum(len(seq) for seq, _, _ in got) + 15) // 16
