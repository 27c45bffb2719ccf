"""SimpleGraph and api.PathSearch on the GPU.  The search must equal the plain-Python restatement of the recursive search on the small
shapes (visit counts and paths, in discovery order), with 1 to 257 searches a call of which one runs to the cost cap, twice in a row,
with ABG_SG_BATCH set to hit the batch seams and with the kernel's limits shrunk so that searches are flagged and redone on the host;
and the binary must write every golden case byte for byte (tests/golden/simplegraph, from the unmodified reference) at the default
batch and at one search a batch."""
import os

import pytest

from abyss_amd import api, build
import simplegraph_golden as sgg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "SimpleGraph")


def run(shape, expect_redone=None, twice=False, lanes=0):
    ps = api.PathSearch()
    try:
        if lanes:
            ps.tune(lanes=lanes)
        ps.set_graph(*shape.graph.csr())
        for _ in range(2 if twice else 1):
            visited, redone, paths = ps.search(shape.searches, max_cost=shape.max_cost)
            for i, (v, p) in enumerate(shape.expected()):
                assert int(visited[i]) == v and paths[i] == p, (shape.name, i)
            if expect_redone is not None:
                assert redone.tolist() == expect_redone, shape.name
    finally:
        ps.close()


def test_equal_bounds_give_what_the_restatement_gives():
    """abg_sg.h keeps no bound-sorted copy of the constraints, on the claim that the order of equal bounds cannot matter: the
    restatement keeps the copy and walks it as the reference does"""
    shape = next(s for s in sgg.small_shapes() if s.name == "equal_bounds")
    assert [len(p) for _, p in shape.expected()] == [4, 2]
    run(shape, expect_redone=[False, False])


@pytest.mark.parametrize("shape", sgg.small_shapes(), ids=lambda s: s.name)
def test_search_equals_the_restatement(shape):
    run(shape, expect_redone=[False] * len(shape.searches), twice=True)


def test_the_eight_bubble_ladder_keeps_201_paths():
    shape = next(s for s in sgg.small_shapes() if s.name == "bubbles_8")
    assert all(len(p) == 201 for _, p in shape.expected())
    run(shape)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_seams_with_one_search_at_the_cost_cap(n):
    shape = sgg.wave_shape(n)
    assert n < 3 or max(v for v, _ in shape.expected()) == sgg.MAX_COST
    run(shape, expect_redone=[False] * n, twice=True)


@pytest.mark.parametrize("n", [65, 257])
def test_every_lane_refills(n):
    """64 lanes for 65 and 257 searches: a lane must take a second search when its first ends (a fresh state on a used stack column),
    the lane of the 100,000-visit search among them or not, and the last searches are taken while that one still runs"""
    shape = sgg.wave_shape(n)
    assert max(v for v, _ in shape.expected()) == sgg.MAX_COST
    run(shape, expect_redone=[False] * n, twice=True, lanes=64)


def test_refill_after_searches_that_record_paths():
    """64 lanes, 200 searches that each record paths and unwind a stack: the second and third search of a lane must start clean"""
    g = sgg.ladder(3)
    end = sgg.along(g, [v for i in (1, 2, 3) for v in (g.branch(i, 1), g.spine(i))])
    searches = [(0, [(g.spine(3), end)]), (0, [(g.spine(2), end), (g.spine(1), end)]), (g.spine(1), [(g.spine(3), end)]), (0, [(g.spine(3), end - 3)])] * 50
    run(sgg.Shape("refill", g, searches), expect_redone=[False] * 200, twice=True, lanes=64)


@pytest.mark.parametrize("batch", ["1", "2", "7"])
def test_batch_seams(batch, monkeypatch):
    monkeypatch.setenv("ABG_SG_BATCH", batch)
    for shape in sgg.small_shapes():
        run(shape)
    run(sgg.wave_shape(65))


def test_batch_seams_with_fewer_lanes_than_searches(monkeypatch):
    monkeypatch.setenv("ABG_SG_BATCH", "130")
    monkeypatch.setenv("ABG_SG_LANES", "64")
    run(sgg.wave_shape(257), expect_redone=[False] * 257)


def test_searches_that_fill_the_arena_together_go_out_again(monkeypatch):
    """bubbles_3 records 8 paths of 6 vertices and 2 words each a search, 64 words: both searches fit an arena of 100 words one at a
    time, not side by side, and neither is left to the host"""
    monkeypatch.setenv("ABG_SG_ARENA_WORDS", "100")
    shape = next(s for s in sgg.small_shapes() if s.name == "bubbles_3")
    run(shape, expect_redone=[False, False], twice=True)


def test_forced_limits_flag_and_redo(monkeypatch):
    """a stack of 3 frames, 1 constraint a search, an arena of 40 words: the searches that outgrow them come back identical and marked"""
    shapes = {s.name: s for s in sgg.small_shapes()}
    monkeypatch.setenv("ABG_SG_STACK_DEPTH", "3")
    run(shapes["bubbles_3"], expect_redone=[True, True])       # six vertices deep
    run(shapes["single_edge"], expect_redone=[False, False])   # one deep
    monkeypatch.delenv("ABG_SG_STACK_DEPTH")
    monkeypatch.setenv("ABG_SG_MAX_CONSTRAINTS", "1")
    run(shapes["bubbles_3"], expect_redone=[False, True])
    run(shapes["equal_bounds"], expect_redone=[True, True])
    monkeypatch.delenv("ABG_SG_MAX_CONSTRAINTS")
    monkeypatch.setenv("ABG_SG_ARENA_WORDS", "40")
    run(shapes["bubbles_3"])                                    # 8 paths of 6 vertices and 2 words each need 64 words a search
    run(shapes["bubbles_8"], expect_redone=[True, True])
    run(shapes["single_edge"], expect_redone=[False, False])
    ps = api.PathSearch()
    try:
        ps.tune(stack_depth=3)
        ps.set_graph(*shapes["bubbles_3"].graph.csr())
        assert ps.search(shapes["bubbles_3"].searches)[1].tolist() == [True, True]
    finally:
        ps.close()


def test_empty_calls_and_bad_input():
    shape = sgg.small_shapes()[0]
    ps = api.PathSearch()
    try:
        with pytest.raises(api.AbyssAmdError, match="no graph has been set"):
            ps.search([(0, [(2, 5)])])
        ps.set_graph(*shape.graph.csr())
        visited, redone, paths = ps.search([])
        assert len(visited) == 0 and len(redone) == 0 and paths == []
        visited, redone, paths = ps.search([(0, [])])  # no constraint: nothing is searched
        assert visited.tolist() == [0] and paths == [[]]
        with pytest.raises(api.AbyssAmdError, match="search 1: no such vertex"):
            ps.search([(0, [(2, 5)]), (len(shape.graph.length), [(2, 5)])])
        with pytest.raises(api.AbyssAmdError, match="no such vertex"):
            ps.search([(0, [(len(shape.graph.length), 5)])])
    finally:
        ps.close()


@pytest.mark.parametrize("mode", ["default", "one_search_a_batch"])
@pytest.mark.parametrize("case", [c for c in sgg.cases() if sgg.needs_device(c)], ids=lambda c: c["name"])
def test_binary_writes_what_the_reference_wrote(case, mode, binary, tmp_path):
    env = {"ABG_SG_BATCH": "1"} if mode == "one_search_a_batch" else {}
    sgg.check_case(case, sgg.run_case([binary], case, tmp_path, env=env))


REFILL = [c for c in sgg.cases() if c.get("searches", 0) > 64]


@pytest.mark.parametrize("case", REFILL, ids=lambda c: c["name"])
def test_binary_with_fewer_lanes_than_searches(case, binary, tmp_path):
    """one wave for more than 64 searches: every golden run of that size with each lane taking a second search"""
    sgg.check_case(case, sgg.run_case([binary], case, tmp_path, env={"ABG_SG_LANES": "64"}))


def test_golden_runs_with_more_than_a_wave_of_searches_exist():
    assert len(REFILL) >= 3 and any("-v" in c["argv"] for c in REFILL)


def test_the_knobs_change_no_output(binary, tmp_path):
    env = {"ABG_SG_STACK_DEPTH": "2", "ABG_SG_MAX_CONSTRAINTS": "1", "ABG_SG_ARENA_WORDS": "16", "ABG_SG_BATCH": "3"}
    for name in ("main.v", "ladder7.adj_v", "fan.adj_v", "loop.adj_v"):
        case = next(c for c in sgg.cases() if c["name"] == name)
        sgg.check_case(case, sgg.run_case([binary], case, tmp_path, env=env))
