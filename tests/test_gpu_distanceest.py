"""DistanceEst and api.DistanceMLE on the GPU.  The scan's arrays (c, L and n per theta) must equal a serial evaluation bit for bit:
against the plain-Python restatement on the small shapes, and against tests/hostcheck/de_check on the jobs of the `wide` golden
case (a PMF too long for LDS) and of `fr_basic`.  The binary must write every golden case byte for byte (tests/golden/distanceest,
from the unmodified reference at -j1), with the default batch and with ABG_DE_BATCH_THETAS set to hit the batch seams.  A build of
abg_de.hip that contracts pmf[i] * w into the add fails the bit comparisons."""
import os
import subprocess

import numpy as np
import pytest

from abyss_amd import api, build
import distanceest_golden as dg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def de_check():
    build.build_hostcheck()
    return build.DE_CHECK


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "DistanceEst")


@pytest.fixture(scope="module")
def mle():
    m = api.DistanceMLE()
    yield m
    m.close()


@pytest.fixture(scope="module")
def restated():
    return {g[0]: dg.py_scan(g[1], g[2], g[4], g[5], g[6], g[7]) for g in dg.small_shapes()}


@pytest.fixture(scope="module")
def dumps(de_check, tmp_path_factory):
    """the contig pairs of a golden input as de_check saw them, with its own serial scan of them: computed once per input"""
    made = {}

    def get(name):
        if name not in made:
            case = next(c for c in dg.cases() if c["name"] == name)
            d = tmp_path_factory.mktemp("dump")
            jf = str(d / "jobs")
            status, out, err, _ = dg.run_case([de_check, "dump", jf], case, d)
            assert status == 0, err
            jobs = dg.read_jobs(jf)
            subprocess.run([de_check, "scan", jf, jf + ".scan"], check=True, timeout=120)
            made[name] = (case, jobs, dg.read_scan(jf + ".scan", jobs["jobs"]), out, err)
        return made[name]
    return get


def assert_same(got, want):
    for g, w, what in zip(got, want, ("c", "L", "n")):
        assert dg.same_bits(g, w), what


@pytest.mark.parametrize("group", dg.small_shapes(), ids=lambda g: g[0])
def test_scan_equals_the_restatement_bit_for_bit(group, restated, mle):
    name, pmf, minp, mean, jobs, values, counts, offsets = group
    mle.set_pmf(np.array(pmf), minp, mean)
    got = mle.scan(jobs, values, counts, offsets)
    assert_same(got, restated[name])
    assert_same(mle.scan(jobs, values, counts, offsets), got)  # twice in a row: the same bits
    try:
        for block in (64, 128, 192):  # the tuning entry point changes no bit
            mle.tune(block)
            assert_same(mle.scan(jobs, values, counts, offsets), got)
    finally:
        mle.tune(0)


@pytest.mark.parametrize("name", ["wide.v", "fr_basic.dist"])
def test_scan_equals_de_check_on_golden_jobs(name, dumps, mle):
    case, jobs, want, _, _ = dumps(name)
    assert len(jobs["jobs"]) >= 2
    if name == "wide.v":
        assert len(jobs["pmf"]) > 20480  # the PMF that does not fit in LDS
    mle.set_pmf(jobs["pmf"], jobs["minp"], jobs["mean"])
    assert_same(mle.scan(jobs["jobs"], jobs["values"], jobs["counts"], jobs["offsets"]), want)


def test_scan_across_batch_seams(dumps, monkeypatch):
    """one job a batch, and batches of a few jobs: the same bits as one batch"""
    _, jobs, want, _, _ = dumps("fr_basic.dist")
    for cap in ("1", str(3 * max(dg.thetas(jobs["jobs"])))):
        monkeypatch.setenv("ABG_DE_BATCH_THETAS", cap)
        m = api.DistanceMLE()
        try:
            m.set_pmf(jobs["pmf"], jobs["minp"], jobs["mean"])
            assert_same(m.scan(jobs["jobs"], jobs["values"], jobs["counts"], jobs["offsets"]), want)
        finally:
            m.close()


@pytest.mark.parametrize("name", ["fr_basic.vv_dot", "rf_matepair.vv_dot", "short_frag.vv_dot"])
def test_estimate_equals_every_reference_estimate(name, dumps, mle, monkeypatch):
    """d= and n= of every estimate the reference made, printed or (below -n) only warned about under -v -v"""
    case, jobs, _, out, err = dumps(name)
    want = dg.parse_dot(dg.golden(case["stdout"]).decode(), case["stderr"])
    assert len(want) >= 10 and sorted(jobs["labels"]) == sorted(want)  # no estimate is left out
    mle.set_pmf(jobs["pmf"], jobs["minp"], jobs["mean"])
    d, n = mle.estimate(jobs["pairs"], jobs["samples"], jobs["sample_offsets"])
    assert [(int(a), int(b)) for a, b in zip(d, n)] == [want[l] for l in jobs["labels"]]
    monkeypatch.setenv("ABG_DE_BATCH_THETAS", "1")  # the tail of batch b beside the scan of batch b + 1, every job its own batch
    m = api.DistanceMLE()
    try:
        m.set_pmf(jobs["pmf"], jobs["minp"], jobs["mean"])
        d1, n1 = m.estimate(jobs["pairs"], jobs["samples"], jobs["sample_offsets"])
    finally:
        m.close()
    assert np.array_equal(d, d1) and np.array_equal(n, n1)


def test_empty_calls_return_cleanly(mle):
    mle.set_pmf(np.array([0.25, 0.5, 0.25]), 0.25, 1.0)
    none = np.zeros(0, dtype=dg.JOB)
    c, like, n = mle.scan(none, [], [], [0])
    assert len(c) == len(like) == len(n) == 0
    jobs = np.array([(5, 4, 3, 3), (0, 1, 2, 3), (7, -9, 1, 1)], dtype=dg.JOB)  # empty, two thetas, empty
    c, like, n = mle.scan(jobs, [1, 2], [1, 1], [0, 0, 2, 2])
    assert len(c) == 2
    assert_same((c, like, n), dg.py_scan([0.25, 0.5, 0.25], 0.25, jobs, [1, 2], [1, 1], [0, 0, 2, 2]))
    d, n = mle.estimate(np.zeros(0, dtype=dg.PAIR), [], [0])
    assert len(d) == len(n) == 0
    with pytest.raises(api.AbyssAmdError, match="pair 0"):  # where the reference asserts, an error code and the reason
        mle.estimate(np.array([(5, 5, 100, 100, 1, 1)], dtype=dg.PAIR), [3], [0, 1])


def boundary_cap(jobs):
    """the thetas of the jobs of the first target, so that the first batch ends where the next target begins"""
    t = dg.thetas(jobs["jobs"])
    first = jobs["labels"][0].split()[0][:-1]
    k = next(i for i, l in enumerate(jobs["labels"]) if l.split()[0][:-1] != first)
    return sum(t[:k]), k


@pytest.mark.parametrize("mode", ["default", "one_job_a_batch"])
@pytest.mark.parametrize("case", dg.cases(), ids=lambda c: c["name"])
def test_binary_writes_what_the_reference_wrote(case, mode, binary, tmp_path):
    env = {"ABG_DE_BATCH_THETAS": "1"} if mode == "one_job_a_batch" else {}
    dg.check_case(case, dg.run_case([binary], case, tmp_path, env=env))


# the runs that estimate pairs of more than one target (`wide` has one job a target: one_job_a_batch cuts it at every target; with
# the orientation forced against the library nothing reaches the estimator)
SEAM_CASES = [c for c in dg.cases() if dg.is_mle(c) and not c["name"].startswith("error.") and c["input"] != "wide" and "forced" not in c["name"]]


@pytest.mark.parametrize("case", SEAM_CASES, ids=lambda c: c["name"])
def test_binary_with_a_batch_that_ends_on_a_target_boundary(case, binary, dumps, tmp_path):
    _, jobs, _, _, _ = dumps(case["name"])
    cap, k = boundary_cap(jobs)
    assert 0 < k < len(jobs["labels"]) and cap > 0
    dg.check_case(case, dg.run_case([binary], case, tmp_path, env={"ABG_DE_BATCH_THETAS": str(cap)}))
