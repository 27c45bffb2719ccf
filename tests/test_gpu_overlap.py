"""Overlap and api.ContigOverlap on the GPU.  The search must equal the plain-Python restatement on the small shapes in both modes,
twice in a row and with ABG_OV_BATCH_PAIRS set to hit the batch seams; find(t, h) must equal find(h^, t^); and the binary must write
every golden case byte for byte (tests/golden/overlap, from the unmodified reference) at the default batch and at one pair a batch."""
import os

import numpy as np
import pytest

from abyss_amd import api, build
import overlap_golden as og

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def binary():
    build.build_cli()
    return os.path.join(build.BIN_DIR, "Overlap")


@pytest.fixture(scope="module")
def restated():
    return {g.name: g.expected() for g in og.small_shapes()}


def assert_equal(co, pairs, want, labels):
    top, n = co.find(pairs)
    lengths, off = co.find(pairs, all=True)
    for i, (w, label) in enumerate(zip(want, labels)):
        assert lengths[int(off[i]):int(off[i + 1])].tolist() == w, label
        assert int(n[i]) == min(3, len(w)) and top[i].tolist() == (w[:3] + [0, 0, 0])[:3], label


@pytest.mark.parametrize("group", og.small_shapes(), ids=lambda g: g.name)
def test_find_equals_the_restatement(group, restated):
    co = api.ContigOverlap()
    try:
        co.set_contigs(group.raw())  # (lower case is folded by set_contigs)
        assert_equal(co, group.pairs, restated[group.name], group.labels)
        assert_equal(co, group.pairs, restated[group.name], group.labels)  # twice in a row
    finally:
        co.close()


@pytest.mark.parametrize("batch", ["1", "2", "7"])
@pytest.mark.parametrize("group", og.small_shapes(), ids=lambda g: g.name)
def test_find_across_batch_seams(group, batch, restated, monkeypatch):
    monkeypatch.setenv("ABG_OV_BATCH_PAIRS", batch)
    co = api.ContigOverlap()
    try:
        co.set_contigs(group.raw())
        assert_equal(co, group.pairs, restated[group.name], group.labels)
    finally:
        co.close()


@pytest.mark.parametrize("group", og.small_shapes(), ids=lambda g: g.name)
def test_a_pair_and_its_complement_match_alike(group, restated):
    co = api.ContigOverlap()
    try:
        co.set_contigs(group.raw())
        flipped = [(h ^ 1, t ^ 1) for t, h in group.pairs]
        assert_equal(co, flipped, restated[group.name], group.labels)
    finally:
        co.close()


def test_empty_calls_and_bad_input():
    co = api.ContigOverlap()
    try:
        co.set_contigs([b"ACGT", b"GTAC"])
        top, n = co.find(np.zeros((0, 2), dtype=np.uint32))
        assert top.shape == (0, 3) and len(n) == 0
        lengths, off = co.find(np.zeros((0, 2), dtype=np.uint32), all=True)
        assert len(lengths) == 0 and off.tolist() == [0]
        assert co.find([(0, 2)], all=True)[0].tolist() == [2]
        with pytest.raises(api.AbyssAmdError, match="no such contig"):
            co.find([(0, 4)])
        with pytest.raises(api.AbyssAmdError, match="contig 1: unexpected character 0x58 at position 2"):
            co.set_contigs([b"ACGT", b"GTXC"])
    finally:
        co.close()


@pytest.mark.parametrize("mode", ["default", "one_pair_a_batch"])
@pytest.mark.parametrize("case", og.cases(), ids=lambda c: c["name"])
def test_binary_writes_what_the_reference_wrote(case, mode, binary, tmp_path):
    env = {"ABG_OV_BATCH_PAIRS": "1"} if mode == "one_pair_a_batch" else {}
    og.check_case(case, og.run_case([binary], case, tmp_path, env=env), [binary])
