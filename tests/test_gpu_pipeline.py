"""abyss-map, DistanceEst and Overlap chained on the GPU, against the unmodified reference run live (oracle/_ref; tests/pipeline_cases.py
has the inputs, the chain and the conditions asserted on the reference's own output).  First the live reference must write committed
goldens, which ties its build flags to them.  Then every program of ours runs on the reference's upstream files, so that a difference
names its stage; then ours run from the top, each stage on what the one before it wrote, and every intermediate file must equal the
reference chain's; then the library entry points take the same shapes.  Every binary is a fresh process with a time limit, one at a
time; the reference chain of an input runs once per module."""
import subprocess

import numpy as np
import pytest

from abyss_amd import api, build
import distanceest_golden as dg
import map_golden as mg
import overlap_golden as og
import pipeline_cases as pc
from test_pipeline_host import CHAINED, map_ref, ref  # noqa: F401  (module-scoped fixtures: one reference run per input here too)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.have_ref(), reason="oracle/_ref not built (make -C oracle ref)")]

REPETITIVE = ["repeats"] + [str(n) for n in pc.WIDTHS]


@pytest.fixture(scope="module")
def gpu():
    build.build_cli()
    return pc.tools("gpu")


@pytest.fixture(scope="module")
def de_check():
    build.build_hostcheck()
    return build.DE_CHECK


def subdir(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return d


# ---- the live reference is the one that wrote the goldens

@pytest.mark.parametrize("what", ["map", "index", "distanceest", "overlap"])
def test_live_reference_writes_the_goldens(what, tmp_path):
    pc.check_reference_writes_golden(what, tmp_path)


# ---- stage by stage, on the reference's upstream files

@pytest.mark.parametrize("name", CHAINED)
def test_index_files_of_the_chain_targets(name, ref, gpu, tmp_path):  # noqa: F811
    r = ref(name)
    pc.check_index(gpu, tmp_path, r.inp.target, pc.read(r.d, r.inp.target), r.fm, r.fai)


@pytest.mark.parametrize("name", REPETITIVE)
def test_index_files_of_repetitive_targets(name, map_ref, gpu, tmp_path):  # noqa: F811
    r = map_ref(name)
    pc.check_index(gpu, tmp_path, r.inp.target, r.inp.files[r.inp.target], r.fm, r.fai)


@pytest.mark.parametrize("name", CHAINED + ["repeats"])
def test_map_on_the_reference_contigs(name, ref, map_ref, gpu, tmp_path):  # noqa: F811
    r = map_ref(name) if name == "repeats" else ref(name)
    pc.check_map(gpu, r, subdir(tmp_path, "j1"))
    pc.check_map(gpu, r, subdir(tmp_path, "j16"), j=16, env={"ABG_MAP_BLOCK_READS": "7"})  # blocks of 7 reads, formatted on 16 threads


@pytest.mark.parametrize("name", CHAINED)
def test_distanceest_on_the_reference_sam(name, ref, gpu, tmp_path):  # noqa: F811
    pc.check_distance(gpu, ref(name), subdir(tmp_path, "default"))
    pc.check_distance(gpu, ref(name), subdir(tmp_path, "one_job_a_batch"), env={"ABG_DE_BATCH_THETAS": "1"})


@pytest.mark.parametrize("name", CHAINED)
def test_overlap_on_the_reference_estimates(name, ref, gpu, tmp_path):  # noqa: F811
    pc.check_overlap(gpu, ref(name), subdir(tmp_path, "default"))
    pc.check_overlap(gpu, ref(name), subdir(tmp_path, "one_pair_a_batch"), env={"ABG_OV_BATCH_PAIRS": "1"})


# ---- the chain

@pytest.mark.parametrize("name", CHAINED)
def test_chain_from_the_top(name, ref, gpu, tmp_path):  # noqa: F811
    """`asm` from the reads (our abyss-bloom-dbg and AdjList first), `cut` from the contigs; the reference's abyss-fixmate and sort in
    between: unitigs, .adj, SAM, .hist, .dist, out.fa and out.adj, the first that differs reported"""
    pc.check_chain(gpu, ref(name), tmp_path, from_reads=True)


# ---- the API at the same shapes

@pytest.mark.parametrize("name", REPETITIVE)
def test_export_equals_the_live_reference_index(name, map_ref):  # noqa: F811
    """the SA at the file's sample period and the whole BWT, on texts whose doubling rounds go on at rank keys of 16, 17 and 18 bits"""
    r = map_ref(name)
    text = r.inp.files[r.inp.target]
    if name == "repeats":
        repeat = 30000
        first = text.split(b"\n")[1]
        assert len(first) == repeat and text.count(first) == 2 and pc.key_bits(len(text)) == 18
    else:
        repeat = pc.BLOCK
        first = text.split(b"\n")[1]
        assert len(first) == repeat and text.count(first) == 2
        assert pc.key_bits(len(text)) == {65534: 16, 65535: 17, 65536: 17, 131071: 18, 131072: 18}[len(text)]
    # (fm_sa counts builds, not rounds: that many rounds ran follows from the text, whose two equal blocks no shorter key tells apart)
    assert pc.doubling_rounds(repeat) >= 7
    fm = api.FMIndex()
    try:
        fm.profile(True)
        fm.build(text)
        assert fm.size() == len(text) and fm.profile_get("fm_sa")[1] == 1
        sa, bwt = fm.export()
    finally:
        fm.close()
    period, want_sa, want_bwt = mg.parse_fm(r.fm)
    assert sa[0] == len(text) and np.array_equal(np.sort(sa), np.arange(len(text) + 1, dtype=np.uint32))
    assert np.array_equal(sa[::period].astype(np.uint64), want_sa)
    assert np.array_equal(bwt, want_bwt)


def test_contig_overlap_on_the_unitigs_and_their_estimates(ref):  # noqa: F811
    """every estimate pair of the reference's lib.dist, as Overlap would search it and as its complement: find() and find(all=True)
    against the plain restatement on the oriented strings"""
    r = ref("asm")
    lines = r.files["unitigs.fa"].split(b"\n")
    names, seqs = [ln[1:].split()[0].decode() for ln in lines[0:-1:2]], lines[1::2]
    index = {n: i for i, n in enumerate(names)}
    pairs = []
    for rec, mate, _, _, side in pc.estimates(r.files["lib.dist"]):
        a, b = 2 * index[rec], 2 * index[mate[:-1]] + (mate[-1] == "-")
        t, h = (a, b) if side == 0 else (b, a)  # (Overlap.cpp:338-340)
        pairs += [(t, h), (h ^ 1, t ^ 1)]
    assert len(pairs) >= 200 and len(set(pairs)) < len(pairs)  # (a junction is seen from both its contigs: pairs come twice)

    def oriented(node):
        return mg.revcomp(seqs[node >> 1]) if node & 1 else seqs[node >> 1]
    want = [og.py_find(oriented(t), oriented(h)) for t, h in pairs]
    assert sum(1 for w in want if w) >= 20 and any(not w for w in want)
    co = api.ContigOverlap()
    try:
        co.set_contigs(seqs)
        top, n = co.find(pairs)
        lengths, off = co.find(pairs, all=True)
    finally:
        co.close()
    for i, w in enumerate(want):
        assert lengths[int(off[i]):int(off[i + 1])].tolist() == w, pairs[i]
        assert int(n[i]) == min(3, len(w)) and top[i].tolist() == (w[:3] + [0, 0, 0])[:3], pairs[i]


def test_distance_mle_on_the_unitig_alignments(ref, de_check, tmp_path):  # noqa: F811
    """d and n of every estimate the reference made on the `asm` alignments, printed or (below -n) only warned about under -v -v"""
    r = ref("asm")
    r.stage_dir(tmp_path, ["lib.sam", "lib.hist"])
    args = pc.DE_ARGS + ["-v", "-v", "--dot", "lib.hist"]
    sam = pc.read(tmp_path, "lib.sam")
    live = pc.run(r.t["DistanceEst"], args, tmp_path, stdin=sam)
    want = dg.parse_dot(live.stdout.decode(), live.stderr.decode())
    jf = str(tmp_path / "jobs")
    d = subprocess.run([de_check, "dump", jf] + args, cwd=str(tmp_path), input=sam, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=pc.TIMEOUT)
    assert d.returncode == 0, d.stderr
    jobs = dg.read_jobs(jf)
    assert len(want) >= 100 and sorted(jobs["labels"]) == sorted(want)  # no estimate is left out
    mle = api.DistanceMLE()
    try:
        mle.set_pmf(jobs["pmf"], jobs["minp"], jobs["mean"])
        dist, n = mle.estimate(jobs["pairs"], jobs["samples"], jobs["sample_offsets"])
    finally:
        mle.close()
    assert [(int(a), int(b)) for a, b in zip(dist, n)] == [want[l] for l in jobs["labels"]]
