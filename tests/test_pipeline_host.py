"""abyss-map, DistanceEst and Overlap chained, without a GPU: tests/pipeline_cases.py runs the unmodified reference (oracle/_ref) live
on seeded inputs, and the hostcheck stand-ins (fm_check map|index, de_check run, ov_check run, adjlist_check) stage by stage on the
reference's upstream files and then as a chain in which each stage reads what the one before it wrote.  test_gpu_pipeline.py is the
same with the GPU binaries."""
import pytest

from abyss_amd import build
import pipeline_cases as pc

pytestmark = pytest.mark.skipif(not pc.have_ref(), reason="oracle/_ref not built (make -C oracle ref)")

CHAINED = ["cut1", "cut2", "asm"]


@pytest.fixture(scope="module")
def host():
    build.build_hostcheck()
    return pc.tools("host")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the reference chain of an input, run once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = pc.Reference(name, tmp_path_factory.mktemp("ref_" + name))
        return made[name]
    return get


@pytest.fixture(scope="module")
def map_ref(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            inp = pc.repeats() if name == "repeats" else pc.width(int(name))
            made[name] = pc.MapReference(inp, tmp_path_factory.mktemp("mapref_" + name))
        return made[name]
    return get


@pytest.mark.parametrize("what", ["map", "index", "distanceest", "overlap"])
def test_live_reference_writes_the_goldens(what, tmp_path):
    pc.check_reference_writes_golden(what, tmp_path)


def test_inputs_are_what_they_claim(ref, map_ref):
    """(the conditions on the reference's output are asserted where it is run: Reference.check, MapReference)"""
    assert [pc.key_bits(n) for n in pc.WIDTHS] == [16, 17, 17, 18, 18]
    assert pc.doubling_rounds(pc.BLOCK) >= 7
    for n in pc.WIDTHS:
        assert len(pc.width(n).files["w.fa"]) == n
    assert 130000 <= len(pc.repeats().files["target.fa"]) <= 136000
    r = ref("asm")
    lengths = [len(s) for s in r.files["unitigs.fa"].split(b"\n")[1::2]]
    assert len(lengths) >= 150 and max(lengths) > 20 * min(lengths)  # hundreds of unitigs of very unequal length
    assert map_ref("repeats").unmapped == 0


@pytest.mark.parametrize("name", CHAINED)
def test_index_files_of_the_chain_targets(name, ref, host, tmp_path):
    r = ref(name)
    pc.check_index(host, tmp_path, r.inp.target, pc.read(r.d, r.inp.target), r.fm, r.fai)


@pytest.mark.parametrize("name", ["repeats"] + [str(n) for n in pc.WIDTHS])
def test_index_files_of_repetitive_targets(name, map_ref, host, tmp_path):
    r = map_ref(name)
    pc.check_index(host, tmp_path, r.inp.target, r.inp.files[r.inp.target], r.fm, r.fai)


@pytest.mark.parametrize("name", CHAINED + ["repeats"])
def test_map_on_the_reference_contigs(name, ref, map_ref, host, tmp_path, monkeypatch):
    r = map_ref(name) if name == "repeats" else ref(name)
    pc.check_map(host, r, tmp_path)
    monkeypatch.setenv("ABG_MAP_BLOCK_READS", "7")
    pc.check_map(host, r, tmp_path, j=16)


@pytest.mark.parametrize("name", CHAINED)
def test_distanceest_on_the_reference_sam(name, ref, host, tmp_path):
    pc.check_distance(host, ref(name), tmp_path)


@pytest.mark.parametrize("name", CHAINED)
def test_overlap_on_the_reference_estimates(name, ref, host, tmp_path):
    pc.check_overlap(host, ref(name), tmp_path)


@pytest.mark.parametrize("name", CHAINED)
def test_chain_from_the_contigs(name, ref, host, tmp_path):
    """every stage on what the stage before it wrote (the unitigs of `asm` are the reference's: no stand-in assembles reads)"""
    pc.check_chain(host, ref(name), tmp_path, from_reads=False)
