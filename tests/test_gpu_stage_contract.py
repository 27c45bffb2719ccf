"""The host contract every stage handle shares, whatever its kernels compute: what profile_get reports for the stage's kernels
and counters, that the profiling switch (or, for the two stages that always time, the reset) does what it says, what creating a
handle on a device that does not exist raises, and that closing twice is harmless.  One table of stages, the smallest workload
that launches each kernel once, and the same assertions for every row."""
import random

import numpy as np
import pytest
import torch

from abyss_amd import _lib, api

pytestmark = pytest.mark.gpu

UNKNOWN = "no_such_kernel"


def _seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _three_seqs():
    rng = random.Random(11)
    return api.concat_seqs([_seq(rng, 100) for _ in range(3)])


def run_rr(f):
    buf, off = _three_seqs()
    f.insert(buf, off, 100)
    f.contains(buf, off)
    f.popcount()


def run_kn(f):
    buf, off = _three_seqs()
    f.load(buf, off)
    f.contains(buf, off)
    f.popcount()


def run_fm(f):
    rng = random.Random(12)
    text = _seq(rng, 2000)
    f.build(text)
    buf, off = api.concat_seqs([text[a:a + 50] for a in (0, 400, 901, 1950)])
    f.map(buf, off, 20)


def run_de(d):
    pmf = np.full(200, 1.0 / 200)
    d.set_pmf(pmf, 1.0 / 200, 99.5)
    jobs = np.array([(0, 49, 100, 200), (10, 57, 150, 150)], dtype=api.DE_JOB)
    d.scan(jobs, np.array([40, 60, 80, 50, 70], dtype=np.int32), np.array([1, 2, 1, 3, 1], dtype=np.uint32),
           np.array([0, 3, 5], dtype=np.uint64))


def run_ov(o):
    rng = random.Random(13)
    a = _seq(rng, 200)
    b = a[-30:] + _seq(rng, 170)  # the last 30 bytes of a are the first 30 of b
    o.set_contigs([a, b, _seq(rng, 200), _seq(rng, 200)])
    top, n = o.find(np.array([(0, 2)], dtype=np.uint32))
    assert n[0] >= 1 and top[0, 0] == 30


def run_sg(s):
    s.set_graph([0, 1, 2, 3, 4, 5, 5], [100] * 6, [1, 2, 3, 4, 5], [-10] * 5)  # 0 -> 1 -> ... -> 5
    s.search([(0, [(3, 1000)])])


def run_mc(m):
    rng = random.Random(14)
    g = _seq(rng, 140)
    m.set_contigs([g[0:60], g[40:100], g[80:140]])  # consecutive contigs share 20 bytes
    seqs, _, redone, _ = m.merge(25, [([0, 2, 4], [0, 20, 20])])
    assert seqs == [g] and not redone.any()


def run_pb(b):
    b.tune(batch=1)
    b.align([(b"A", b"A")] * 70)


def run_mp(p):
    rng = random.Random(15)
    p.tune(batch=1)
    p.align([(_seq(rng, 40), _seq(rng, 40)) for _ in range(70)])


class Stage:
    def __init__(self, name, cls, args, run, kernels, counters=(), exact=()):
        self.name, self.cls, self.args, self.run, self.kernels, self.counters, self.exact = name, cls, args, run, kernels, counters, exact
        self.switched = hasattr(cls, "profile")
        self.prefix = "abg_" + name

    def make(self, **kw):
        return self.cls(*self.args, **kw)


STAGES = [
    Stage("rr", api.ReadFilter, (1 << 20, 32, 3), run_rr, ("rr_insert", "rr_contains", "rr_popcount")),
    Stage("kn", api.KonnectorBloom, (32, 8 << 20), run_kn, ("kn_pack", "kn_insert", "kn_contains", "kn_popcount")),
    Stage("fm", api.FMIndex, (), run_fm, ("fm_sa", "fm_occ", "fm_map"), ("fm_map_steps",)),
    Stage("de", api.DistanceMLE, (), run_de, ("de_scan",), ("de_scan_terms",)),
    Stage("ov", api.ContigOverlap, (), run_ov, ("ov_rc", "ov_search"), ("ov_search_bytes",)),
    Stage("sg", api.PathSearch, (), run_sg, ("sg_search",)),
    Stage("mc", api.PathMerge, (), run_mc, ("mc_junction", "mc_splice"), ("mc_bytes",)),
    # always on, a launch a pair: 70 launches cross the drain at 64 pending event pairs
    Stage("pb", api.BubbleAlign, (), run_pb, ("pb_lane",), ("pb_cells",), (("pb_lane", 70), ("pb_launches", 70))),
    Stage("mp", api.PairMerge, (), run_mp, ("mp_wave",), ("mp_cells",), (("mp_wave", 70), ("mp_launches", 70))),
]
stages = pytest.mark.parametrize("st", STAGES, ids=lambda s: s.name)


def snapshot(h, st):
    return {k: h.profile_get(k) for k in st.kernels}


@stages
def test_kernels_and_counters_are_reported(st):
    h = st.make()
    try:
        if st.switched:
            st.run(h)  # before the first profile(True): nothing is recorded
            assert snapshot(h, st) == {k: (0.0, 0) for k in st.kernels}
            h.profile(True)
        st.run(h)
        for k in st.kernels:
            ms, launches = h.profile_get(k)
            assert launches >= 1 and ms > 0, (k, ms, launches)
        for c in st.counters:
            assert h.profile_get(c)[1] >= 1, c
        for name, n in st.exact:
            assert h.profile_get(name)[1] == n, name
        assert h.profile_get(UNKNOWN) == (0.0, 0)
    finally:
        h.close()


@stages
def test_the_switch_or_the_reset(st):
    h = st.make()
    try:
        if st.switched:
            h.profile(True)
            st.run(h)
            h.profile(False)
            before = snapshot(h, st)
            st.run(h)  # switched off: not one launch more, not a microsecond
            assert snapshot(h, st) == before
            h.profile(True)
            st.run(h)
            after = snapshot(h, st)
            for k in st.kernels:
                assert after[k][1] > before[k][1] and after[k][0] > before[k][0], k
        else:
            st.run(h)
            before = snapshot(h, st)
            st.run(h)
            after = snapshot(h, st)
            for k in st.kernels:
                assert after[k][1] == 2 * before[k][1] and after[k][0] > before[k][0], k
            h.profile_reset()
            for name in st.kernels + st.counters + tuple(n for n, _ in st.exact) + (UNKNOWN,):
                assert h.profile_get(name) == (0.0, 0), name
            st.run(h)  # and it counts from zero again
            for name, n in st.exact:
                assert h.profile_get(name)[1] == n, name
    finally:
        h.close()


def test_path_search_counts_steps_only_when_asked():
    s = api.PathSearch()
    try:
        s.profile(True)
        run_sg(s)
        assert s.profile_get("sg_search")[1] >= 1 and s.profile_get("sg_steps") == (0.0, 0)
        s.profile(True, count_steps=True)
        run_sg(s)
        assert s.profile_get("sg_steps")[1] >= 1
    finally:
        s.close()


@stages
def test_a_device_that_does_not_exist(st):
    with pytest.raises(api.AbyssAmdError) as e:
        st.make(device=torch.cuda.device_count())
    assert "%s_create failed (%d)" % (st.prefix, _lib.ABG_ENODEV) in str(e.value)
    assert "HIP device ordinal out of range" in str(e.value)


def test_bad_parameters_come_before_the_device():
    with pytest.raises(api.AbyssAmdError) as e:
        api.KonnectorBloom(0, 8 << 20, device=torch.cuda.device_count())
    assert "abg_kn_create failed (%d)" % _lib.ABG_EINVAL in str(e.value)
    assert "bad filter size, level count, k (1..192) or window" in str(e.value)
    with pytest.raises(api.AbyssAmdError) as e:
        api.ReadFilter(1 << 20, 0, device=torch.cuda.device_count())
    assert "abg_rr_create failed (%d)" % _lib.ABG_EINVAL in str(e.value)
    assert "bad filter size, hash count or r" in str(e.value)


@stages
def test_close_twice(st):
    h = st.make()
    h.close()
    h.close()
    h.__del__()  # a closed object's __del__ does nothing
    assert not h._h
