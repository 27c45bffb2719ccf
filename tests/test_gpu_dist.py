"""The partitioned multi-GPU path on a real MI355X (a box with ONE GPU), in worker processes
(tests/dist_gpu_worker.py) that load torch first like bench.py does:

* the library's RCCL communicator with a single rank and ABG_FORCE_DIST=1 -- the partitioned
  kernels (FHashClaimT<true>, FEvalDist / FApplyDist, the hipcub compaction, the drain hand-over,
  the split classification and the merge of walk results) and every RCCL call (ncclAllReduce,
  in-place ncclAllGather) run on the device, each collective an identity;
* two and three ranks sharing the GPU, joined by gloo through host copies;
* two to eight ranks sharing the GPU on the inputs of the CPU suite's hard cases (tests/dist_cases.py: a commit that needs
  a second pass, saturating counters, tile and route overflow, kept reads, spaced seeds, routing over uneven owner ranges),
  one launch per world size.

All must reproduce the reference's single sequential run bit for bit, and exit cleanly."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_gpu_worker.py")


def result_of(r):
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    return json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_rccl_single_rank_partitioned_path_reproduces_reference_runs_and_oracle():
    env = dict(os.environ, ABG_FORCE_DIST="1")
    r = subprocess.run([sys.executable, WORKER, "rccl1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("k64", "k40_mixed", "k48_K16", "share_total", "counting_filter", "results", "contigs", "visited",
                "assembly_counters"):
        assert out[key], (key, out)
    assert out["n_contigs"] > 10
    # (round 6: the single-GPU rules on the partitioned path leave this small run's rounds nothing -- the partitioned reservation
    # rounds are exercised by the same run under round 2's rule below)
    assert all(v > 0 for nm, v in out["launches"].items() if nm != "insert_apply"), out["launches"]
    assert out["launches"]["dist_pack"] > 0 and out["launches"]["co_settle"] > 0, out["launches"]
    env["ABG_COSETTLE"] = "0"
    r = subprocess.run([sys.executable, WORKER, "rccl1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("k64", "k40_mixed", "k48_K16", "counting_filter", "results", "contigs", "visited", "assembly_counters"):
        assert out[key], (key, out)
    assert out["launches"]["insert_apply"] > 0 and out["launches"]["co_settle"] == 0, out["launches"]


def test_rccl_single_rank_routed_path_reproduces_reference_runs_and_oracle():
    """The routed form of PASS 1 (Engine::insert_tiles_routed) with the real kernels -- FRoutePack, FBinCoarseRec,
    FRouteReply / FRouteCombine / FRouteTgt, the pending records -- on one rank, each exchange a device copy."""
    env = dict(os.environ, ABG_FORCE_DIST="1", ABG_DIST_ROUTE_MIN="1")
    r = subprocess.run([sys.executable, WORKER, "rccl1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("k64", "k40_mixed", "k48_K16", "share_total", "counting_filter", "results", "contigs", "visited",
                "assembly_counters"):
        assert out[key], (key, out)
    assert out["launches"]["route_pack"] > 0 and out["launches"]["route_reply"] > 0, out["launches"]


@pytest.mark.parametrize("world,route", [(2, "0"), (3, "0"), (2, "2"), (3, "2")])
def test_ranks_sharing_one_gpu_match_oracle(world, route):
    """route "2": the (op, counter) pairs are routed to the ranks that own the counters (abg_comm::all_to_all_v, here
    through gloo on host copies); "0": the all-gather form."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", ABG_DIST_ROUTE_MIN=route)
    env.pop("ABG_FORCE_DIST", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(29700 + world), WORKER, "staged"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("counting_filter", "results", "contigs", "visited", "assembly_counters", "ranks_agree"):
        assert out[key], (key, out)
    assert out["n_contigs"] > 10
    assert out["comm_calls"]["all_reduce"] > 0
    assert (out["comm_calls"].get("all_to_all_v", 0) > 0) == (route != "0"), out["comm_calls"]


@pytest.mark.parametrize("world,route", [(2, "0"), (3, "2")])
def test_sliced_filter_on_ranks_sharing_one_gpu(world, route):
    """abg_params.slice_filter (ABG_SLICE_FILTER=1): each rank allocates its own range of the counters only, PASS 2 probes the
    gathered bit plane, coverage goes through FPcCover and an all-reduce -- the real kernels, against the oracle (the counting
    filter is exported rank by rank).  The CPU twin of this test runs with the other ranks' counters unmapped
    (tests/test_dist_partition.py::test_filter_that_fits_no_single_rank)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", ABG_DIST_ROUTE_MIN=route, ABG_SLICE_FILTER="1")
    env.pop("ABG_FORCE_DIST", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(29710 + world), WORKER, "staged"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("counting_filter", "results", "contigs", "visited", "assembly_counters", "ranks_agree"):
        assert out[key], (key, out)
    assert out["n_contigs"] > 10
    assert 0 < out["stats"]["counter_bytes_held"] <= (1 << 22) // world + 128, out["stats"]


def test_rccl_single_rank_sliced_filter_reproduces_reference_runs_and_oracle():
    """The sliced filter through the library's RCCL communicator (one rank): the plane's all-gather, the coverage all-reduce and
    the rank-by-rank export are RCCL calls on the engine's stream."""
    env = dict(os.environ, ABG_FORCE_DIST="1", ABG_SLICE_FILTER="1")
    r = subprocess.run([sys.executable, WORKER, "rccl1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out = result_of(r)
    for key in ("k64", "k40_mixed", "k48_K16", "share_total", "counting_filter", "results", "contigs", "visited",
                "assembly_counters"):
        assert out[key], (key, out)
    assert out["launches"]["pc_cover"] > 0 and out["launches"]["solid_plane"] > 0 and out["held"] == (1 << 24) + 64, out


def test_bench_runs_configs4_scaled_down_on_two_ranks():
    """`bench.py --gpus N --config 4` (k=96, B=500G, 1.2 G pairs on eight GPUs) scaled down to what two ranks sharing this
    GPU can hold: a sliced filter, the reads in three chunks per pass (every chunk all-gathered), the launch path of the
    driver's multi-GPU run (ranks started by bench.py itself)."""
    env = dict(os.environ, ABG_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("ABG_FORCE_DIST", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--comm", "staged", "--slice-filter", "--chunks", "3",
                        "--config", "4", "--pairs", "300000", "--bloom", "120M", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                        "--no-end-to-end"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    c = d["config"]
    assert d["n_gpus"] == 2 and c["ranks_agree"] is True and c["chunks"] == 3 and "k=96" in c["workload"], c
    assert 0 < c["counter_bytes_per_rank"] < 0.51 * (120 << 20) / 1.125 + 4096, c
    assert c["unitigs"] > 1000 and d["value"] > 0


# ---- the CPU suite's hard cases (tests/test_dist_partition.py) with the real kernels: tests/dist_gpu_worker.py `cases` ----
# world -> the cases of its one launch, as the worker's SPECs (case[+arg][:ENV=VAL,...]; route = ABG_DIST_ROUTE_MIN)
LAUNCHES = {
    2: ["oracle:ABG_TILE_CAP=300", "oracle:ABG_TILED=0", "golden+k48_K16:route=2", "golden+s_mixed_k32_H12_kc3"],
    3: ["bigbatch:route=0", "bigbatch:route=0,ABG_PAR_COMMIT_MAX_GB=0,ABG_T_TAGS=5", "tiny_filter:route=0", "saturate", "saturate_tiled:route=2",
        "oracle:route=2,ABG_ROUTE_CAP=500", "sliced_checkpoint:ABG_SLICE_FILTER=1", "golden+s_tandem_k32"],
    # (from four ranks on the pairs are routed by default)
    4: ["oracle", "bigbatch", "tiny_filter", "saturate_tiled", "kept", "shared", "golden+k64:ABG_SLICE_FILTER=1",
        "sliced:ABG_SLICE_FILTER=1,ABG_ROUTE_CAP=64", "bigbatch:ABG_SLICE_FILTER=1,ABG_PAR_COMMIT_MAX_GB=0,ABG_T_TAGS=5"],
    5: ["tiny_filter", "golden+s_mixed_k40_H6", "shared"],
    8: ["golden+k32", "bigbatch", "sliced+shared:ABG_SLICE_FILTER=1"],
}
# seconds a launch may take: five times its first passing run on an MI355X, at least 120.  Those runs took 4.9, 6.6, 10.6, 6.4 and
# 9.0 s on 2, 3, 4, 5 and 8 ranks and 4.8 s for the selftest (notes/README.md has the cases' figures): 120 everywhere
LAUNCH_TIMEOUT = {2: 120, 3: 120, 4: 120, 5: 120, 8: 120, "selftest": 120}
FAULT = []  # the note a launch leaves that timed out, ended by a signal or reported a GPU fault: nothing more is started after it
_results = {}
ILLEGAL = "an illegal memory access was encountered"


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if FAULT:
        pytest.fail("not started: an earlier launch faulted or hung (%s)" % FAULT[0])


def _launch(key, world, port, args):
    """One torch.distributed.run of the worker (at most eight ranks, one launch at a time); the parsed RESULT, cached."""
    if FAULT:
        pytest.fail("not started: an earlier launch faulted or hung (%s)" % FAULT[0])
    if key in _results:
        kind, val = _results[key]
        if kind == "error":
            pytest.fail("the launch of %s failed: %s" % (key, val))
        return val
    assert world <= 8
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    for name in ("ABG_FORCE_DIST", "ABG_DIST_ROUTE_MIN", "ABG_SLICE_FILTER"):
        env.pop(name, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER] + args
    t0 = time.time()
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=LAUNCH_TIMEOUT[key])
    except subprocess.TimeoutExpired as e:
        FAULT.append("launch %s: no end within %d s" % (key, LAUNCH_TIMEOUT[key]))
        _results[key] = ("error", FAULT[-1])
        pytest.fail(FAULT[-1] + ": " + ((e.stderr or b"").decode(errors="replace")[-2000:]))
    wall = time.time() - t0
    text = r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace")
    # (the launcher reports a rank that a signal ended as "exitcode  : -11")
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137) or ILLEGAL in text or re.search(r"exitcode\s*:\s*(-\d+|134|139|124|137)\b", text):
        FAULT.append("launch %s: status %d" % (key, r.returncode))
    if r.returncode != 0:
        _results[key] = ("error", "status %d: %s" % (r.returncode, text[-3000:]))
        pytest.fail(_results[key][1])
    out = result_of(r)
    print("launch %s: %.1f s" % (key, wall))
    for spec, v in out.items():  # (the figures notes/README.md records)
        if isinstance(v, dict):
            print("  %s: %s s, all_to_all_v %d," % (spec, v["seconds"], v["comm_calls"]["all_to_all_v"]), {n: v["stats"][n] for n in (
                "commit_rounds", "walk_rounds", "insert_rounds", "tiled_ops", "tiled_pending", "tile_overflows", "counter_bytes_held")})
    _results[key] = ("ok", out)
    return out


@pytest.fixture(scope="module")
def hard_cases():
    """world -> {SPEC: what the worker collected for it}; the launch of a world size is made when its first test asks."""
    return lambda world: _launch(world, world, 29740 + world, ["cases"] + LAUNCHES[world])


def _parse(spec):
    head, _, tail = spec.partition(":")
    name, _, arg = head.partition("+")
    env = dict(item.split("=", 1) for item in tail.split(",") if item)
    if "route" in env:
        env["ABG_DIST_ROUTE_MIN"] = env.pop("route")
    return name, arg, env


def _counters_of(name, arg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_cases
    if name == "golden":
        return json.load(open(os.path.join(ROOT, "tests", "golden", arg + ".json")))["counters"]
    if name in dist_cases.SYNTHETIC:
        return dist_cases.SYNTHETIC[name][2]
    return {"saturate": 4096, "saturate_tiled": 1 << 22, "kept": 1 << 20, "sliced_checkpoint": 1 << 19}[name]


@pytest.mark.parametrize("world,spec", [(w, s) for w in sorted(LAUNCHES) for s in LAUNCHES[w]], ids=lambda v: "w%d" % v if isinstance(v, int) else v)
def test_hard_cases_of_the_partitioned_path_with_the_real_kernels(world, spec, hard_cases):
    """The assertions of the CPU twins in tests/test_dist_partition.py (same bytes, same knobs: tests/dist_cases.py), on
    ranks that exchange data between real kernels: the 64-lane votes of the partitioned commit where their answer decides a
    second pass, atomics between workgroups, LDS tiles, kernels behind staged collectives; from four ranks on the routed
    exchange over uneven owner ranges.  Besides the verdicts, each case must have taken its path."""
    out = hard_cases(world)[spec]
    name, arg, env = _parse(spec)
    keys = ("filtered_popcount", "fasta", "readlog", "trace", "counters") if name == "golden" else \
        ("counting_filter",) if name.startswith("saturate") else ("counting_filter", "results", "contigs", "visited", "assembly_counters")
    for key in keys + ("ranks_agree",):
        assert out[key] is True, (key, out)
    st, calls = out["stats"], out["comm_calls"]
    assert calls["all_reduce"] > 0, calls
    route = env.get("ABG_DIST_ROUTE_MIN")
    if "ABG_ROUTE_CAP" in env:
        # Engine::insert_tiles_routed learns that a sender's room ran out from the all-reduce of the counts, BEFORE the first
        # exchange: a batch that falls back never calls all_to_all_v, and with a room this small every batch does (the CPU
        # twin: all_to_all_v == 0, 14 fall-backs).  That the routed pack ran is shown by the fall-backs themselves -- only it
        # reads ABG_ROUTE_CAP -- and by nothing having gone through the tiles.
        assert st["tile_overflows"] > 0 and st["tiled_ops"] == 0, st
    elif world >= 4 or route == "2":
        assert calls["all_to_all_v"] > 0, calls
    if route == "0":
        assert calls["all_to_all_v"] == 0, calls
    if name == "bigbatch":
        assert st["commit_rounds"] > st["walk_rounds"], st
        assert out["n_contigs"] > 20
    if name == "tiny_filter":
        assert st["insert_rounds"] > 20, st
    if name.startswith("saturate"):
        assert out["saturated"] == 255, out
    if name == "saturate_tiled":
        assert st["tiled_ops"] > 0 and st["tiled_pending"] > 254, st
    if "ABG_TILE_CAP" in env or "ABG_ROUTE_CAP" in env:
        assert st["tile_overflows"] > 0, st
    if env.get("ABG_TILED") == "0":
        assert st["tiled_ops"] == 0, st
    if env.get("ABG_SLICE_FILTER") == "1":
        assert 0 < st["counter_bytes_held"] <= _counters_of(name, arg) // world + 128, st
    if name in ("kept", "oracle"):
        assert out["n_contigs"] > 10


def test_communicator_selftest_on_device_buffers_world4():
    """abyss_amd.dist.selftest over StagedTorchComm with the buffers in device memory (torch tensors, moved through
    abg_dev_copy): all 10 checks on every rank.  The CPU twin only ever used host memory."""
    out = _launch("selftest", 4, 29750, ["selftest"])
    assert len(out["ranks"]) == 4
    for r in out["ranks"]:
        assert r["ok"] and r["checks"] == 10 and not r["failed"], r


def _gpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:  # noqa: BLE001
        return 0


@pytest.mark.skipif(_gpus() < 2, reason="needs two GPUs: the first real multi-rank run of the RCCL communicator")
def test_two_real_ranks_over_rccl_agree_with_one_gpu(tmp_path):
    """bench.py --gpus 2 as the driver launches it (one process per GPU, backend nccl = RCCL): the
    library's own communicator (in-place ncclAllGather, the ragged broadcast group, all_reduce per
    round) between two real ranks, against the same job on one GPU; then the host binary's --gpus 2."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ABG_FORCE_DIST", None)
    args = ["--pairs", "400000", "--bloom", "160M", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=env, timeout=900)
    assert one.returncode == 0, one.stderr.decode()[-2000:]
    a = json.loads([ln for ln in one.stdout.decode().splitlines() if ln.startswith("{")][-1])
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29731", os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--scaling", "strong"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert two.returncode == 0, two.stderr.decode()[-3000:]
    b = json.loads([ln for ln in two.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert b["n_gpus"] == 2 and b["config"]["ranks_agree"] is True and "note" not in b["config"], b["config"]
    # (the two runs draw their reads with different seeds -- every rank generates its own share -- so the
    # unitig sets are those of two samples of the same genome: close, not equal)
    assert abs(b["config"]["unitig_bp"] - a["config"]["unitig_bp"]) < 0.02 * a["config"]["unitig_bp"]
    # the drop-in binary with --gpus 2 writes the FASTA of the one-GPU run
    from abyss_amd import build, synth
    m1, m2 = synth.make_read_set(200000, 40.0)
    synth.write_fastq(str(tmp_path / "r1.fq"), m1, "r", 1)
    synth.write_fastq(str(tmp_path / "r2.fq"), m2, "r", 2)
    cli = build.build_cli()
    r1 = subprocess.run([cli, "-k32", "-q3", "-b100M", "r1.fq", "r2.fq"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r2 = subprocess.run([cli, "-k32", "-q3", "-b100M", "--gpus=2", "r1.fq", "r2.fq"], cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=600)
    assert r1.returncode == 0 and r2.returncode == 0, r2.stderr.decode()[-2000:]
    assert r1.stdout == r2.stdout and len(r1.stdout) > 100000
