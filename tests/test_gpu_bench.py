"""bench.py on one GPU at a small size: a plain run prints the headline line without the legs that take runs of their own
(no_events, cpu_baseline, end_to_end); --full adds them on the same reads."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(*args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pairs", "200000", "--bloom", "256M"] + list(args),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])


def test_plain_run_leaves_the_other_legs_to_full():
    plain = bench_line("--steps", "2", "--warmup", "1")
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["unit"] == "Mk-mers/s" and plain["higher_is_better"] is True and plain["dtype"] == "u64"
    assert not {"no_events", "cpu_baseline", "end_to_end"} & set(plain), sorted(plain)
    # (the 3 s between the drop-in binary's runs are for its timing, not for what is checked here)
    full = bench_line("--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", env=dict(os.environ, ABG_E2E_GAP_S="0.5"))
    assert full["no_events"]["steps"] == 1 and full["no_events"]["ms_per_step"] > 0
    assert "cpu_baseline" not in full
    e2e = full["end_to_end"]
    assert e2e["rc"] == 0 and len(e2e["wall_ms_runs"]) == 3
    assert e2e["unitigs"] == full["config"]["unitigs"] == plain["config"]["unitigs"] > 100, (e2e["unitigs"], full["config"], plain["config"])
