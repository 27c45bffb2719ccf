"""How many of PASS 1's `lead` stores the implicit rule leaves out (TileEnv::lead_implicit, abg_engine.h), counted where one thread
runs the kernels' logic: the host-check build, which prints the judges' two counters when ABG_LEAD_COUNT is set.

The read set is the benchmark's recipe at a size a CPU gets through: 50x coverage, 0.5 % substitution errors, 2x150 bp, k = 64,
four hash functions, a filter of 71.6 counters per genome base (configs[1]: 2^31 counters for 30 Mbp), and the engine's own batch
size, at which a bin of 2^15 counters sees 2^11 pairs of a batch.

usage: python tools/count_lead_stores.py [--genome 400000]"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(root)r + "/tests", %(root)r + "/oracle"]
import numpy as np
from abyss_amd import api, synth
from test_hostcheck import HostCheck
genome = %(genome)d
m1, m2 = synth.make_read_set(genome, 50.0, read_len=150, err=0.005)
buf, off = api.matrix_to_seqs(synth.codes_to_ascii(np.concatenate([m1, m2])))
counters = int(genome * 71.6) // 8 * 8
hc = HostCheck(64, counters, num_hashes=4, insert_batch=0, claim_log2=20)
hc.load(buf, off)
st = hc.stats()
print("ops", st["tiled_ops"], "pending", st["tiled_pending"], "overflows", st["tile_overflows"], "counters", counters)
del hc
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=400000)
    a = ap.parse_args()
    out = {}
    for knob in ("1", "0"):
        env = dict(os.environ, ABG_LEAD_COUNT="1", ABG_LEAD_IMPLICIT=knob)
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "genome": a.genome}], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            return 1
        m = re.search(r"lead_stores made=(\d+) skipped=(\d+)", r.stderr)
        out[knob] = (int(m.group(1)), int(m.group(2)), r.stdout.strip())
    made, skipped, line = out["1"]
    print(line)
    print("explicit: %d stores" % out["0"][0])
    print("implicit: %d stores made, %d left out (%.1f %% of %d)" % (made, skipped, 100.0 * skipped / (made + skipped), made + skipped))
    assert out["0"] == (made + skipped, 0, line), out
    return 0


if __name__ == "__main__":
    sys.exit(main())
