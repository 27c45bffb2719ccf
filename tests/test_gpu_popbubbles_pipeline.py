"""MergeContigs -> PopBubbles -> MergeContigs, the three rules abyss-pe runs between the unitigs' graph and the first mapping, chained on
the real unitigs of tests/pipeline_cases.py:asm() (held as asm.fa / asm.adj / asm.path in tests/golden/popbubbles): each stage's files
must be what the unmodified reference's chain wrote (chain.1.*, chain.2.*, chain.3.fa), and each stage reads what the stage before it
wrote here, not the golden.  Nothing is read from the reference tree."""
import os
import subprocess

import pytest

from abyss_amd import build
import popbubbles_golden as pbg

pytestmark = pytest.mark.gpu


def test_merge_pop_merge_on_real_unitigs(tmp_path):
    build.build_cli()
    tool = lambda name: os.path.join(build.BIN_DIR, name)
    k = "-k%d" % int(pbg.golden("chain.k"))
    for name in ("asm.fa", "asm.adj", "asm.path"):
        (tmp_path / name).write_bytes(pbg.golden(name))

    def run(argv, stdout=None):
        r = subprocess.run(argv, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr
        if stdout:
            (tmp_path / stdout).write_bytes(r.stdout)

    run([tool("MergeContigs"), k, "--adj", "-g", "chain.1.adj", "-o", "chain.1.fa", "asm.fa", "asm.adj", "asm.path"])
    run([tool("PopBubbles"), k, "-g", "chain.2.adj", "chain.1.fa", "chain.1.adj"], stdout="chain.2.path")
    run([tool("MergeContigs"), k, "-o", "chain.3.fa", "chain.1.fa", "chain.1.adj", "chain.2.path"])
    for name in ("chain.1.adj", "chain.1.fa", "chain.2.adj", "chain.2.path", "chain.3.fa"):
        assert (tmp_path / name).read_bytes() == pbg.golden(name), name
    assert pbg.golden("chain.2.path").count(b"\t") >= 5 and len(pbg.golden("chain.2.path").split(b"\t")[0].split()) >= 5  # popped contigs, then paths
