"""Build helpers: compile the HIP library (product) and the checkers (test infrastructure).

The product is one shared library, ``abyss_amd/lib/libabyss_amd.so`` (plus the host binaries over its C ABI in ``abyss_amd/bin``), built in-tree with
``hipcc --offload-arch=gfx950`` from ``abyss_amd/csrc/abg_kernels.hip``; hipcc
cross-compiles without a GPU.  The checkers (``oracle/liboracle.so``, ``oracle/abg_oracle``,
``oracle/_ref/*`` when /root/reference is present, ``tests/hostcheck/libhostcheck.so``) are
only ever loaded by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abyss_amd", "csrc")
LIB = os.path.join(ROOT, "abyss_amd", "lib", "libabyss_amd.so")
BIN_DIR = os.path.join(ROOT, "abyss_amd", "bin")
ORACLE_DIR = os.path.join(ROOT, "oracle")
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck.so")
REFERENCE = "/root/reference"


def _newer(target: str, sources) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _run(cmd, cwd=None):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("build step failed: %s" % " ".join(cmd))
    return r.stdout


def hipcc() -> str:
    for c in ("hipcc", "/opt/rocm/bin/hipcc"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("hipcc not found")


def csrc_files():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [os.path.join(ROOT, "include", "abyss_amd.h")]


OBJ_DIR = os.path.join(ROOT, "abyss_amd", "lib", "obj")
# translation units of the library and what each is rebuilt for (the big one takes minutes; the others seconds)
UNITS = {
    "abg_kernels": ["abg_kernels.hip", "abg_core.h", "abg_engine.h", "abg_walk.h", "abg_host.h", "abg_overlap.h"],
    "abg_rr": ["abg_rr.hip", "abg_rr.h", "abg_core.h"],
    "abg_kn": ["abg_kn.hip", "abg_kn.h", "abg_core.h"],
    "abg_fm": ["abg_fm.hip", "abg_fm.h", "abg_core.h"],
    "abg_de": ["abg_de.hip", "abg_de.h", "abg_core.h"],
    "abg_ov": ["abg_ov.hip", "abg_ov.h", "abg_core.h"],
    "abg_sg": ["abg_sg.hip", "abg_sg.h", "abg_core.h"],
    "abg_mc": ["abg_mc.hip", "abg_mc.h", "abg_ov.h", "abg_core.h"],
    "abg_pb": ["abg_pb.hip", "abg_pb.h", "abg_mc.h", "abg_ov.h", "abg_core.h"],
    "abg_mp": ["abg_mp.hip", "abg_mp.h", "abg_mc.h", "abg_ov.h", "abg_core.h"],
}
# flags a unit adds to the common command line (abg_de: its sums must match a serial evaluation bit for bit, so no product may be
# fused into an add, on the device or in the host tail)
UNIT_FLAGS = {"abg_de": ["-ffp-contract=off"]}


def build_lib(force: bool = False) -> str:
    """libabyss_amd.so: the gfx950 kernels + C ABI, one object per translation unit."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    header = os.path.join(ROOT, "include", "abyss_amd.h")
    objs, procs = [], []
    for unit, deps in UNITS.items():
        obj = os.path.join(OBJ_DIR, unit + ".o")
        objs.append(obj)
        if force or _newer(obj, [os.path.join(CSRC, d) for d in deps] + [header]):
            cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + UNIT_FLAGS.get(unit, []) + \
                ["-c", "-o", obj, os.path.join(CSRC, unit + ".hip")]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out)
            raise RuntimeError("build step failed: %s" % " ".join(cmd))
    if force or procs or _newer(LIB, objs):
        _run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


def build_cli(force: bool = False) -> str:
    """abyss_amd/bin/abyss-bloom-dbg: the drop-in host binary (C++ over the C ABI)."""
    src = os.path.join(CSRC, "host", "bloom_dbg_main.cc")
    out = os.path.join(BIN_DIR, "abyss-bloom-dbg")
    if not os.path.exists(src):
        return ""
    deps = [src] + [os.path.join(CSRC, "host", f) for f in os.listdir(os.path.join(CSRC, "host"))]
    if force or _newer(out, deps + [LIB]):
        os.makedirs(BIN_DIR, exist_ok=True)
        build_lib()
        _run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", out, src,
              "-L" + os.path.dirname(LIB), "-labyss_amd", "-Wl,-rpath,$ORIGIN/../lib", "-lpthread"])
        _run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o",
              os.path.join(BIN_DIR, "abyss-bloom"), os.path.join(CSRC, "host", "bloom_main.cc"),
              "-L" + os.path.dirname(LIB), "-labyss_amd", "-Wl,-rpath,$ORIGIN/../lib", "-lpthread"])
        _run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o",
              os.path.join(BIN_DIR, "AdjList"), os.path.join(CSRC, "host", "adjlist_main.cc"),
              "-L" + os.path.dirname(LIB), "-labyss_amd", "-Wl,-rpath,$ORIGIN/../lib", "-lpthread"])
        _run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o",
              os.path.join(BIN_DIR, "abyss-rresolver-short"), os.path.join(CSRC, "host", "rresolver_main.cc"),
              "-L" + os.path.dirname(LIB), "-labyss_amd", "-Wl,-rpath,$ORIGIN/../lib", "-lpthread"])
        for name, main in (("abyss-map", "map_main.cc"), ("abyss-index", "index_main.cc"), ("DistanceEst", "distanceest_main.cc"),
                           ("Overlap", "overlap_main.cc"), ("SimpleGraph", "simplegraph_main.cc"), ("MergeContigs", "mergecontigs_main.cc"),
                           ("PopBubbles", "popbubbles_main.cc"), ("abyss-mergepairs", "mergepairs_main.cc")):
            _run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o",
                  os.path.join(BIN_DIR, name), os.path.join(CSRC, "host", main),
                  "-L" + os.path.dirname(LIB), "-labyss_amd", "-Wl,-rpath,$ORIGIN/../lib", "-lpthread"] +
                 (["-ffp-contract=off"] if name == "DistanceEst" else []))
    return out


def build_oracle(force: bool = False) -> None:
    """C restatement (always) and the unmodified reference (when its sources are present)."""
    targets = ["oracle"]
    if os.path.isdir(REFERENCE):
        targets.append("ref")
    if force:
        _run(["make", "-C", ORACLE_DIR, "clean"])
    _run(["make", "-C", ORACLE_DIR, "-j8"] + targets)


READER_CHECK = os.path.join(ROOT, "tests", "hostcheck", "reader_check")
ADJLIST_CHECK = os.path.join(ROOT, "tests", "hostcheck", "adjlist_check")
RRESOLVER_CHECK = os.path.join(ROOT, "tests", "hostcheck", "rresolver_check")
KN_CHECK = os.path.join(ROOT, "tests", "hostcheck", "kn_check")
FM_CHECK = os.path.join(ROOT, "tests", "hostcheck", "fm_check")
DE_CHECK = os.path.join(ROOT, "tests", "hostcheck", "de_check")
OV_CHECK = os.path.join(ROOT, "tests", "hostcheck", "ov_check")
SG_CHECK = os.path.join(ROOT, "tests", "hostcheck", "sg_check")
MC_CHECK = os.path.join(ROOT, "tests", "hostcheck", "mc_check")
PB_CHECK = os.path.join(ROOT, "tests", "hostcheck", "pb_check")
MP_CHECK = os.path.join(ROOT, "tests", "hostcheck", "mp_check")


def build_hostcheck(force: bool = False) -> str:
    # (hostcheck_ext.cc includes hostcheck.cc and adds the entry points written after it)
    src = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_ext.cc")
    if force or _newer(HOSTCHECK, [src, os.path.join(ROOT, "tests", "hostcheck", "hostcheck.cc")] + csrc_files()):
        _run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", HOSTCHECK, src])
    rsrc = os.path.join(ROOT, "tests", "hostcheck", "reader_check.cc")
    if force or _newer(READER_CHECK, [rsrc, os.path.join(CSRC, "host", "fasta_reader.h")]):
        _run(["g++", "-std=c++17", "-O2", "-o", READER_CHECK, rsrc])
    asrc = os.path.join(ROOT, "tests", "hostcheck", "adjlist_check.cc")
    if force or _newer(ADJLIST_CHECK, [asrc, HOSTCHECK, os.path.join(CSRC, "host", "adjlist_core.h"),
                                       os.path.join(CSRC, "host", "fasta_reader.h")]):
        _run(["g++", "-std=c++17", "-O2", "-o", ADJLIST_CHECK, asrc, "-L" + os.path.dirname(HOSTCHECK), "-lhostcheck",
              "-Wl,-rpath,$ORIGIN"])
    hsrc = [os.path.join(CSRC, "host", f) for f in ("rresolver_core.h", "graph_writers.h", "fasta_reader.h", "si_bytes.h")]
    csrc = os.path.join(ROOT, "tests", "hostcheck", "rresolver_check.cc")
    if force or _newer(RRESOLVER_CHECK, [csrc, os.path.join(CSRC, "abg_rr.h"), os.path.join(CSRC, "abg_core.h")] + hsrc):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", RRESOLVER_CHECK, csrc, "-lpthread"])
    ksrc = os.path.join(ROOT, "tests", "hostcheck", "kn_check.cc")
    kdeps = [ksrc] + [os.path.join(CSRC, f) for f in ("abg_kn.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("bloom_core.h", "fasta_reader.h")]
    if force or _newer(KN_CHECK, kdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", KN_CHECK, ksrc, "-lpthread"])
    fsrc = os.path.join(ROOT, "tests", "hostcheck", "fm_check.cc")
    fdeps = [fsrc] + [os.path.join(CSRC, f) for f in ("abg_fm.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("map_core.h", "fasta_reader.h")]
    if force or _newer(FM_CHECK, fdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", FM_CHECK, fsrc, "-lpthread"])
    dsrc = os.path.join(ROOT, "tests", "hostcheck", "de_check.cc")
    ddeps = [dsrc] + [os.path.join(CSRC, f) for f in ("abg_de.h", "abg_core.h")] + [os.path.join(CSRC, "host", "distanceest_core.h")]
    if force or _newer(DE_CHECK, ddeps):  # (no -march and no contraction: its sums are the reference's, bit for bit)
        _run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", DE_CHECK, dsrc, "-lpthread"])
    osrc = os.path.join(ROOT, "tests", "hostcheck", "ov_check.cc")
    odeps = [osrc] + [os.path.join(CSRC, f) for f in ("abg_ov.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("overlap_core.h", "rresolver_core.h", "graph_writers.h", "fasta_reader.h", "si_bytes.h")]
    if force or _newer(OV_CHECK, odeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OV_CHECK, osrc, "-lpthread"])
    ssrc = os.path.join(ROOT, "tests", "hostcheck", "sg_check.cc")
    sdeps = [ssrc] + [os.path.join(CSRC, f) for f in ("abg_sg.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("simplegraph_core.h", "overlap_core.h", "rresolver_core.h", "graph_writers.h", "fasta_reader.h", "si_bytes.h")]
    if force or _newer(SG_CHECK, sdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", SG_CHECK, ssrc, "-lpthread"])
    msrc = os.path.join(ROOT, "tests", "hostcheck", "mc_check.cc")
    mdeps = [msrc] + [os.path.join(CSRC, f) for f in ("abg_mc.h", "abg_ov.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("mergecontigs_core.h", "overlap_core.h", "rresolver_core.h", "graph_writers.h", "fasta_reader.h", "si_bytes.h")]
    if force or _newer(MC_CHECK, mdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", MC_CHECK, msrc, "-lpthread"])
    psrc = os.path.join(ROOT, "tests", "hostcheck", "pb_check.cc")
    pdeps = [psrc] + [os.path.join(CSRC, f) for f in ("abg_pb.h", "abg_mc.h", "abg_ov.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("popbubbles_core.h", "rresolver_core.h", "graph_writers.h", "fasta_reader.h", "si_bytes.h")]
    if force or _newer(PB_CHECK, pdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", PB_CHECK, psrc, "-lpthread"])
    qsrc = os.path.join(ROOT, "tests", "hostcheck", "mp_check.cc")
    qdeps = [qsrc] + [os.path.join(CSRC, f) for f in ("abg_mp.h", "abg_mc.h", "abg_ov.h", "abg_core.h")] + \
        [os.path.join(CSRC, "host", f) for f in ("mergepairs_core.h", "fasta_reader.h")]
    if force or _newer(MP_CHECK, qdeps):
        _run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", MP_CHECK, qsrc, "-lpthread"])
    return HOSTCHECK


def build_all(force: bool = False) -> None:
    build_lib(force)
    build_cli(force)
    build_oracle(force)
    build_hostcheck(force)


if __name__ == "__main__":
    build_all("--force" in sys.argv)
    print("built:", LIB)
