"""Worker of tests/test_dist_partition.py: one rank of a partitioned run on the CPU.

Every rank drives a tests/hostcheck session (the product's device logic executed serially)
joined to the others by abyss_amd.dist.StagedTorchComm over gloo; rank 0 also runs the same
input through the oracle (or compares with a golden reference run) and prints one JSON line.
TEST INFRASTRUCTURE: launched with torch.distributed.run, world_size 2 or 3.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import dist_cases as cases  # noqa: E402
from abyss_amd import _lib, api, dist as adist  # noqa: E402
from test_hostcheck import HostCheck  # noqa: E402


class DistHostCheck(HostCheck):
    """The engine of tests/dist_cases.py's cases on the CPU."""

    def attach(self):
        self.comm = adist.StagedTorchComm(*adist.host_memory_io())
        if os.environ.get("ABG_TEST_OLD_COMM_ABI"):
            # a caller compiled against the header whose abg_comm ended after all_reduce: struct_size is a zeroed field there, and
            # what lies behind the struct is not a function pointer
            self.comm.struct.struct_size = 0
            self.comm.struct.all_to_all_v = adist.A2A_FN(0)
        self.l.hc_attach_comm.argtypes = [C.c_void_p, C.c_void_p]
        assert self.l.hc_attach_comm(self.h, C.byref(self.comm.struct)) == 0
        vp = C.c_void_p
        self.l.hc_share_reads.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
        self.l.hc_load_packed.argtypes = [vp, vp, vp, vp, C.c_uint64]
        self.l.hc_assemble_packed.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, _lib.CONTIG_CB, vp]

    def share(self, words, woff, lens):
        gw, go, gl, nt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert self.l.hc_share_reads(self.h, words.ctypes.data, woff.ctypes.data, lens.ctypes.data, len(lens),
                                     C.byref(gw), C.byref(go), C.byref(gl), C.byref(nt)) == 0
        return gw, go, gl, nt.value

    def load_packed(self, gw, go, gl, n):
        assert self.l.hc_load_packed(self.h, gw, go, gl, n) == 0

    def assemble_packed(self, gw, go, gl, n):
        res = np.zeros(n, dtype=np.uint8)
        out = []

        def cb(_u, c):
            c = c.contents
            out.append(api.ContigRecord(c.contig_id, c.read_index, c.seq, c.coverage, bool(c.redundant), c.left_ext,
                                        c.right_ext, c.left_code, c.right_code, c.seed_pos))
        assert self.l.hc_assemble_packed(self.h, gw, go, gl, n, res.ctypes.data, _lib.CONTIG_CB(cb), None) == 0
        return res, out

    def keep_reads(self, on=True, expected_bases=0):
        assert HostCheck.keep_reads(self, on, expected_bases) == 0

    def assemble_kept(self, n):
        rc, res, out = HostCheck.assemble_kept(self, n)
        assert rc == 0
        return res, out

    def import_counters(self, arr):
        self.l.hc_counters_import.argtypes = [C.c_void_p, C.c_void_p]
        assert self.l.hc_counters_import(self.h, arr.ctypes.data) == 0

    def close(self):
        if self.h:
            self.l.hc_destroy(self.h)
            self.h = None


def make_engine(case):
    hc = DistHostCheck(case.k, case.counters, case.num_hashes, case.min_cov, case.trim, insert_batch=case.insert_batch,
                       claim_log2=case.claim_log2, p2_first=case.p2_first, mask=case.mask)
    hc.attach()
    return hc


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    what = sys.argv[1]
    if what == "selftest":
        # abyss_amd.dist.selftest (what bench.py runs on the RCCL communicator before the timed steps of an N > 1 run) over gloo:
        # a sound communicator passes every check on every rank; one whose all_to_all_v delivers a part to the wrong place, or
        # whose all_reduce forgets a rank, is caught
        comm = adist.StagedTorchComm(*adist.host_memory_io())
        good = adist.selftest(comm, adist.HostBuf)
        real_a2a, real_ar = comm._a2a, comm._ar  # (the thunks themselves: a field read back from the struct aliases the field)

        def bad_a2a(user, send, sc, sd, recv, rc, rd, stream):
            rc_ = real_a2a(user, send, sc, sd, recv, rc, rd, stream)
            n = sum(int(rc[q]) for q in range(world))
            if n > 1:
                C.memmove(recv, recv + 1, n - 1)  # (everything one byte early)
            return rc_

        def bad_ar(user, buf, count, dtype, op, stream):
            return 0  # (nothing combined)
        keep = (adist.A2A_FN(bad_a2a), adist.AR_FN(bad_ar))
        comm.struct.all_to_all_v = keep[0]
        bad1 = adist.selftest(comm, adist.HostBuf)
        comm.struct.all_to_all_v = real_a2a
        comm.struct.all_reduce = keep[1]
        bad2 = adist.selftest(comm, adist.HostBuf)
        ok = {"good": good, "bad_a2a": bad1, "bad_all_reduce": bad2}
        box = [None] * world
        dist.all_gather_object(box, ok)
        if rank == 0:
            print("RESULT " + json.dumps({"ranks": box}), flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return
    if what not in cases.NAMES:
        raise SystemExit("unknown case")
    ok, hc, _ = cases.run(what, sys.argv[2] if len(sys.argv) > 2 else None, make_engine, rank, world)
    if what == "sliced":
        ok["direct_access_refused"] = not bool(hc.l.hc_counters(hc.h))
    ok["stats"] = cases.shared_stats(hc)
    ok["comm_calls"] = hc.comm.calls
    # every rank must have reached the same verdicts
    flat = json.dumps({k: v for k, v in ok.items() if k not in ("comm_calls", "comm_pass1")}, sort_keys=True)  # (what a rank sent is its own business)
    box = [None] * world
    dist.all_gather_object(box, flat)
    ok["ranks_agree"] = all(b == box[0] for b in box)
    if rank == 0:
        print("RESULT " + json.dumps(ok), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
