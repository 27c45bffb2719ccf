"""The mapping goldens (tests/golden/map, written by tests/golden/make_map.py): cases.json and the targets, reads, index files and SAM
outputs packed in data.tar.gz; and the one input too large to commit, the 2 Mbp target with its reads, which is generated here
(the goldens hold the digests of its index files and the SAM of its reads)."""
import functools
import hashlib
import struct

import numpy as np

import golden_archive

files, golden, cases = golden_archive.bind("map")


def _mix(x):
    """splitmix64 of an array of uint64: the same values on every numpy"""
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def random_bases(n, seed):
    with np.errstate(over="ignore"):
        r = _mix(np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3))
    return np.frombuffer(b"ACGT", dtype=np.uint8)[(r >> np.uint64(33)) & np.uint64(3)].tobytes()


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


BIG_CONTIGS = [(i, 20000 + 3571 * (i % 23)) for i in range(34)]  # about 2 Mbp in 34 contigs


@functools.lru_cache(maxsize=None)
def big_target():
    """big.fa: numeric ids, one sequence line a record"""
    out = []
    for i, n in BIG_CONTIGS:
        out.append(b">%d\n%s\n" % (i, random_bases(n, 1000 + i)))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def big_reads(n=3000, length=150):
    """big_reads.fa: reads of big.fa on both strands, every seventh with a substitution, every 31st with an N"""
    seqs = [random_bases(m, 1000 + i) for i, m in BIG_CONTIGS]
    with np.errstate(over="ignore"):
        r = _mix(np.arange(3 * n, dtype=np.uint64) + np.uint64(77))
    out = []
    for j in range(n):
        c = int(r[3 * j] % np.uint64(len(seqs)))
        at = int(r[3 * j + 1] % np.uint64(len(seqs[c]) - length))
        s = bytearray(seqs[c][at:at + length])
        e = int(r[3 * j + 2] % np.uint64(length))
        if j % 7 == 3:
            s[e] = b"ACGT"[(b"ACGT".index(s[e]) + 1) % 4]
        if j % 31 == 5:
            s[e] = ord("N")
        s = bytes(s)
        if j % 2:
            s = revcomp(s)
        out.append(b">b%d/%d\n%s\n" % (j, 1 + j % 2, s))
    return b"".join(out)


def input_bytes(name):
    """a case's input by name: from the archive, or generated"""
    if name == "big.fa":
        return big_target()
    if name == "big_reads.fa":
        return big_reads()
    return golden(name)


def sha256(data):
    return hashlib.sha256(data).hexdigest()


def parse_fm(data):
    """(sample period, sampled SA, BWT with 255 for the sentinel) of a .fm file (FMIndex.h:512-526, BitArrays.h, bit_array.cc)"""
    version, period, na, rest = data.split(b"\n", 3)
    assert version == b"FM 64 1" and rest[:int(na)] == b"-ACGT"
    ns, rest = rest[int(na):].split(b"\n", 1)
    ns = int(ns)
    sa = np.frombuffer(rest[:8 * ns], dtype="<u8")
    rest = rest[8 * ns:]
    arrays, = struct.unpack("<I", rest[:4])
    rest, bwt = rest[4:], None
    for c in range(arrays):
        m, = struct.unpack("<Q", rest[:8])
        words = (m + 63) // 64
        bits = np.unpackbits(np.frombuffer(rest[8:8 + 8 * words], dtype=np.uint8), bitorder="little")[:m]
        rest = rest[8 + 8 * words:]
        if bwt is None:
            bwt = np.full(m, 255, dtype=np.uint8)
        bwt[bits == 1] = c
    assert not rest
    return int(period), sa, bwt
