"""The inputs of the large Konnector cases (tests/golden/konnector/large.json, written by tests/golden/make_konnector.py).

long.fa holds two records too long for one staging slot of abg_kn (64 MiB less its padding): the first is 67,108,576 bases,
the shortest length a slot once refused, and the second 80 MiB.  Their bases come from splitmix64 in numpy uint64 arithmetic, so the bytes
do not depend on library versions; large.json keeps their sha256 and the CPU suite checks it.  Both records carry N runs and
copies of reads.fa's records planted across the places where a slot or a piece of a long record ends.
"""
import hashlib

import numpy as np

LONG_LENGTHS = (67108576, 80 << 20)
LONG_SEED = 0x6B6E5F6C6F6E67
SLOT = 64 << 20
# places a planted read straddles: the end of the piece a 64 MiB slot holds (SLOT - 256 - 32 - 1 bases), the start of the next
# piece at k 64 (63 bases before it), the first length a slot refused, 64 MiB, and a few more
BOUNDARIES = (1 << 20, 1 << 25, SLOT - 289 - 63, SLOT - 289, SLOT - 288, SLOT, SLOT + 4096, 40 << 20)

_M = (1 << 64) - 1


def splitmix64(seed, n):
    """n outputs of splitmix64 started at `seed` (uint64; the state after output i is seed + (i + 1) * golden gamma)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


class _Draws:
    """Python integers from one splitmix64 stream (positions and lengths)."""

    def __init__(self, seed):
        self.seed, self.i = seed, 0

    def below(self, n):
        self.i += 1
        z = (self.seed + self.i * 0x9E3779B97F4A7C15) & _M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
        return (z ^ (z >> 31)) % n


def random_bases(seed, n):
    """n bases of ACGT, two bits of splitmix64 output each (lowest bits first)."""
    words = splitmix64(seed, (n + 31) // 32)
    out = np.empty(len(words) * 32, dtype=np.uint8)
    for j in range(32):
        out[j::32] = ((words >> np.uint64(2 * j)) & np.uint64(3)).astype(np.uint8)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[out[:n]]


def fasta_records(buf):
    """The sequences of a one-line-per-record FASTA (reads.fa)."""
    return [l for l in buf.split(b"\n") if l and not l.startswith(b">")]


def long_record(r, length, reads):
    seq = random_bases(LONG_SEED + 1000003 * r, length)
    d = _Draws(LONG_SEED ^ (r + 1) << 32)
    for _ in range(40):  # N runs of 1 .. 2000 bases
        n = 1 + d.below(2000)
        at = d.below(length - n)
        seq[at:at + n] = ord("N")
    long_reads = [x for x in reads if len(x) >= 150]
    spots = []
    for b in BOUNDARIES:
        if b < length:
            spots += [b - 75, b - 1, b - 149]  # a 150+ base read across b, ending just past it, starting just before it
    spots += [0, length - 150]
    spots += [d.below(length - 300) for _ in range(500)]
    for at in spots:
        x = long_reads[d.below(len(long_reads))]
        at = max(0, min(at, length - len(x)))
        seq[at:at + len(x)] = np.frombuffer(x, dtype=np.uint8)
    return seq


def write_long_fasta(path, reads_fa):
    """long.fa from reads.fa's bytes; returns (sha256, bytes)."""
    reads = fasta_records(reads_fa)
    h = hashlib.sha256()
    size = 0
    with open(path, "wb") as f:
        for r, length in enumerate(LONG_LENGTHS):
            for part in (b">long%d\n" % r, long_record(r, length, reads).tobytes(), b"\n"):
                f.write(part)
                h.update(part)
                size += len(part)
    return h.hexdigest(), size


def sha256_file(path):
    """(sha256, bytes) of a file, read as a stream."""
    h = hashlib.sha256()
    size = 0
    with open(path, "rb") as f:
        while True:
            b = f.read(16 << 20)
            if not b:
                break
            h.update(b)
            size += len(b)
    return h.hexdigest(), size
