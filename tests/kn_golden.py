"""The Konnector goldens (tests/golden/konnector, written by tests/golden/make_konnector.py): cases.json, and the reads, hash
vectors and filter files packed in data.tar.gz."""
import functools
import io
import json
import os

import golden_archive
from util import GOLDEN

KN = os.path.join(GOLDEN, "konnector")
files, golden, cases = golden_archive.bind("konnector")


def hash_vectors():
    return json.loads(golden("hash_vectors.json"))


def workdir(tmp_path):
    """The reads and every golden filter file written into tmp_path (commands refer to them by their plain names)."""
    for name, data in files().items():
        if name.endswith(".bloom") or name.startswith("reads."):
            with open(os.path.join(str(tmp_path), name), "wb") as f:
                f.write(data)
    return str(tmp_path)


@functools.lru_cache(maxsize=None)
def large():
    """large.json: the digests of the large cases (filters past 2^32 bits, records longer than a staging slot)."""
    return json.load(open(os.path.join(KN, "large.json")))


def filter_header(data):
    """(k, bits, start, end, seed) and the level's bytes of a filter file (Bloom::writeHeader: version, k, size and window, seed)."""
    lines = data.split(b"\n", 4)
    bits, start, end = (int(x) for x in lines[2].split(b"\t"))
    return (int(lines[1]), bits, start, end, int(lines[3])), lines[4]
