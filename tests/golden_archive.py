"""How the golden modules read tests/golden/<stage>: cases.json, and every other file of the stage packed in data.tar.gz.  Both are
read once a process and shared by whoever asks."""
import functools
import json
import os
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def files(stage):
    """name -> bytes of every file in the stage's data.tar.gz"""
    with tarfile.open(os.path.join(HERE, "golden", stage, "data.tar.gz")) as tar:
        return {m.name: tar.extractfile(m).read() for m in tar.getmembers() if m.isfile()}


@functools.lru_cache(maxsize=None)
def cases(stage):
    return json.load(open(os.path.join(HERE, "golden", stage, "cases.json")))


def bind(stage):
    """(files, golden, cases) of one stage: files() and cases() as above, golden(name) one file's bytes"""
    return functools.partial(files, stage), lambda name: files(stage)[name], functools.partial(cases, stage)
