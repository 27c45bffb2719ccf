"""The loader of the contig graph, as Overlap, SimpleGraph, MergeContigs, PopBubbles and abyss-rresolver-short run it (through
tests/hostcheck, so without a device): the formats it refuses, a contig with one vertex, a graph built with another k, and the two
formats it reads, with blank lines in front.  Every line on stderr and the exit status are compared; the texts were recorded from
the build in which each of the five cores carried its own copy of the loader."""
import os
import re
import subprocess

import pytest

from abyss_amd import build

CONTIGS = b">0 8 10\nACGTACGG\n>1 8 12\nCGGTTACA\n"
WELL_FORMED = {
    "adj": b"\n\n0 8 10\t; 1+\t;\n1 8 12\t;\t; 0+\n",
    "dot": b'\n \n\ndigraph adj {\ngraph [k=4]\nedge [d=-3]\n"0+" [l=8 C=10]\n"0-" [l=8 C=10]\n"1+" [l=8 C=12]\n"1-" [l=8 C=12]\n'
           b'"0+" -> "1+"\n"1-" -> "0-"\n}\n',
}
OTHER_FORMATS = {"@": b"\n\n@SQ\tSN:0\tLN:8\n", "H": b" \nH\tVN:Z:1.0\n", ">": b"\n>0\nACGTACGG\n", "g": b"\t\ngraph adj {\n}\n"}
ONE_VERTEX = b'digraph adj {\ngraph [k=4]\n"0+" [l=8 C=10]\n}\n'
OTHER_K = WELL_FORMED["dot"].replace(b"[k=4]", b"[k=5]")

# program -> (checker, the arguments in front of the options, the options and files around the graph `g`, what fail() puts first)
PROGRAMS = {
    "Overlap": ("OV_CHECK", ["run"], ["-k4", "-o", "out.fa", "contigs.fa", "g", "est.dist"], "Overlap: error: "),
    "SimpleGraph": ("SG_CHECK", ["run"], ["-k4", "-o", "out.path", "g", "est.dist"], "SimpleGraph: error: "),
    "MergeContigs": ("MC_CHECK", ["run"], ["-k4", "-o", "out.fa", "contigs.fa", "g", "paths"], "MergeContigs: error: "),
    "PopBubbles": ("PB_CHECK", ["run"], ["-k4", "contigs.fa", "g"], "PopBubbles: error: "),
    # (the contigs' file is not there: the run ends right after the graph)
    "abyss-rresolver-short": ("RRESOLVER_CHECK", [], ["-b1M", "-k4", "-g", "o.g", "-c", "o.fa", "missing.fa", "g", "reads.fa"], "error: "),
}

STATS = "V=4 E=2 E/V=0.5\nDegree: ▅▅\n        01234\n0: 50% 1: 50% 2-4: 0% 5+: 0% max: 1\n"
SG_SUMMARY = ("\nSeed too short: 0\nSeeds with no edges: 0\nEdges removed: 0\nTotal paths attempted: 0\nUnique path: 0\nNo possible paths: 0\n"
              "No valid paths: 0\nRepetitive: 0\nMultiple valid paths: 0\nToo many solutions: 0\nToo complex: 0\n"
              "\nThe minimum number of pairs in a distance estimate is 4294967295.\n")
# program -> (status, stdout, stderr) of the well-formed graphs under -v, the same for both formats
PAST_THE_LOADER = {
    "Overlap": (0, "Overlap: 0\nScaffold: 0\nNo overlap: 0\nInsignificant (<5bp): 0\nHomopolymer: 0\nMotif: 0\nAmbiguous: 0\n", ""),
    "SimpleGraph": (0, STATS + SG_SUMMARY, "Reading `g'...\nReading `est.dist'...\n"),
    "MergeContigs": (0, "", "Reading `g'...\nRead 4 vertices.\nReading `contigs.fa'...\nRead 2 sequences.\nReading `paths'...\nRead 0 paths.\n"),
    "PopBubbles": (0, "", "Reading `g'...\n" + STATS + "Reading `contigs.fa'...\n"
                   "Bubbles: 0 Popped: 0 Scaffolds: 0 Complex: 0 Too long: 0 Too many: 0 Dissimilar: 0\n"),
    "abyss-rresolver-short": (1, "", "Loading contig graph from `g'...\nContig graph loaded.\n" + STATS + "Loading contigs from `missing.fa'...\n"
                              "error: `missing.fa': No such file or directory\n"),
}


@pytest.fixture(scope="module", autouse=True)
def checkers():
    build.build_hostcheck()


def run(program, tmp, graph, verbose=False):
    checker, front, argv, _ = PROGRAMS[program]
    tmp = str(tmp)
    for name, data in (("contigs.fa", CONTIGS), ("g", graph), ("est.dist", b""), ("paths", b""), ("reads.fa", b">r\nACGTACGGTTACA\n")):
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(data)
    e = dict(os.environ)
    e.pop("COLUMNS", None)
    r = subprocess.run([getattr(build, checker)] + front + (["-v"] if verbose else []) + argv, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=e, timeout=60)
    # (getopt's own messages name argv[0]; nothing here should come from getopt, and a line that did would show as it is)
    r.stderr = "".join(re.sub(r"^\S*/\w+_check: ", program + ": ", ln) for ln in r.stderr.decode().splitlines(True))
    r.stdout = r.stdout.decode()
    return r


def refused(program, tmp, graph, message):
    r = run(program, tmp, graph)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", PROGRAMS[program][3] + message + "\n")


@pytest.mark.parametrize("first", sorted(OTHER_FORMATS))
@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_other_formats_are_refused_by_their_first_byte(program, first, tmp_path):
    refused(program, tmp_path, OTHER_FORMATS[first], "`g': this build reads the contig graph in GraphViz (--dot) or ADJ format only")


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_a_contig_with_one_vertex_is_refused(program, tmp_path):
    refused(program, tmp_path, ONE_VERTEX, "`g': a contig is missing one of its two vertices")


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_a_graph_built_with_another_k_is_refused(program, tmp_path):
    r = run(program, tmp_path, OTHER_K)  # (the reader's own line: no program in front of it)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "error: the graph was built with k=5, not 4\n")


@pytest.mark.parametrize("graph", sorted(WELL_FORMED))
@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_a_well_formed_graph_after_blank_lines_gets_past_the_loader(program, graph, tmp_path):
    r = run(program, tmp_path, WELL_FORMED[graph], verbose=True)
    assert (r.returncode, r.stdout, r.stderr) == PAST_THE_LOADER[program]
