"""Shared by the pipeline tests (test_pipeline_host.py, test_gpu_pipeline.py): seeded inputs at the shapes abyss-pe produces, and the
chain from contigs to joined contigs

    abyss-map -j1 -l40 R1 R2 T | abyss-fixmate -l40 -h lib.hist | LC_ALL=C sort -snk3 -k4 > lib.sam
    DistanceEst -j1 -k64 -l40 -s200 -n10 -o lib.dist lib.hist < lib.sam
    AdjList -k64 -m50 T > T.adj
    Overlap -k64 -g out.adj -o out.fa T T.adj lib.dist

run by any set of programs: the unmodified reference's (oracle/_ref, built by `make -C oracle ref`), the hostcheck stand-ins or the
GPU binaries.  abyss-fixmate is always the reference's.  Nothing here is read from tests/golden: every input is generated, and the
reference runs live.  Reference(...) asserts, on the reference's own output, the conditions that keep a comparison from passing on
nothing."""
import functools
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np

from abyss_amd import build, synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_distanceest as md  # noqa: E402  (make_pairs: the read pairs of the DistanceEst goldens)
import make_map as mm  # noqa: E402

REF = os.path.join(build.ORACLE_DIR, "_ref")
REF_PROGRAMS = ("abyss-bloom-dbg", "AdjList", "abyss-map", "abyss-index", "abyss-fixmate", "DistanceEst", "Overlap")
K, L, MIN_ADJ = 64, 40, 50
DE_ARGS = ["-j1", "-k%d" % K, "-l%d" % L, "-s200", "-n10"]
WIDTHS = (65534, 65535, 65536, 131071, 131072)  # FM targets around the sizes at which the doubling rounds' rank keys widen
TIMEOUT = 120


def have_ref():
    return all(os.path.exists(os.path.join(REF, p)) for p in REF_PROGRAMS)


# ---- programs: name -> (file to execute, the argv it is given in front of its arguments)

def tools(kind):
    """`ref`: the unmodified reference; `host`: the hostcheck stand-ins; `gpu`: abyss_amd/bin.  Each program is started under its
    plain name (argv[0]), as abyss-pe starts it through PATH, so that the @PG line of a SAM file is the same whoever wrote it."""
    t = {p: (os.path.join(REF, p), [p]) for p in REF_PROGRAMS}
    if kind == "host":
        t["abyss-map"] = (build.FM_CHECK, [build.FM_CHECK, "map"])
        t["abyss-index"] = (build.FM_CHECK, [build.FM_CHECK, "index"])
        t["DistanceEst"] = (build.DE_CHECK, [build.DE_CHECK, "run"])
        t["Overlap"] = (build.OV_CHECK, [build.OV_CHECK, "run"])
        t["AdjList"] = (build.ADJLIST_CHECK, [build.ADJLIST_CHECK])
    elif kind == "gpu":
        for p in REF_PROGRAMS:
            if p != "abyss-fixmate":
                t[p] = (os.path.join(build.BIN_DIR, p), [p])
    elif kind != "ref":
        raise ValueError(kind)
    return t


def run(tool, args, cwd, stdin=b"", env=None):
    exe, argv = tool
    e = dict(os.environ, LC_ALL="C")
    e.pop("COLUMNS", None)
    e.update(env or {})
    r = subprocess.run(argv + list(args), executable=exe, cwd=str(cwd), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e,
                       timeout=TIMEOUT)
    assert r.returncode == 0, (argv + list(args), r.returncode, r.stderr[-2000:])
    return r


def read(d, name):
    with open(os.path.join(str(d), name), "rb") as f:
        return f.read()


def write(d, name, data):
    with open(os.path.join(str(d), name), "wb") as f:
        f.write(data)


def with_command_line(sam, argv):
    """a SAM file with the CL: of its @PG line replaced (tests/test_map_host.py:expected_sam)"""
    lines = sam.split(b"\n")
    assert lines[1].startswith(b"@PG\t") and b"\tCL:" in lines[1]
    lines[1] = lines[1][:lines[1].index(b"\tCL:") + 4] + " ".join(argv).encode()
    return b"\n".join(lines)


def program_lines(err):
    """stderr without the directory of argv[0], which getopt and the programs' own messages print"""
    return [re.sub(r"^\S*/([A-Za-z_-]+): ", r"\1: ", ln) for ln in err.decode().splitlines()]


# ---- the stages

def stage_unitigs(t, d, reads):
    """abyss-bloom-dbg as abyss-pe runs it, sized for 100 kbp"""
    r = run(t["abyss-bloom-dbg"], ["-j1", "-k%d" % K, "-b8M", "-H4", "-q3"] + reads, d)
    write(d, "unitigs.fa", r.stdout)
    return r.stdout


def stage_adj(t, d, target, fmt=None, out="T.adj"):
    r = run(t["AdjList"], ["-k%d" % K, "-m%d" % MIN_ADJ] + (["--" + fmt] if fmt else []) + [target], d)
    write(d, out, r.stdout)
    return r.stdout


def stage_map(t, d, target, reads, l=L, j=1, env=None):
    """(SAM, the argv after the program's name)"""
    args = ["-j%d" % j, "-l%d" % l] + reads + [target]
    return run(t["abyss-map"], args, d, env=env).stdout, args


def stage_mates(ref, d, sam, l=L):
    """the reference's abyss-fixmate and sort(1) over a SAM: lib.hist and lib.sam"""
    r = run(ref["abyss-fixmate"], ["-l%d" % l, "-h", "lib.hist"], d, stdin=sam)
    s = subprocess.run(["sort", "-snk3", "-k4"], input=r.stdout, stdout=subprocess.PIPE, env=dict(os.environ, LC_ALL="C"), check=True, timeout=TIMEOUT)
    write(d, "lib.sam", s.stdout)
    return read(d, "lib.hist"), s.stdout


def stage_distance(t, d, extra=(), out="lib.dist", env=None):
    """(the -o file, stdout, stderr)"""
    r = run(t["DistanceEst"], DE_ARGS + list(extra) + ["-o", out, "lib.hist"], d, stdin=read(d, "lib.sam"), env=env)
    return read(d, out), r.stdout, r.stderr


def stage_overlap(t, d, target, adj="T.adj", dist="lib.dist", extra=(), env=None):
    """{out.fa, out.adj, stdout, stderr}"""
    for f in ("out.fa", "out.adj"):
        if os.path.exists(os.path.join(str(d), f)):
            os.remove(os.path.join(str(d), f))
    r = run(t["Overlap"], list(extra) + ["-k%d" % K, "-g", "out.adj", "-o", "out.fa", target, adj, dist], d, env=env)
    return {"out.fa": read(d, "out.fa"), "out.adj": read(d, "out.adj"), "stdout": r.stdout, "stderr": r.stderr}


CHAIN_ORDER = ["unitigs.fa", "T.adj", "map.sam", "lib.hist", "lib.sam", "lib.dist", "out.fa", "out.adj", "overlap.stdout"]


def chain(t, ref, d, inp):
    """the whole chain with the programs `t` (mates and sort: `ref`), each stage on what the stage before it wrote: every file, in
    pipeline order"""
    out = {}
    for name, data in inp.files.items():
        write(d, name, data)
    if inp.from_reads:
        out["unitigs.fa"] = stage_unitigs(t, d, inp.reads)
    out["T.adj"] = stage_adj(t, d, inp.target)
    out["map.sam"], _ = stage_map(t, d, inp.target, inp.reads)
    out["lib.hist"], out["lib.sam"] = stage_mates(ref, d, out["map.sam"])
    out["lib.dist"] = stage_distance(t, d)[0]
    o = stage_overlap(t, d, inp.target)
    out["out.fa"], out["out.adj"], out["overlap.stdout"] = o["out.fa"], o["out.adj"], o["stdout"]
    return out


def first_difference(got, want):
    """the first file, in pipeline order, that differs, and where: None when all are equal"""
    for name in CHAIN_ORDER:
        if name not in want or name not in got:
            continue
        a, b = got[name], want[name]
        if a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            line = a.count(b"\n", 0, at) + 1
            return "%s differs at byte %d (line %d): got %r, want %r" % (name, at, line, a[max(0, at - 60):at + 60], b[max(0, at - 60):at + 60])
    return None


# ---- inputs

class Input:
    def __init__(self, name, files, target, reads, from_reads=False, l=L, note=None):
        self.name, self.files, self.target, self.reads, self.from_reads, self.l, self.note = name, files, target, reads, from_reads, l, note or {}


def _periodic_unit(rng, p):
    while True:
        u = mm.rand_seq(rng, p)
        if len(set(u)) >= min(p, 2) and not any(u == u[:q] * (p // q) for q in range(1, p) if p % q == 0):
            return u


# the junctions of `cut` that share a run of period 1 (homopolymer) or a short motif: junction number -> (period, run length).  A
# run must show three matches l, l - p, l - 2p and be at least Overlap's -m (5) long; it stays below AdjList's -m50.
PLANTED = {4: (1, 9), 13: (1, 14), 22: (1, 23), 31: (1, 6), 8: (2, 11), 17: (3, 14), 26: (7, 24), 35: (2, 30), 40: (3, 19)}


@functools.lru_cache(maxsize=None)
def cut(seed):
    """contigs of 300 to 1500 bp cut from 80,000 random bases, each reverse-complemented with probability 1/2; the next one starts
    after an overlap of k - 1 (30 %: AdjList joins those), of 5 to 49 (25 %), of 1 to 4 (10 %) or a gap of 1 to 200 (35 %); the
    junctions of PLANTED share a homopolymer or a motif instead.  12,000 pairs of 100 bp, fragments of 400 +- 40."""
    rng = random.Random(seed)
    genome = list(mm.rand_seq(rng, 80000))
    layout, at, planted = [], 0, []
    while at + 300 <= len(genome):
        n = min(rng.randrange(300, 1501), len(genome) - at)
        layout.append((at, n, rng.random() < 0.5))
        j = len(layout) - 1  # the junction after contig j
        x = rng.random()
        if j in PLANTED:
            step = -PLANTED[j][1]
            planted.append((at + n + step, ) + PLANTED[j])
        elif x < 0.30:
            step = -(K - 1)
        elif x < 0.55:
            step = -rng.randrange(5, 50)
        elif x < 0.65:
            step = -rng.randrange(1, 5)
        else:
            step = rng.randrange(1, 201)
        at += n + step
    for s, p, run_len in planted:  # genome[s:s + run_len] is what the two contigs share
        if s + run_len + 1 >= len(genome):
            continue
        unit = _periodic_unit(rng, p)
        rep = (unit * (run_len // p + 2))[:run_len]
        before = [c for c in "ACGT" if c not in (rep[p - 1], rep[0], rep[-1])][0]   # breaks the period on either side
        after = [c for c in "ACGT" if c not in (unit[run_len % p], rep[0], rep[-1])][0]
        genome[s - 1:s + run_len + 1] = before + rep + after
    genome = "".join(genome)
    contigs = []
    for i, (a, n, flip) in enumerate(layout):
        s = genome[a:a + n]
        s = mm.revcomp(s) if flip else s
        contigs.append((str(i) if i % 3 == 2 else "%d %d %d" % (i, len(s), 20 * len(s)), s))  # a third without the length and coverage comment
    r1, r2 = md.make_pairs(rng, genome, 12000, 400, 40)
    return Input("cut%d" % seed, {"contigs.fa": mm.fasta(contigs), "r1.fa": r1, "r2.fa": r2}, "contigs.fa", ["r1.fa", "r2.fa"],
                 note={"contigs": len(contigs)})


@functools.lru_cache(maxsize=None)
def asm():
    """4,000 pairs of 150 bp of a 100 kbp diploid genome at 12x: the reference's abyss-bloom-dbg makes 211 unitigs of them"""
    m1, m2 = synth.make_read_set(100000, 12.0, genome_seed=12, read_seed=13)
    files = {}
    for name, m, mate in (("r1.fq", m1, 1), ("r2.fq", m2, 2)):
        seqs = synth.codes_to_ascii(m)
        files[name] = b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, mate, seqs[i].tobytes(), b"I" * m.shape[1]) for i in range(m.shape[0]))
    return Input("asm", files, "unitigs.fa", ["r1.fq", "r2.fq"], from_reads=True)


BLOCK = 20000  # the duplicated block of the `widths` targets


def doubling_rounds(repeat, first=21):
    """prefix doubling from a key of `first` symbols tells two suffixes apart once the key is longer than what they share: a repeat of
    `repeat` symbols needs at least ceil(log2(repeat / first)) doublings"""
    return int(np.ceil(np.log2(repeat / first)))


@functools.lru_cache(maxsize=None)
def repeats():
    """an FM target of about 133 kB, most of it repeated: a 30 kbp contig twice, A x 5000, 20 kbp of a period-7 unit, the reverse
    complement of 8 kbp of the first contig, 40 kbp of random sequence; 3,000 reads of 150 bp cut from the records on both strands"""
    rng = random.Random(20261020)
    first = mm.rand_seq(rng, 30000)
    recs = [("0", first), ("polyA", "A" * 5000), ("2 30000 0", first), ("3", (_periodic_unit(rng, 7) * 3000)[:20000]), ("4", mm.revcomp(first[11000:19000])),
            ("5", mm.rand_seq(rng, 40000))]
    reads = []
    for i in range(3000):
        s = recs[rng.randrange(len(recs))][1]
        at = rng.randrange(0, len(s) - 150 + 1)
        q = s[at:at + 150]
        reads.append(">q%d/%d\n%s\n" % (i, 1 + i % 2, mm.revcomp(q) if rng.random() < 0.5 else q))
    return Input("repeats", {"target.fa": mm.fasta(recs), "reads.fa": "".join(reads).encode()}, "target.fa", ["reads.fa"], l=30)


@functools.lru_cache(maxsize=None)
def width(size):
    """an FM target of exactly `size` bytes that holds a 20 kbp block twice and a 3 kbp homopolymer: the doubling rounds go on, with
    rank keys of the width this size asks for, until the two blocks are told apart"""
    rng = random.Random(size)
    block = mm.rand_seq(rng, BLOCK)
    recs = [("0", block), ("1", block), ("2", "C" * 3000)]
    rest = size - len(mm.fasta(recs)) - len(">3\n\n")
    assert rest > 0
    data = mm.fasta(recs + [("3", mm.rand_seq(rng, rest))])
    assert len(data) == size and data.count(block.encode()) == 2
    return Input("width%d" % size, {"w.fa": data}, "w.fa", [])


def key_bits(n):
    """the width of a rank in the doubling rounds of a text of n bytes: ranks 1..n, 0 past the end"""
    return int(n + 1).bit_length()


INPUTS = {"cut1": lambda: cut(1), "cut2": lambda: cut(2), "asm": asm}


# ---- the reference's run of an input, with every variant the stage tests compare

def overlap_summary(text):
    return dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^([A-Z][A-Za-z ]+?)(?: \(<\d+bp\))?: (\d+)$", text.decode(), re.M))


def estimates(dist):
    """(record, mate, d, n, which list) of every estimate of a .dist file"""
    out = []
    for line in dist.decode().splitlines():
        side = 0
        for e in line.split()[1:]:
            if e == ";":
                side = 1
                continue
            m, d, n, _ = e.split(",")
            out.append((line.split()[0], m, int(d), int(n), side))
    return out


class Reference:
    """the reference chain on an input of INPUTS, run once in `d`, which then holds every file a stage of ours needs as its input"""

    def __init__(self, name, d):
        assert have_ref(), "oracle/_ref is not built (make -C oracle ref)"
        self.inp, self.d, self.name = INPUTS[name](), str(d), name
        t = self.t = tools("ref")
        self.files = chain(t, t, d, self.inp)
        inp = self.inp
        self.map_args = ["-j1", "-l%d" % L] + inp.reads + [inp.target]
        self.dot, _, self.v_err = stage_distance(t, d, ["--dot", "-v"], out="lib.dist.dot")
        self.adj_dot = stage_adj(t, d, inp.target, fmt="dot", out="T.dot")
        self.overlap = {"default": stage_overlap(t, d, inp.target), "v": stage_overlap(t, d, inp.target, extra=["-v"]),
                        "dot": stage_overlap(t, d, inp.target, adj="T.dot", dist="lib.dist.dot")}
        self.summary = overlap_summary(self.files["overlap.stdout"])
        self.fm, self.fai = index_files(t, d, inp.target, read(d, inp.target))
        for ext in (".fm", ".fai"):  # (so that no later abyss-map in this directory finds them)
            os.remove(os.path.join(self.d, inp.target + ext))
        self.check()

    def check(self):
        """what the reference's output must hold before anything of ours is compared with it"""
        est, s = estimates(self.files["lib.dist"]), self.summary
        assert len(est) >= 100, len(est)
        if self.name.startswith("cut"):
            assert s["Overlap"] >= 10 and s["Scaffold"] >= 10 and s["Insignificant"] >= 1 and s["Homopolymer"] >= 1 and s["Motif"] >= 1, s
        else:
            assert s["Overlap"] >= 5 and s["Scaffold"] >= 5, s
        assert any(e[2] < 0 for e in est) and any(e[2] > 0 for e in est)  # negative estimates next to gaps
        assert self.overlap["v"]["stdout"] != self.overlap["default"]["stdout"]

    def stage_dir(self, d, names):
        """a directory of its own for a stage of ours, with the reference's files `names` in it"""
        for n in names:
            shutil.copy(os.path.join(self.d, n), os.path.join(str(d), n))
        return d


class MapReference:
    """the reference's abyss-index and abyss-map on `repeats` or a `widths` target"""

    def __init__(self, inp, d):
        assert have_ref(), "oracle/_ref is not built (make -C oracle ref)"
        self.inp, self.d = inp, str(d)
        t = tools("ref")
        for name, data in inp.files.items():
            write(d, name, data)
        self.sam = None
        if inp.reads:  # (before any index file exists: the reference builds its own)
            self.sam, self.map_args = stage_map(t, d, inp.target, inp.reads, l=inp.l)
            body = [ln.split(b"\t") for ln in self.sam.split(b"\n") if ln and not ln.startswith(b"@")]
            self.multi = sum(1 for f in body if f[2] != b"*" and f[4] == b"0")
            self.unmapped = sum(1 for f in body if f[2] == b"*")
            assert len(body) == 3000 and self.multi >= 1000, (len(body), self.multi, self.unmapped)
        run(t["abyss-index"], [inp.target], d)
        self.fm, self.fai = read(d, inp.target + ".fm"), read(d, inp.target + ".fai")
        os.remove(os.path.join(self.d, inp.target + ".fm"))
        os.remove(os.path.join(self.d, inp.target + ".fai"))


def index_files(t, d, target_name, data):
    """(.fm, .fai) that abyss-index of `t` writes for a target"""
    write(d, target_name, data)
    run(t["abyss-index"], [target_name], d)
    return read(d, target_name + ".fm"), read(d, target_name + ".fai")


# ---- one stage of ours on the reference's upstream files: a difference names its stage

def check_index(t, d, target_name, data, want_fm, want_fai):
    fm, fai = index_files(t, d, target_name, data)
    assert fai == want_fai
    assert len(fm) == len(want_fm) and fm == want_fm


def check_map(t, ref, d, j=1, env=None):
    """`ref`: a Reference or a MapReference"""
    inp = ref.inp
    for name in [inp.target] + inp.reads:
        write(d, name, read(ref.d, name))
    want = ref.sam if isinstance(ref, MapReference) else ref.files["map.sam"]
    sam, args = stage_map(t, d, inp.target, inp.reads, l=inp.l, j=j, env=env)
    want = with_command_line(want, ["abyss-map"] + args)
    assert sam.split(b"\n")[:2] == want.split(b"\n")[:2]  # @HD, and @PG with the command line as it was given
    assert sam == want, first_difference({"map.sam": sam}, {"map.sam": want})


def check_distance(t, ref, d, env=None):
    """the -o file, the --dot output and the -v stderr, on the reference's lib.sam and lib.hist"""
    ref.stage_dir(d, ["lib.sam", "lib.hist"])
    got = stage_distance(t, d, env=env)[0]
    assert got == ref.files["lib.dist"], first_difference({"lib.dist": got}, {"lib.dist": ref.files["lib.dist"]})
    dot, out, err = stage_distance(t, d, ["--dot", "-v"], out="lib.dist.dot", env=env)
    assert dot == ref.dot and out == b""
    assert program_lines(err) == program_lines(ref.v_err)


def check_overlap(t, ref, d, env=None):
    """out.fa, out.adj and stdout: as the chain runs it, with -v, and from the --dot forms of both graphs"""
    ref.stage_dir(d, [ref.inp.target, "T.adj", "T.dot", "lib.dist", "lib.dist.dot"])
    for mode, kw in (("default", {}), ("v", {"extra": ["-v"]}), ("dot", {"adj": "T.dot", "dist": "lib.dist.dot"})):
        got, want = stage_overlap(t, d, ref.inp.target, env=env, **kw), ref.overlap[mode]
        for name in ("out.fa", "out.adj", "stdout"):
            assert got[name] == want[name], (mode, first_difference({"out.fa": got[name]}, {"out.fa": want[name]}))
        assert program_lines(got["stderr"]) == program_lines(want["stderr"]), mode


def check_chain(t, ref, d, from_reads):
    """ours from the top (from the reads where the input has them and `from_reads` says so, else from the reference's contigs)"""
    inp = ref.inp
    if inp.from_reads and not from_reads:
        inp = Input(inp.name, dict(inp.files, **{"unitigs.fa": ref.files["unitigs.fa"]}), inp.target, inp.reads)
    got = chain(t, ref.t, d, inp)
    assert sorted(got) == sorted(k for k in ref.files if k in got) and len(got) >= 8
    diff = first_difference(got, ref.files)
    assert diff is None, diff


# ---- the live reference is the one that wrote the goldens

def check_reference_writes_golden(what, d):
    """one committed golden case of each stage from oracle/_ref: a reference built with other flags (a contracted pmf[i] * w, say)
    fails here"""
    import distanceest_golden as dg
    import map_golden as mg
    import overlap_golden as og
    t = tools("ref")
    if what == "map":
        case = next(c for c in mg.cases()["map"] if c["name"] == "letters_l30")
        for name in [case["target"]] + case["queries"]:
            write(d, name, mg.input_bytes(name))
        assert run(t["abyss-map"], case["argv"], d).stdout == mg.golden(case["sam"])
    elif what == "index":
        write(d, "letters.fa", mg.input_bytes("letters.fa"))
        run(t["abyss-index"], ["letters.fa"], d)
        assert read(d, "letters.fa.fm") == mg.golden("letters.fa.fm") and read(d, "letters.fa.fai") == mg.golden("letters.fa.fai")
    elif what == "distanceest":
        case = next(c for c in dg.cases() if c["name"] == "fr_basic.dist")
        dg.check_case(case, dg.run_case([t["DistanceEst"][0]], case, d))
        case = next(c for c in dg.cases() if c["name"] == "fr_basic.vv_dot")
        dg.check_case(case, dg.run_case([t["DistanceEst"][0]], case, d))
    elif what == "overlap":
        case = next(c for c in og.cases() if c["name"] == "main.default")
        assert og.needs_device(case)  # a case in which pairs reach the search
        og.check_case(case, og.run_case([t["Overlap"][0]], case, d), [t["Overlap"][0]])
    else:
        raise ValueError(what)
