"""MD:Z of the SAM writer (sam_core.h mdEmit) on the CPU: tests/md_host.cpp, a program of its own built
with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, formats hand-written hits
over a small three-contig index (count pass, then write pass, which must agree) and every MD is
compared with the rule's plain restatement, tests/md_ref.py.  The cases are the smallest at which the
word-wise compare can go wrong: match runs around the 32-base step at every alignment of the window,
mismatches at the ends, deletions, insertions and clips, N on either side, the reverse strand, lines
that start before or end behind their contig, the merged split forms as printed, pairs and a rescued
mate.  With sam_tags = 0 the text is the MD-on text with the tags stripped.  No GPU."""
import os
import random
import re
import shutil
import subprocess

import pytest

import md_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def _genome():
    rng = random.Random(20)
    c1 = "".join(rng.choice("ACGT") for _ in range(900))
    c2 = "".join(rng.choice("ACGT") for _ in range(200))
    c2 = c2[:80] + "N" * 40 + c2[120:]
    c3 = "".join(rng.choice("ACGT") for _ in range(150))
    return [("c1", c1), ("c2", c2), ("c3", c3)]


GENOME = _genome()
CONTIGS = dict(GENOME)
_CIG = re.compile(r"(\d+)([MIDNSHPX])")


def seq_for(ci, pos, cigar, rng, subs=()):
    """A printed SEQ that follows `cigar` from `pos` on contig ci (reference bases under M, random ones
    under I and S, A where the reference has none), then the substitutions subs: (q, base or None = another base)."""
    ref = GENOME[ci][1]
    out, r = [], pos
    for n, op in _CIG.findall(cigar):
        n = int(n)
        if op in "MX":
            for _ in range(n):
                c = ref[r - 1] if 1 <= r <= len(ref) else "A"
                out.append(c if c in "ACGT" else "A")
                r += 1
        elif op in "DN":
            r += n
        elif op in "IS":
            out += [rng.choice("ACGT") for _ in range(n)]
    for q, b in subs:
        out[q] = b if b else {"A": "C", "C": "G", "G": "T", "T": "A"}[out[q]]
    return "".join(out)


class Cases:
    def __init__(self):
        self.lines, self.rng, self.n = [], random.Random(7), 0

    def _read(self, seq, strand):
        self.n += 1
        read = revcomp(seq) if strand else seq
        self.lines.append("READ r%d %s %s" % (self.n, read if read else "-", "I" * len(read) if read else "*"))

    def _hit(self, ci, pos, ml, qs, qe, diff, strand, nh, nxt, cigar):
        self.lines.append("HIT %d %d %d %d %d %d %d %d %d %s" % (ci, pos, ml, qs, qe, diff, strand, nh, nxt, cigar or "-"))

    def single(self, ci, pos, cigar, strand=0, subs=(), seq=None):
        """one hit, one line; the read is the printed SEQ (reverse-complemented for strand 1)"""
        s = seq_for(ci, pos, cigar, self.rng, subs) if seq is None else seq
        self._read(s, strand)
        self._hit(ci, pos, len(s), 0, len(s), len(subs), strand, 1, -1, cigar)
        self.lines.append("END")

    def chain(self, seq, strand, h, s):
        """a head hit and its split: (contig, pos, matchLength, qStart, qEnd, strand, numHits, cigar) each"""
        self._read(seq, strand)
        self._hit(h[0], h[1], h[2], h[3], h[4], 1, h[5], h[6], 1, h[7])
        self._hit(s[0], s[1], s[2], s[3], s[4], 0, s[5], s[6], -1, s[7])
        self.lines.append("END")

    def pair(self, m1, m2, rescue=None, ins=(50, 500)):
        """mates as (seq, strand, [(contig, pos, cigar, numHits)]); rescue = (which, contig, pos, strand, diff, cigar)"""
        for seq, strand, hits in (m1, m2):
            self._read(seq, strand)
            for ci, pos, cigar, nh in hits:
                self._hit(ci, pos, len(seq), 0, len(seq), 0, strand, nh, -1, cigar)
        if rescue:
            self.lines.append("RESCUE %d %d %d %d %d 1 %s" % rescue)
        self.lines.append("PAIR %d %d" % ins)


def build_cases():
    c = Cases()
    rng = c.rng
    # match runs of every length around the 32-base step, the run starting at text offsets 0, 1, 31, 33
    # modulo 32 (contig c1 starts at text offset 0): a mismatch, the run, a mismatch, three matches
    for run in (0, 1, 31, 32, 33, 63, 64, 65, 128):
        for o in (0, 1, 31, 33):
            pos = o if o else 32  # the run starts at contig position pos + 1 = text offset pos
            c.single(0, pos, "%dM" % (run + 5), subs=[(0, None), (run + 1, None)])
            c.single(0, pos + 64, "%dM" % (run + 5), strand=1, subs=[(0, None), (run + 1, None)])
    # mismatches at the first and at the last base, adjacent mismatches, no mismatch
    c.single(0, 100, "50M", subs=[(0, None)])
    c.single(0, 100, "50M", subs=[(49, None)])
    c.single(0, 100, "50M", subs=[(0, None), (49, None)])
    c.single(0, 101, "50M", subs=[(20, None), (21, None), (22, None)])
    c.single(0, 97, "64M", subs=[(31, None), (32, None)])
    c.single(0, 97, "64M")
    # D at an element boundary followed directly by a mismatch: ...^XY0Z...
    c.single(0, 200, "20M2D30M", subs=[(20, None)])
    c.single(0, 200, "20M2D30M", strand=1, subs=[(20, None)])
    c.single(0, 33, "32M1D32M")
    c.single(0, 10, "5M3D5M2D5M")
    # I, and S leading, trailing and in the middle
    c.single(0, 300, "30M2I30M", subs=[(40, None)])
    c.single(0, 300, "5S40M", subs=[(5, None)])
    c.single(0, 300, "40M7S", subs=[(39, None)])
    c.single(0, 300, "3S27M1S52M4S", subs=[(31, None)])
    c.single(0, 300, "27M1S52M", strand=1)
    c.single(0, 300, "10M5N10M")
    # N in the read, in the reference, in both (c2 has N at 81..120)
    c.single(0, 400, "60M", subs=[(0, "N"), (30, "N"), (59, "N")])
    c.single(1, 60, "100M")
    c.single(1, 60, "100M", subs=[(25, "N"), (26, "N"), (70, "N")])
    c.single(1, 60, "100M", strand=1, subs=[(25, "N"), (61, "N")])
    c.single(1, 90, "10M3D10M")
    # POS <= 0, a window running into the next contig, the last contig's end
    c.single(2, -1, "80M")
    c.single(2, 0, "40M", strand=1)
    c.single(2, -70, "40M")
    c.single(0, 881, "50M")
    c.single(0, 899, "4M3D10M")
    c.single(1, 181, "64M", strand=1)
    c.single(2, 141, "30M")
    c.single(2, 150, "1M2D3M")
    c.single(2, 200, "33M")
    # read lengths
    for m in (1, 40, 129, 300, 512):
        subs = [(m // 2, None)] if m > 1 else []
        c.single(0, 7, "%dM" % m, subs=subs)
        c.single(0, 37, "%dM" % m, strand=1, subs=subs + ([(m - 1, "N")] if m > 1 else []))
    c.single(0, 7, "1M", subs=[(0, None)])
    # a CIGAR longer than SEQ (SEQ past its end reads as N), and an empty CIGAR
    c.single(0, 50, "40M", seq=seq_for(0, 50, "30M", rng))
    c.single(0, 50, "", seq=seq_for(0, 50, "30M", rng))
    # the merged forms of a split chain, as printed (samChain):
    full = seq_for(0, 500, "60M", rng) + seq_for(1, 10, "40M", rng)
    # list a + S(postS): unique head, unique split on another contig, head not shorter
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (1, 10, 40, 60, 100, 0, 1, "40M"))
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "55M5S"), (1, 10, 40, 60, 100, 0, 1, "40M"))
    # ... and a repeated split: S of the split's query range, after list a
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (1, 10, 40, 60, 100, 0, 3, "40M"))
    full = seq_for(2, 20, "40M", rng) + seq_for(0, 600, "60M", rng, subs=[(0, None), (33, None)])
    # list a + list b: unique both, other contig, the split longer (printed on the split's contig from
    # its POS - the head's length: the head's part is compared with whatever lies there)
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 1, "40M"), (0, 600, 60, 40, 100, 0, 1, "60M"))
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 1, "38M2S"), (0, 600, 60, 40, 100, 0, 1, "2S28M2D30M"))
    c.chain(revcomp(full), 1, (2, 20, 40, 0, 40, 1, 1, "38M2S"), (0, 600, 60, 40, 100, 1, 1, "2S58M"))
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 1, "40M"), (0, 30, 60, 40, 100, 0, 1, "60M"))  # POS <= 0
    # S(preS) + list b: repeated head, unique split
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 2, "40M"), (0, 600, 60, 40, 100, 0, 1, "60M"))
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 2, "40M"), (0, 600, 60, 40, 100, 0, 1, "5S25M1I29M"))
    # a two-line split record: unique both, one contig (the second also on the other strand)
    full = seq_for(0, 500, "60M", rng, subs=[(10, None)]) + seq_for(0, 700, "40M", rng, subs=[(39, None)])
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (0, 700, 40, 60, 100, 0, 1, "40M"))
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (0, 700, 40, 60, 100, 1, 1, "40M"))
    c.chain(revcomp(full), 1, (0, 500, 60, 0, 60, 1, 1, "20M1D40M"), (0, 700, 40, 60, 100, 1, 1, "40M"))
    # pairs: a proper pair, an unmapped mate, a rescued mate (RescueOut::cig), a rescued mate 1
    a = seq_for(0, 100, "50M", rng, subs=[(3, None)])
    b = seq_for(0, 300, "20M1D30M", rng, subs=[(20, None)])
    c.pair((a, 0, [(0, 100, "50M", 1)]), (b, 1, [(0, 300, "20M1D30M", 1)]))
    c.pair((a, 0, [(0, 100, "50M", 2), (0, 101, "50M", 2)]), (b, 1, []))
    c.pair((a, 0, [(0, 100, "50M", 1)]), (b, 1, []), rescue=(2, 0, 300, 1, 2, "20M1D30M"))
    c.pair((b, 1, []), (a, 0, [(0, 100, "50M", 1)]), rescue=(1, 0, 300, 1, 2, "20M1D30M"), ins=(10, 100))
    c.pair((a, 1, []), (b, 0, []))
    return "\n".join(c.lines) + "\n"


@pytest.fixture(scope="module")
def md_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("md_host")
    exe = d / "md_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-fopenmp", "-I", CSRC] + SAN + [
        "-o", str(exe), os.path.join(HERE, "md_host.cpp"), os.path.join(CSRC, "host_index.cpp"), os.path.join(CSRC, "sam.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    fasta = d / "g.fa"
    fasta.write_text("".join(">%s\n%s\n" % (n, s) for n, s in GENOME))
    cases = d / "cases.txt"
    cases.write_text(build_cases())

    def run(tags):
        env = dict(os.environ)
        env.update({"OMP_NUM_THREADS": "2", "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1",
                    "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
        r = subprocess.run([str(exe), str(fasta), str(cases), str(tags)], capture_output=True, env=env, timeout=300)
        err = r.stderr.decode(errors="replace")
        for tag in ("Sanitizer", "runtime error"):
            assert tag not in err, err[-6000:]
        assert r.returncode == 0, (r.returncode, err[-4000:])
        return r.stdout.decode()

    return run


@pytest.fixture(scope="module")
def sam_md(md_host):
    return md_host(1)


def test_every_md_follows_the_rule(sam_md):
    n = md_ref.check_sam(sam_md, CONTIGS)
    lines = sam_md.splitlines()
    assert n >= 130 and n < len(lines)  # (and some lines are unmapped: no MD)
    for line in lines:
        if int(line.split("\t")[1]) & 0x4:
            assert "MD:Z:" not in line


def test_cases_are_what_they_claim(sam_md):
    """the printed lines hold the forms the cases were written for"""
    recs = [l.split("\t") for l in sam_md.splitlines()]
    mds = [md_ref.md_field("\t".join(f))[0] for f in recs]
    cig = [f[5] for f in recs]
    assert any(re.search(r"\^[ACGT]{2}0[ACGT]", m or "") for m in mds)            # D, then a mismatch at once
    assert any(re.fullmatch(r"\d+M\d+S\d+M", c) for c in cig)                      # an S in the middle
    assert any(re.fullmatch(r"\d+S\d+M\d+S\d+M\d+S", c) for c in cig)
    assert any(int(f[3]) <= 0 for f in recs)
    assert any(int(f[1]) & 0x10 and m for f, m in zip(recs, mds))
    assert any(m and "N" in m for m in mds)
    assert any(m == "0" and f[5] == "" for f, m in zip(recs, mds))                 # an empty CIGAR
    assert any(m == "128" for m in mds) or any(re.search(r"[ACGT]128[ACGT]", m or "") for m in mds)
    assert any(int(f[1]) & 0x1 and int(f[1]) & 0x40 and not int(f[1]) & 0x80 and f[6] == "=" for f in recs)  # split lines
    assert {len(f[9]) for f in recs} >= {1, 40, 129, 300, 512}
    # the merged forms: list a + S, list a + list b (merged at the seam), S + list b (merged)
    assert "55M45S" in cig and "60M40S" in cig and "100M" in cig and "38M4S28M2D30M" in cig and "45S25M1I29M" in cig
    # a literal value, worked by hand: mismatch at the first base, 31 matches, mismatch, 3 matches
    f = recs[2 * 4 * 2]  # run = 31, offset 0, forward
    assert f[5] == "36M" and re.fullmatch(r"0[ACGT]31[ACGT]3", md_ref.md_field("\t".join(f))[0])


def test_tags_off_is_the_same_text_without_md(md_host, sam_md):
    plain = md_host(0)
    assert "MD:Z:" not in plain
    assert md_ref.strip_md(sam_md) == plain
