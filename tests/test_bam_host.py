"""The BAM record writer (csrc/bam_core.h) on the CPU: tests/bam_host.cpp, a program of its own built with the
host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, formats hand-written hits through the BAM
writer and through the SAM writer (count pass, then write pass, which must agree), and every record must
equal tests/bam_ref.py's encoding of the line the SAM writer prints for the same hits (include/gwa.h: a
record is a function of the printed line).  The cases are the smallest at which packing and sizing can go
wrong: SEQ lengths around the nibble pair and the 16-code chunk, both strands, N, absent and odd-length
qualities, names up to the 254-byte limit and one past it, every CIGAR form samChain prints, POS <= 0, "*"
and empty contig names, split records, pairs, the tags with and without MD, and the bin around every level's
edge.  The cases of tests/test_md_host.py run through it as well.  No GPU."""
import os
import random
import re
import shutil
import subprocess

import pytest

import bam_ref
import test_md_host as MH

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = MH.CSRC
CXX = MH.CXX

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

# the FASTA names carry a description: RNAME, @SQ and the BAM header cut it at the first space
FASTA_NAMES = {"c1": "c1 first contig", "c2": "c2\tsecond", "c3": "c3"}
CONTIG_TABLE = [(n, len(s)) for n, s in MH.GENOME]
SEQ_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 129)
NAME_LENGTHS = (0, 1, 16, 17, 254)
QCHARS = [chr(c) for c in range(33, 127)]


class Cases(MH.Cases):
    """md_host's case writer with a name and a quality per read"""

    def __init__(self):
        super().__init__()
        self.name = self.qual = None  # overrides for the next read

    def _read(self, seq, strand):
        self.n += 1
        read = MH.revcomp(seq) if strand else seq
        name = "r%d" % self.n if self.name is None else self.name
        qual = "".join(self.rng.choice(QCHARS) for _ in read) if self.qual is None else self.qual
        if qual in ("*", "@empty") and self.qual is None:  # (a drawn one-base quality must not read as a keyword)
            qual = "I"
        if not read and self.qual is None:
            qual = "@empty"
        self.lines.append("READ %s %s %s" % (name if name else "@empty", read if read else "-", qual))
        self.name = self.qual = None

    def unmapped(self, seq):
        self._read(seq, 0)
        self.lines.append("END")

    def bin(self, flag, beg, reflen):
        self.lines.append("BIN %d %d %d" % (flag, beg, reflen))


BIN_CASES = []


def _bin_cases():
    out = [(0, 0, 0), (0, 0, 1), (4, 100, 10), (0, -1, 10), (0, -5, 0)]
    for sh in (14, 17, 20, 23, 26):
        e = 1 << sh
        for k in (1, 3):
            out += [(0, k * e - 2, 1), (0, k * e - 1, 0), (0, k * e - 1, 1), (0, k * e - 1, 2), (0, k * e, 0), (0, k * e, 1),
                    (0, k * e - 50, 100)]
    top = (1 << 29) - 1
    out += [(0, top - 1, 0), (0, top - 1, 1), (0, top - 1, 2), (0, top, 0), (0, top, 1), (0, top - 100, 200), (0, 0, top),
            (0, 0, top + 1)]
    return out


def build_cases():
    c = Cases()
    rng = c.rng
    # SEQ lengths around the nibble pair and the 16-code chunks, both strands, an N at either end, qualities
    # drawn from all of 33..126
    for m in SEQ_LENGTHS:
        subs = [(0, "N")] if m in (3, 17, 33) else [(m - 1, "N")] if m in (2, 16, 32, 129) else []
        for strand in (0, 1):
            c.single(0, 7, "%dM" % m, strand=strand, subs=subs)
            c.qual = "*"
            c.single(0, 9, "%dM" % m, strand=strand)
        c.unmapped(MH.seq_for(0, 7, "%dM" % m, rng, subs))
        c.qual = "*"
        c.unmapped(MH.seq_for(0, 7, "%dM" % m, rng))
    # l_seq 0: an unmapped empty read with and without a quality, a mapped one
    c.unmapped("")
    c.qual = "*"
    c.unmapped("")
    c.single(0, 7, "", seq="")
    # the quality bytes 33 and 126 at the chunk edges
    for strand in (0, 1):
        c.qual = "!" + "~" * 15 + "!~" + "5" * 14 + "~"
        c.single(0, 100, "33M", strand=strand)
    c.qual = "!"
    c.single(0, 100, "1M")
    c.qual = "~"
    c.unmapped("N")
    c.unmapped("N" * 40)
    # names up to the limit
    for ln in NAME_LENGTHS:
        for strand in (0, 1):
            c.name = "".join(rng.choice("abcXYZ019_:/") for _ in range(ln))
            c.single(0, 50, "40M", strand=strand)
        c.name = "n" * ln
        c.unmapped("ACGTTGCA")
    # CIGAR forms: an X element, an empty CIGAR next to a SEQ, a 0-length element, every op
    c.single(0, 300, "10M1X10M", subs=[(10, None)])
    c.single(0, 50, "", seq=MH.seq_for(0, 50, "30M", rng))
    c.single(0, 50, "10M0I10M")
    c.single(0, 50, "2H3S10M2I5M3D5M10N5M1P5M1X2S")
    # POS 1, 0, negative; a line past its contig's end; "*" and empty RNAME; NM absent
    c.single(0, 1, "40M")
    c.single(0, 0, "40M", strand=1)
    c.single(2, -70, "40M")
    c.single(0, 881, "50M")
    c.single(2, 150, "1M2D3M")
    for chr_ in (-3, -2):
        s = MH.seq_for(0, 10, "30M", rng)
        c._read(s, 0)
        c._hit(chr_, 10, 30, 0, 30, 0, 0, 1, -1, "30M")
        c.lines.append("END")
    s = MH.seq_for(0, 10, "30M", rng)
    c._read(s, 1)
    c._hit(0, 10, 30, 0, 30, -1, 1, 2, -1, "30M")
    c.lines.append("END")
    # two chains of one read (allhits)
    s = MH.seq_for(0, 10, "35M", rng)
    c._read(s, 0)
    c._hit(0, 10, 35, 0, 35, 0, 0, 2, -1, "35M")
    c._hit(1, 3, 35, 0, 35, 2, 0, 2, -1, "30M5S")
    c.lines.append("END")
    # split records (two lines): "=", both strands; qualities cut at matchLength, SEQ at qStart / qEnd, so
    # that QUAL and SEQ differ in length on both lines; no quality; on "*" (RNEXT prints the name) and on
    # the empty name (RNEXT "=")
    full = MH.seq_for(0, 500, "60M", rng) + MH.seq_for(0, 700, "41M", rng)
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (0, 700, 41, 60, 101, 0, 1, "41M"))
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (0, 700, 41, 60, 101, 1, 1, "41M"))
    c.chain(MH.revcomp(full), 1, (0, 500, 55, 0, 60, 1, 1, "60M"), (0, 700, 41, 60, 101, 1, 1, "41M"))
    c.chain(full, 0, (0, 500, 70, 3, 60, 0, 1, "57M"), (0, 700, 41, 61, 101, 0, 1, "40M"))
    c.qual = "*"
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (0, 700, 41, 60, 101, 0, 1, "41M"))
    c.chain(full, 0, (-3, 500, 60, 0, 60, 0, 1, "60M"), (-3, 700, 41, 60, 101, 0, 1, "41M"))
    c.chain(full, 0, (-2, 500, 60, 0, 60, 0, 1, "60M"), (-2, 700, 41, 60, 101, 0, 1, "41M"))
    # the merged one-line forms: list a + S, list a + list b merged at the seam, S + list b merged, POS <= 0
    full = MH.seq_for(0, 500, "60M", rng) + MH.seq_for(1, 10, "40M", rng)
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "55M5S"), (1, 10, 40, 60, 100, 0, 1, "40M"))
    c.chain(full, 0, (0, 500, 60, 0, 60, 0, 1, "60M"), (1, 10, 40, 60, 100, 0, 3, "40M"))
    full = MH.seq_for(2, 20, "40M", rng) + MH.seq_for(0, 600, "60M", rng)
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 1, "38M2S"), (0, 600, 60, 40, 100, 0, 1, "2S28M2D30M"))
    c.chain(MH.revcomp(full), 1, (2, 20, 40, 0, 40, 1, 1, "38M2S"), (0, 600, 60, 40, 100, 1, 1, "2S58M"))
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 1, "40M"), (0, 30, 60, 40, 100, 0, 1, "60M"))
    c.chain(full, 0, (2, 20, 40, 0, 40, 0, 2, "40M"), (0, 600, 60, 40, 100, 0, 1, "5S25M1I29M"))
    # pairs: proper, one mate unmapped, both unmapped, a rescued mate 2 and mate 1, mates on two contigs, one
    # mate without a quality, odd lengths
    a = MH.seq_for(0, 100, "51M", rng, subs=[(3, None)])
    b = MH.seq_for(0, 300, "20M1D30M", rng, subs=[(20, None)])
    d = MH.seq_for(1, 20, "33M", rng)
    c.pair((a, 0, [(0, 100, "51M", 1)]), (b, 1, [(0, 300, "20M1D30M", 1)]))
    c.pair((b, 1, [(0, 300, "20M1D30M", 1)]), (a, 0, [(0, 100, "51M", 1)]))
    c.pair((a, 0, [(0, 100, "51M", 2), (0, 101, "51M", 2)]), (b, 1, []))
    c.pair((a, 1, []), (b, 0, []))
    c.pair((a, 0, [(0, 100, "51M", 1)]), (b, 1, []), rescue=(2, 0, 300, 1, 2, "20M1D30M"))
    c.pair((b, 1, []), (a, 0, [(0, 100, "51M", 1)]), rescue=(1, 0, 300, 1, 2, "20M1D30M"), ins=(10, 100))
    c.pair((a, 0, [(0, 100, "51M", 1)]), (d, 1, [(1, 20, "33M", 1)]))
    c.pair((d, 1, [(1, 20, "33M", 1)]), (b, 0, []))
    return c


def _framed(c, name):
    """one mapped read called `name` after the cases c"""
    c.name = name
    c.single(0, 50, "40M")
    return c


@pytest.fixture(scope="module")
def bam_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_host")
    exe = d / "bam_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-fopenmp", "-I", CSRC] + MH.SAN + [
        "-o", str(exe), os.path.join(HERE, "bam_host.cpp"), os.path.join(CSRC, "host_index.cpp"), os.path.join(CSRC, "sam.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    fasta = d / "g.fa"
    fasta.write_text("".join(">%s\n%s\n" % (FASTA_NAMES[n], s) for n, s in MH.GENOME))
    count = [0]

    def run(case_text, tags):
        """(units [(sam text, bam bytes)], reported lines, header bytes)"""
        count[0] += 1
        base = d / ("run%d" % count[0])
        cases = d / ("cases%d.txt" % count[0])
        cases.write_text(case_text)
        env = dict(os.environ)
        env.update({"OMP_NUM_THREADS": "2", "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1",
                    "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
        outs = [str(base) + x for x in (".sam", ".bam", ".hdr")]
        r = subprocess.run([str(exe), str(fasta), str(cases), str(tags)] + outs, capture_output=True, env=env, timeout=300)
        err = r.stderr.decode(errors="replace")
        for tag in ("Sanitizer", "runtime error"):
            assert tag not in err, err[-6000:]
        assert r.returncode == 0, (r.returncode, err[-4000:])
        sam = open(outs[0], "rb").read().decode("latin-1")
        bam = open(outs[1], "rb").read()
        rep = r.stdout.decode().splitlines()
        units, sa, ba = [], 0, 0
        for l in rep:
            if l.startswith("UNIT "):
                ns, nb = (int(x) for x in l.split()[1:])
                units.append((sam[sa:sa + ns], bam[ba:ba + nb]))
                sa, ba = sa + ns, ba + nb
        assert sa == len(sam) and ba == len(bam)
        return units, rep, open(outs[2], "rb").read()

    return run


@pytest.fixture(scope="module")
def runs(bam_host):
    """the cases of this file and of test_md_host.py, with MD (1) and without (0)"""
    own, md = "\n".join(build_cases().lines) + "\n", MH.build_cases()
    return {tags: (bam_host(own, tags), bam_host(md, tags)) for tags in (0, 1)}


def check_units(units, md):
    n = 0
    for sam, bam in units:
        assert sam.endswith("\n")
        lines = sam.split("\n")[:-1]
        want = [bam_ref.encode_line(l, CONTIG_TABLE, md=md) for l in lines]
        got = bam_ref.records(bam)
        assert [g.hex() for g in got] == [w.hex() for w in want], sam
        for l, g in zip(lines, got):
            assert bam_ref.render(g, CONTIG_TABLE) == bam_ref.normalise(l)
        n += len(lines)
    return n


@pytest.mark.parametrize("tags", [0, 1])
def test_records_equal_the_encoding_of_the_printed_lines(runs, tags):
    (own, rep, _), (mdu, _, _) = runs[tags]
    assert not [l for l in rep if not l.startswith("UNIT ")]
    assert check_units(own, bool(tags)) >= 130  # (133 lines by the count of build_cases)
    assert check_units(mdu, bool(tags)) >= 130
    mdlines = [l for sam, _ in own + mdu for l in sam.split("\n")[:-1] if "\tMD:Z:" in l]
    assert (len(mdlines) >= 200) if tags else not mdlines


def test_md_changes_nothing_but_the_tag(runs):
    """a record with MD is the record without it plus "MDZ<value>NUL", block_size adjusted"""
    for (a, _, _), (b, _, _) in zip(runs[0], runs[1]):
        for (sam0, bam0), (sam1, bam1) in zip(a, b):
            for l1, r0, r1 in zip(sam1.split("\n")[:-1], bam_ref.records(bam0), bam_ref.records(bam1)):
                m = re.search(r"\tMD:Z:([^\t]*)$", l1)
                extra = b"MDZ" + m.group(1).encode() + b"\0" if m else b""
                assert r1[4:] == r0[4:] + extra and len(r1) == len(r0) + len(extra)


def test_cases_are_what_they_claim(runs):
    """the printed lines hold the forms the cases were written for"""
    (own, _, _), _ = runs[1]
    recs = [l.split("\t") for sam, _ in own for l in sam.split("\n")[:-1]]
    cig = [f[5] for f in recs]
    fwd = {len(f[9]) for f in recs if not int(f[1]) & 0x10}
    rev = {len(f[9]) for f in recs if int(f[1]) & 0x10}
    assert fwd >= set(SEQ_LENGTHS) | {0} and rev >= set(SEQ_LENGTHS)
    assert {len(f[0]) for f in recs} >= set(NAME_LENGTHS)
    assert any("N" in f[9] for f in recs) and any(f[9] == "N" * 40 for f in recs)
    assert any(f[10] == "*" and len(f[9]) > 1 for f in recs) and any(f[10] == "*" and len(f[9]) == 1 for f in recs)
    assert any(f[10] != "*" and len(f[10]) != len(f[9]) and int(f[1]) & 0x1 for f in recs)  # a split record's QUAL
    assert any("!" in f[10] and "~" in f[10] for f in recs)
    assert "10M1X10M" in cig and "" in cig and "55M45S" in cig and "38M4S28M2D30M" in cig and "45S25M1I29M" in cig
    assert "60M40S" in cig and "2H3S10M2I5M3D5M10N5M1P5M1X2S" in cig
    assert {"1", "0"} <= {f[3] for f in recs} and any(int(f[3]) < 0 for f in recs)
    assert any(f[2] == "*" and not int(f[1]) & 0x4 for f in recs) and any(f[2] == "" for f in recs)
    assert any(f[2] == "c1" and int(f[3]) + 49 > 900 for f in recs)  # past the contig's end
    split = [f for f in recs if int(f[1]) & 0x41 == 0x41 and not int(f[1]) & 0x80 and f[7] != "0"]
    assert any(f[6] == "=" for f in split) and any(f[6] == "*" for f in split)
    pairs = [f for f in recs if int(f[1]) & 0xC0 and int(f[1]) & 0x1 and f[5] != ""]
    assert any(int(f[1]) & 0x2 for f in pairs) and any(int(f[1]) & 0x8 and not int(f[1]) & 0x4 for f in pairs)
    assert any(int(f[1]) & 0xC == 0xC for f in pairs)
    assert any(f[6] not in ("=", "*") for f in pairs)  # mates on two contigs
    assert any("NM:i:" not in "\t".join(f) and "X0:i:" in "\t".join(f) for f in recs)
    assert any("MD:Z:" in "\t".join(f) for f in recs)


def test_literal_record(bam_host):
    """one record worked by hand from the specification, not through bam_ref"""
    c = Cases()
    c.name, c.qual = "q", "!5~"
    c.single(0, 3, "3M", seq="ACN")
    (units, _, _) = bam_host("\n".join(c.lines) + "\n", 0)
    sam, bam = units[0]
    assert sam == "q\t66\tc1\t3\t1\t3M\t*\t0\t0\tACN\t!5~\tNM:i:0\tXP:Z:U\tX0:i:1\n"
    want = (bytes([62, 0, 0, 0]) + bytes([0, 0, 0, 0]) + bytes([2, 0, 0, 0]) + bytes([2, 1]) + bytes([0x49, 0x12]) +
            bytes([1, 0]) + bytes([66, 0]) + bytes([3, 0, 0, 0]) + b"\xff\xff\xff\xff" * 2 + bytes([0, 0, 0, 0]) + b"q\0" +
            bytes([0x30, 0, 0, 0]) + bytes([0x12, 0xF0]) + bytes([0, 20, 93]) + b"NMi\0\0\0\0" + b"XPZU\0" + b"X0i\1\0\0\0")
    assert bam.hex() == want.hex()


def test_a_255_byte_name_is_refused(bam_host):
    c = _framed(Cases(), "k" * 254)
    _framed(c, "k" * 255)
    c.name = "k" * 300
    c.pair(("ACGTACGT", 0, []), ("ACGTACGA", 0, []))
    units, rep, _ = bam_host("\n".join(c.lines) + "\n", 0)
    assert len(units) == 1 and [l for l in rep if not l.startswith("UNIT ")] == ["LONGNAME 255", "LONGNAME 300"]
    with pytest.raises(ValueError):
        bam_ref.encode_line("k" * 255 + "\t4\t*\t0\t1\t\t*\t0\t0\tA\t*", CONTIG_TABLE)


def test_bin(bam_host):
    cases = _bin_cases()
    c = Cases()
    for b in cases:
        c.bin(*b)
    _, rep, _ = bam_host("\n".join(c.lines) + "\n", 0)
    want = []
    for flag, beg, reflen in cases:
        want.append(bam_ref.BIN_UNMAPPED if flag & 4 or beg < 0 else bam_ref.reg2bin(beg, beg + max(reflen, 1)) & 0xFFFF)
    assert rep == ["BIN %d" % w for w in want]
    # the specification's levels, by hand: the first bin of each and an interval across a 16 kb edge
    assert bam_ref.reg2bin(0, 1) == 4681 and bam_ref.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585
    assert bam_ref.reg2bin(0, 1 << 29) == 0 and bam_ref.reg2bin(-1, 0) == 4680 == bam_ref.BIN_UNMAPPED
    assert bam_ref.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767


def test_header(runs):
    hdr = runs[0][0][2]
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIG_TABLE)
    assert hdr == bam_ref.header(CONTIG_TABLE, text)
    assert bam_ref.parse_header(hdr) == (text, CONTIG_TABLE, len(hdr))
    assert hdr[:4] == b"BAM\1" and hdr.endswith(b"\3\0\0\0c3\0" + (150).to_bytes(4, "little"))
