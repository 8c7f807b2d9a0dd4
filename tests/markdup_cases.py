"""The hand-written record streams of the duplicate-marking tests (include/gwa.h "Duplicate marking"), shared by
test_markdup_host.py (the host build under sanitizers) and test_gpu_markdup.py (the device through
gwa_bam_sorter_add_records).  Every case is a list of runs [(run id, [record bytes])] on CONTIGS; the records
come from bam_ref.encode_line."""
import random
import struct

import bai_ref
import bam_ref

CONTIGS = [("c1", 1 << 29), ("c2", 300000), ("c3", 1000)]
SLICE = bai_ref.SLICE
QUERY_OPS = "MIS=X"


def rec(name, flag, rname, pos, cigar, quals=None, lseq=None):
    """pos: 0-based.  quals: raw quality bytes (any value 0..255), default 30s; l_seq follows the CIGAR unless
    lseq is given"""
    ops = bam_ref.parse_cigar(cigar)
    if lseq is None:
        lseq = sum(n for n, op in ops if op in QUERY_OPS) if quals is None else len(quals)
    if quals is None:
        quals = bytes([30]) * lseq
    assert len(quals) == lseq
    line = "%s\t%d\t%s\t%d\t1\t%s\t*\t0\t0\t%s\t%s" % (name, flag, rname, pos + 1, cigar or "*", "A" * lseq, "I" * lseq)
    r = bytearray(bam_ref.encode_line(line, CONTIGS))
    lname, ncig = r[12], struct.unpack_from("<H", r, 16)[0]
    at = 36 + lname + 4 * ncig + (lseq + 1) // 2
    r[at:at + lseq] = quals
    assert at + lseq == len(r)
    return bytes(r)


def sized(size, pos, rname="c2", flag=0):
    """a mapped record of exactly `size` bytes at pos"""
    for nl in range(1, 12):
        for l in range(1, size):
            if 36 + nl + 1 + 4 + (l + 1) // 2 + l == size:
                r = rec("n" * nl, flag, rname, pos, "%dM" % l)
                assert len(r) == size
                return r
    raise AssertionError(size)


U5_CIGARS = ["20M", "5S20M", "20M5S", "3H5S20M4S2H", "2H20M3H", "5S10M2I3D4N6=7X2H", "4S6M1I3M2D5M3N4M6S", "", "7S", "3H4S",
             "1S1M1S"]


def u5_case():
    """both strands over every CIGAR shape, pos -1 and -6, and a reverse pair of records whose indel moves pos
    while u5 agrees"""
    recs = []
    for ci, cg in enumerate(U5_CIGARS):
        for flag in (0, 16):
            for pos in (1000 + 100 * ci, -1, -6):
                recs.append(rec("u%d" % len(recs), flag, "c2", pos, cg, lseq=0 if cg == "" else None))
    recs.append(rec("indelA", 16, "c1", 100, "30M", bytes([40]) * 30))
    recs.append(rec("indelB", 16, "c1", 98, "10M2D20M", bytes([20]) * 30))
    recs.append(rec("wrap", 0, "c1", -(1 << 31), "5S3M"))  # u5 below -2^31: taken mod 2^32
    return [(0, recs)]


def u5_by_hand():
    """[(record, u5)] worked out by hand from the rule"""
    return [(rec("a", 0, "c2", 1000, "3H5S20M4S2H"), 992), (rec("a", 16, "c2", 1000, "3H5S20M4S2H"), 1025),
            (rec("a", 16, "c2", 1000, "5S10M2I3D4N6=7X2H"), 1031), (rec("a", 0, "c2", -6, "5S20M"), -11),
            (rec("a", 16, "c2", -6, "", lseq=0), -6), (rec("a", 16, "c2", 50, "7S"), 56), (rec("a", 0, "c2", 50, "7S"), 43),
            (rec("a", 16, "c1", 98, "10M2D20M"), 129), (rec("a", 16, "c1", 100, "30M"), 129)]


def qual_case():
    """l_seq at the edges of the 16-byte pieces under names of 1-16 bytes: the quality starts at every offset
    mod 16; bytes 14 / 15 / 93 / 94 / 0xFF among ordinary ones, all 0xFF, all 14"""
    rng = random.Random(7)
    recs, pos = [], 10
    for lseq in (0, 1, 15, 16, 17, 255, 256, 257, 512):
        for nl in range(1, 17):
            q = bytes(rng.choice((14, 15, 93, 94, 0xFF, 0, 200, rng.randrange(16, 93))) for _ in range(lseq))
            pos += 7
            recs.append(rec("q" * nl, rng.choice((0, 16)), "c2", pos, "%dM" % lseq if lseq else "", q))
    for nl in (3, 8):
        for lseq in (16, 33, 257):
            for fill in (0xFF, 14, 15, 93):
                pos += 7
                recs.append(rec("f" * nl, 0, "c2", pos, "%dM" % lseq, bytes([fill]) * lseq))
    # (several runs: a run's last record ends where its buffer ends)
    return [(i, recs[i::5]) for i in range(5)]


def _pe(name, f1, f2, p1, p2, c1="30M", c2="30M", q1=30, q2=30, ref1="c2", ref2="c2"):
    return [rec(name, f1, ref1, p1, c1, bytes([q1]) * sum(n for n, o in bam_ref.parse_cigar(c1) if o in QUERY_OPS)),
            rec(name, f2, ref2, p2, c2, bytes([q2]) * sum(n for n, o in bam_ref.parse_cigar(c2) if o in QUERY_OPS))]


def pairing_case():
    long_a, long_b = "L" * 40, "M" * 200
    runs = [
        (0, [rec("abcx", 0x41, "c2", 100, "30M"), rec("abcy", 0x91, "c2", 300, "30M")]),   # names differ in the last byte
        (1, [rec("abc", 0x41, "c2", 100, "30M"), rec("abcd", 0x91, "c2", 300, "30M")]),    # ... in length
        (2, [rec("s", 0x41, "c2", 100, "30M"), rec("s", 0x51, "c2", 300, "30M")]),         # 0x40 then 0x40
        (3, [rec("t", 0x81, "c2", 100, "30M"), rec("t", 0x51, "c2", 300, "30M")]),         # 0x80 first
        (4, _pe("h", 0x49, 0x85, 100, 100, c2="", q2=40)),                                  # one mate 0x4
        (5, _pe("h2", 0x4D, 0x8D, 100, 100)),                                               # both 0x4
        (6, [rec("v", 0x41, "c2", 100, "30M"), rec("v", 0x941, "c2", 5000, "10M20H"), rec("v", 0x141, "c2", 7000, "30M"),
             rec("v", 0x91, "c2", 300, "30M")]),                                            # 0x800 / 0x100 in between
        (7, [rec("x", 0, "c2", 50, "30M"), rec("cut", 0x41, "c2", 100, "30M")]),           # a pair cut across two runs
        (8, [rec("cut", 0x91, "c2", 300, "30M"), rec("y", 0, "c2", 60, "30M")]),
        (9, [rec("sp", 0x41, "c2", 100, "20M10S"), rec("sp", 0x81, "c1", 9000, "20S10M")]),  # the pieces of a split read
        (10, []),
        (11, [rec("one", 0x41, "c2", 100, "30M")]),
        (12, _pe("two", 0x41, 0x91, 100, 300)),
        (13, _pe(long_a, 0x41, 0x91, 100, 300) + _pe(long_b, 0x41, 0x91, 100, 300) +
             [rec(long_a, 0x41, "c2", 100, "30M"), rec(long_a[:17] + "x" + long_a[18:], 0x91, "c2", 300, "30M"),
              rec(long_b, 0x41, "c2", 100, "30M"), rec(long_b[:150] + "x" + long_b[151:], 0x91, "c2", 300, "30M"),
              rec(long_b, 0x41, "c2", 100, "30M"), rec(long_b[:-1] + "x", 0x91, "c2", 300, "30M"),
              rec("p", 0x41, "c2", 100, "30M"), rec("p", 0x91, "c2", 300, "30M"), rec("p", 0x91, "c2", 300, "30M")]),
    ]
    return runs


def decision_case():
    """run ids 0 .. 4; the test adds them in reversed order too"""
    r0, r1, r2, r3, r4 = [], [], [], [], []
    # pair groups of 2 and of 5, distinct scores, the best one neither first nor last
    for i, q in enumerate((20, 35)):
        r0 += _pe("g2_%d" % i, 0x61, 0x91, 1000, 1200, q1=q, q2=q)
    for i, q in enumerate((20, 25, 40, 30, 22)):
        (r0, r1, r2, r3, r4)[i].extend(_pe("g5_%d" % i, 0x61, 0x91, 2000, 2300, q1=q, q2=q))
    # FR against RF at the same coordinates: not duplicates; mates swapped: duplicates
    r1 += _pe("fr", 0x61, 0x91, 3000, 3200) + _pe("rf", 0x51, 0xA1, 3000 - 29, 3200 + 29)
    r1 += _pe("sw1", 0x61, 0x91, 4000, 4200, q1=33, q2=33) + _pe("sw2", 0x51, 0xA1, 4200, 4000, q1=31, q2=31)
    # a score tie inside a run and one across runs: the lowest ordinal stays
    r2 += _pe("tie_a", 0x61, 0x91, 5000, 5200) + _pe("tie_b", 0x61, 0x91, 5000, 5200)
    r1 += _pe("xt_1", 0x61, 0x91, 6000, 6200)
    r3 += _pe("xt_3", 0x61, 0x91, 6000, 6200)
    r0 += _pe("xt_0", 0x61, 0x91, 6000, 6200, q1=29, q2=31)  # (the sum ties too)
    # soft clips: the same unclipped ends from other pos
    r2 += _pe("clip_a", 0x61, 0x91, 7000, 7200, q1=45, q2=45) + _pe("clip_b", 0x61, 0x91, 7004, 7190, c1="4S26M", c2="30M10S")
    # both mates on one strand at one coordinate: the two end keys are equal
    for i, q in enumerate((21, 23, 22)):
        (r0, r2, r4)[i].extend(_pe("eq_%d" % i, 0x41, 0x81, 8000, 8000, q1=q, q2=q))
    # fragments: a group among fragments, and one at a pair's end (all duplicates, whatever their score)
    r3 += [rec("fa", 0, "c2", 9000, "30M", bytes([20]) * 30), rec("fb", 0, "c2", 9000, "30M", bytes([40]) * 30),
           rec("fc", 0, "c2", 9003, "3S27M", bytes([40]) * 30), rec("fd", 16, "c2", 9000, "30M", bytes([10]) * 30)]
    r4 += [rec("pe_f1", 0, "c2", 1000, "30M", bytes([93]) * 30), rec("pe_f2", 16, "c2", 2300, "30M", bytes([93]) * 30),
           rec("pe_f3", 0, "c2", 1000, "30M", bytes([93]) * 30)]
    # a fragment from a half-mapped pair (its unmapped mate has coordinates) against plain fragments
    r3 += _pe("half", 0x49, 0x85, 10000, 10000, c2="", q1=35, q2=50) + [rec("plain", 0, "c2", 10000, "30M", bytes([36]) * 30)]
    r4 += [rec("plain2", 0, "c2", 10000, "30M", bytes([34]) * 30)]
    # refID -1 with coordinates, secondary and supplementary records at a duplicate's place: never marked
    r4 += [rec("star", 0, "*", 9000, "30M"), rec("star2", 0, "*", 9000, "30M"), rec("sec", 0x100, "c2", 9000, "30M"),
           rec("sup", 0x800, "c2", 9000, "30M"), rec("unm", 0x4, "c2", 9000, "")]
    # the same key on another contig is another key
    r4 += [rec("other", 0, "c1", 9000, "30M")]
    return [(0, r0), (1, r1), (2, r2), (3, r3), (4, r4)]


def edge_case():
    """Runs whose sorted stream has a marked record with byte 19 (FLAG's high byte) as the first byte of a
    slice, and another with it as the last byte of a slice.  Returns (runs, [stream offsets of the two])."""
    keep = [rec("k1", 0, "c2", 10, "40M", bytes([40]) * 40), rec("k2", 0, "c2", 20, "40M", bytes([40]) * 40)]
    dups = [rec("d1", 0, "c2", 100010, "100000H40M", bytes([20]) * 40), rec("d2", 0, "c2", 200020, "200000H40M", bytes([20]) * 40)]
    out, at, pos = list(keep), sum(map(len, keep)), 1000
    starts = []
    for d, target in zip(dups, (SLICE - 19, 3 * SLICE - 20)):
        while target - at > 400:
            out.append(sized(100, pos))
            at += 100
            pos += 10
        gap = target - at
        assert gap >= 120
        out += [sized(60, pos), sized(gap - 60, pos + 10)]
        pos = 100010 + 10
        at = target
        starts.append(at)
        out.append(d)
        at += len(d)
    out += [sized(100, 250000 + i) for i in range(30)]
    runs = [(0, out[::3]), (1, out[1::3]), (2, out[2::3])]
    return runs, starts


def world_case(seed=5):
    """about 900 records on two contigs in several runs: pairs, fragments and half-mapped pairs, a third of them
    copies of earlier templates under new names and other qualities, placed anywhere in the stream"""
    rng = random.Random(seed)
    temps = []

    def template(i, src=None):
        name = "w%d" % i
        if src is None:
            kind = rng.choice(("pair", "pair", "frag", "half"))
            c = rng.choice(("c1", "c2"))
            p1 = rng.randrange(0, 20000)
            l1, l2 = rng.randrange(30, 120), rng.randrange(30, 120)
            src = (kind, c, p1, p1 + rng.randrange(50, 400), l1, l2, rng.random() < 0.5)
        kind, c, p1, p2, l1, l2, flip = src
        q1 = bytes(rng.choice((rng.randrange(2, 60), 30)) for _ in range(l1))
        q2 = bytes(rng.choice((rng.randrange(2, 60), 30)) for _ in range(l2))
        if rng.random() < 0.3:
            q1, q2 = bytes([30]) * l1, bytes([30]) * l2  # (score ties)
        if kind == "frag":
            recs = [rec(name, 16 if flip else 0, c, p1, "%dM" % l1, q1)]
        elif kind == "half":
            recs = [rec(name, 0x49 | (0x10 if flip else 0), c, p1, "%dM" % l1, q1), rec(name, 0x85, c, p1, "", q2)]
        else:
            f1, f2 = (0x61, 0x91) if not flip else (0x51, 0xA1)
            a, b = (p1, p2) if not flip else (p2, p1)
            recs = [rec(name, f1, c, a, "%dM" % l1, q1), rec(name, f2, c, b, "%dM" % l2, q2)]
        return src, recs

    for i in range(600):
        if temps and rng.random() < 0.34:
            src = rng.choice(temps)[0]
            if src[0] == "pair" and rng.random() < 0.3:  # a fragment at the pair's first end
                src = (rng.choice(("frag", "half")), src[1], src[3] if src[6] else src[2], 0, src[4], src[5], src[6])
            temps.append(template(i, src))
        else:
            temps.append(template(i))
    runs, at, rid = [], 0, 0
    while at < len(temps):
        n = rng.choice((1, 40, 97, 150))
        runs.append((rid, [r for _, recs in temps[at:at + n] for r in recs]))
        at += n
        rid += 1 + rng.randrange(3)
    return runs
