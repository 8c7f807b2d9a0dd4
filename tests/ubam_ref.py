"""BAM as read input, in pure Python: the reference the decoder (csrc/bam_in_core.h, csrc/bam_in.hip) and the
framing of csrc/record_stream.cpp are tested against, restating include/gwa.h "BAM input".

A record writer that can produce any record (every flag, name, all 16 base codes, a quality, none, CIGAR and
tag filler, and field values that contradict each other), reads_of -- the contract: names to the first NUL,
SEQ letters with FLAG 0x10 reverse-complemented back, quality + 33 or None, 0x100 / 0x800 records skipped,
errors with the record's index and byte offset --, fastq_of, and a file writer on inflate_ref.cut_members
and bam_ref.header.  The test cases of tests/test_bam_in_host.py and tests/test_gpu_bam_in.py are listed here
once (cases, malformed)."""
import random
import struct

import bam_ref
import inflate_ref

LETTERS = "=ACMGRSVTWYHKDBN"
COMP = str.maketrans("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN")
SKIP = 0x100 | 0x800


class UbamError(Exception):
    pass


def revcomp(s):
    return s[::-1].translate(COMP)


def record(name, seq, qual, flag=4, cigar=(), tags=b"", l_read_name=None, block_size=None, nul=True, l_seq=None):
    """One alignment record from its stored fields.  name: bytes without the NUL; seq: letters of LETTERS as
    stored; qual: None (0xFF bytes), a str of printable characters, or the stored bytes; cigar: u32 values;
    l_read_name, l_seq and block_size override the computed values; nul=False leaves the name's NUL out."""
    name = name.encode("latin-1") if isinstance(name, str) else name
    nm = name + (b"\0" if nul else b"")
    nib = [LETTERS.index(c) for c in seq] + [0]
    packed = bytes(nib[2 * i] << 4 | nib[2 * i + 1] for i in range((len(seq) + 1) // 2))
    if qual is None:
        q = b"\xff" * len(seq)
    elif isinstance(qual, str):
        q = bytes(ord(c) - 33 for c in qual)
    else:
        q = bytes(qual)
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm) if l_read_name is None else l_read_name, 0, 4680, len(cigar), flag,
                       len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", c) for c in cigar) + packed + q + tags
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def read_record(name, seq, qual, flag=4, **kw):
    """the record of a read: with FLAG 0x10 the stored SEQ is its reverse complement and the quality reversed"""
    if flag & 0x10:
        seq = revcomp(seq)
        qual = qual[::-1] if qual is not None else None
    return record(name, seq, qual, flag, **kw)


def _label(index, at):
    return "BAM record %d at byte %d: " % (index, at)


def walk(data, index0=0, byte0=0):
    """[(offset, flag)] of every record of the chain, which must end exactly at len(data)"""
    out, at = [], 0
    while at < len(data):
        lab = _label(index0 + len(out), byte0 + at)
        if len(data) - at < 4:
            raise UbamError(lab + "the chain of block_size fields ends %d bytes before the data's end" % (len(data) - at))
        bs, = struct.unpack_from("<I", data, at)
        if bs < 32:
            raise UbamError(lab + "block_size %d is below the 32 fixed bytes" % bs)
        if bs + 4 > len(data) - at:
            raise UbamError(lab + "block_size %d runs past the data's end (%d bytes)" % (bs, byte0 + len(data)))
        lname, ncig, flag, lseq = data[at + 12], *struct.unpack_from("<HHI", data, at + 16)
        if lname > bs - 32:
            raise UbamError(lab + "the read name (%d bytes) runs past the record" % lname)
        if lname + 4 * ncig > bs - 32:
            raise UbamError(lab + "the CIGAR (%d elements) runs past the record" % ncig)
        if lname + 4 * ncig + (lseq + 1) // 2 + lseq > bs - 32:
            raise UbamError(lab + "SEQ and QUAL (l_seq %d) run past the record" % lseq)
        out.append((at, flag))
        at += bs + 4
    return out


def kept_starts(data):
    """the offsets of the records that are reads, and the number of all records"""
    w = walk(data)
    return [at for at, flag in w if not flag & SKIP], len(w)


def reads_of(data, index0=0, byte0=0):
    """[(name, seq, qual or None)] of headerless records: the contract of include/gwa.h "BAM input".  The chain
    is validated first; then the lowest record with a content error is reported."""
    reads = []
    for k, (at, flag) in enumerate(walk(data, index0, byte0)):
        if flag & SKIP:
            continue
        lab = _label(index0 + k, byte0 + at)
        lname, ncig, _, lseq = data[at + 12], *struct.unpack_from("<HHI", data, at + 16)
        if lname == 0:
            raise UbamError(lab + "l_read_name is 0 (a read name holds at least its NUL)")
        nm = data[at + 36:at + 36 + lname]
        if b"\0" not in nm:
            raise UbamError(lab + "the read name has no NUL inside its l_read_name %d bytes" % lname)
        s0 = at + 36 + lname + 4 * ncig
        q0 = s0 + (lseq + 1) // 2
        seq = "".join(LETTERS[data[s0 + i // 2] >> 4 if i % 2 == 0 else data[s0 + i // 2] & 15] for i in range(lseq))
        q = data[q0:q0 + lseq]
        if lseq > 0 and q[0] == 0xFF:
            qual = None
        else:
            for i, b in enumerate(q):
                if b > 93:
                    raise UbamError(lab + "quality byte %d is %d (at most 93 prints as SAM QUAL)" % (i, b))
            qual = "".join(chr(b + 33) for b in q)
        if flag & 0x10:
            seq, qual = revcomp(seq), (qual[::-1] if qual is not None else None)
        reads.append((nm[:nm.index(b"\0")].decode("latin-1"), seq, qual))
    return reads


def fastq_of(reads):
    """the FASTQ text of reads that all have a quality"""
    assert all(q is not None for _, _, q in reads)
    return "".join("@%s\n%s\n+\n%s\n" % r for r in reads).encode("latin-1")


def bam_bytes(records, text="", contigs=()):
    """an inflated BAM: header and records"""
    return bam_ref.header(list(contigs), text) + records


def bam_file(records, text="", contigs=(), seed=1, lo=300, hi=4000, eof=True):
    """a BAM file whose BGZF members hold lo..hi inflated bytes each, so that the header and the records
    straddle them"""
    return inflate_ref.cut_members(bam_bytes(records, text, contigs), seed=seed, lo=lo, hi=hi, eof=eof)


# ---- the test cases --------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 129, 512)


def _rand_read(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n)), "".join(chr(33 + rng.randrange(94)) for _ in range(n))


def random_records(n, seed=7, max_len=150):
    """about n random records: both strands, all codes now and then, absent qualities, skipped records, names
    with blanks, CIGAR and tag filler"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.choice((rng.randrange(0, 40), rng.randrange(90, max_len), 100, 100))
        seq, qual = _rand_read(rng, ln, LETTERS if rng.random() < 0.1 else "ACGTN")
        flag = rng.choice((4, 4, 4 | 0x10, 0x10, 0, 0x4D, 0x8D | 0x10, 4 | 0x100, 0x800, 0x900 | 0x10))
        name = "r%d%s" % (i, rng.choice(("", "", " x y", "/1", "\tz" * rng.randrange(3))))
        out.append(read_record(name, seq, None if rng.random() < 0.15 else qual, flag,
                               cigar=[rng.randrange(1 << 32) for _ in range(rng.randrange(6))],
                               tags=bytes(rng.randrange(256) for _ in range(rng.randrange(41)))))
    return b"".join(out)


def cases():
    """[(name, headerless records)]: the well-formed inputs"""
    rng = random.Random(5)
    out = [("empty", b"")]
    for ln in LENGTHS:
        for flag in (4, 4 | 0x10):
            seq, qual = _rand_read(rng, ln, "ACGTN")
            out.append(("len%d_flag%d" % (ln, flag), read_record("l%d" % ln, seq, qual, flag)))
    for k in range(16):  # every code at an even and at an odd position, on both strands
        for flag in (0, 0x10):
            seq = "A" * 4 + LETTERS[k] + "C" * 4 + LETTERS[k] + "G" * 7
            assert seq[4] == seq[9]
            out.append(("code%d_flag%d" % (k, flag), record("c", seq, "I" * len(seq), flag)))
    for nl in (0, 1, 16, 17, 254):
        out.append(("name%d" % nl, read_record("n" * nl, "ACGTACGTAC", "ABCDEFGHIJ", 4 | 0x10)))
    out.append(("name_blanks", read_record("a b\tc /1", "ACGT", "IIII")))
    out.append(("name_second_nul", record(b"ab\0cd", "ACGT", "IIII")))  # the bytes before the first NUL
    for ncig in range(6):  # the packed SEQ at every offset mod 16, and more
        for tl in (0, 1, 7, 40):
            for nl in range(1, 5):
                seq, qual = _rand_read(rng, 37, "ACGT")
                out.append(("cig%d_tags%d_name%d" % (ncig, tl, nl),
                            read_record("x" * nl, seq, qual, 0x10 if (ncig + nl) % 2 else 0,
                                        cigar=[(37 << 4) | 0] * ncig, tags=bytes(range(tl)))))
    out.append(("qual_0_93", record("q", "ACGTACGTACGTACGTAC", bytes([0, 93] * 9))))
    out.append(("qual_0_93_rev", record("q", "ACGTACGTACGTACGTAC", bytes([0, 93] * 9), 0x10)))
    out.append(("qual_absent", record("q", "ACGTA", None)))
    out.append(("qual_absent_rest_arbitrary", record("q", "ACGTA", b"\xff\x00\x5e\xff\x01", 0x10)))
    out.append(("qual_mixed", record("a", "ACGT", None) + record("b", "ACGT", "IIII") + record("c", "AC", None, 0x10)
                + record("d", "ACGTT", "ABCDE", 0x10)))
    out.append(("lseq0_byte_follows", record("z", "", "", tags=b"\xff\x07")))
    r = lambda n, f=4: read_record(n, "ACGTTGCA", "IIIIHHHH", f)  # noqa: E731
    out.append(("skip_front", r("s", 0x100) + r("a") + r("b")))
    out.append(("skip_middle", r("a") + r("s", 0x800) + r("b")))
    out.append(("skip_end", r("a") + r("b") + r("s", 0x900)))
    out.append(("skip_run", r("a") + r("s", 0x100) + r("t", 0x800 | 0x10) + r("u", 0x100) + r("b") + r("v", 0x800)))
    out.append(("skip_all", r("s", 0x100) + r("t", 0x800)))
    out.append(("random2000", random_records(2000)))
    return out


def malformed():
    """[(name, headerless records, the exact message)]; the bad record is record 2, behind a read and a skipped
    record, so its index counts all records"""
    good = read_record("g", "ACGTACGT", "IIIIIIII")
    skipped = read_record("s", "ACGT", "IIII", 0x100)
    pre = good + skipped
    at = len(pre)
    lab = _label(2, at)
    base = record("bad", "ACGTACGTACGTACGTAC", "I" * 18)
    out = []

    def add(name, rec, what, tail=good):
        out.append((name, pre + rec + tail, lab + what))

    add("block_size_31", record("bad", "", "", block_size=31), "block_size 31 is below the 32 fixed bytes")
    need = len(base) - 4
    add("block_size_one_short", record("bad", "ACGTACGTACGTACGTAC", "I" * 18, block_size=need - 1),
        "SEQ and QUAL (l_seq 18) run past the record")
    add("l_read_name_0", record(b"", "ACGT", "IIII", l_read_name=0, nul=False), "l_read_name is 0 (a read name holds at least its NUL)")
    add("name_without_nul", record(b"abcd", "ACGT", "IIII", nul=False),
        "the read name has no NUL inside its l_read_name 4 bytes")
    add("quality_94", record("bad", "ACGTACGTACGTACGTAC", bytes([0] * 16 + [94, 0])), "quality byte 16 is 94 (at most 93 prints as SAM QUAL)")
    add("quality_94_reverse", record("bad", "ACGTACGTACGTACGTAC", bytes([0, 94] + [0] * 16), 0x10),
        "quality byte 1 is 94 (at most 93 prints as SAM QUAL)")
    add("quality_ff_not_first", record("bad", "ACGTA", b"\x00\xff\xff\xff\xff"), "quality byte 1 is 255 (at most 93 prints as SAM QUAL)")
    whole = pre + base
    out.append(("chain_one_short", whole[:-1], lab + "block_size %d runs past the data's end (%d bytes)" % (need, len(whole) - 1)))
    out.append(("chain_one_long", whole + b"\x07",
                _label(3, len(whole)) + "the chain of block_size fields ends 1 bytes before the data's end"))
    return out
