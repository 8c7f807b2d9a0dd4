"""A plain restatement of the BAM contract of include/gwa.h in Python (no pysam, no samtools): the record
of one printed SAM line written from the SAM specification's tables (section 4.2 layout, section 5.3
reg2bin), the header, and a decoder that renders records back as SAM lines.  Shared by test_bam_host.py (CPU)
and test_gpu_bam.py.  Not derived from csrc/bam_core.h."""
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"                      # SAM specification 4.2: op codes 0..8
BASE_CODE = {"=": 0, "A": 1, "C": 2, "M": 3, "G": 4, "R": 5, "S": 6, "V": 7, "T": 8, "W": 9, "Y": 10, "H": 11,
             "K": 12, "D": 13, "B": 14, "N": 15}
BASE_OF = "=ACMGRSVTWYHKDBN"
BIN_UNMAPPED = 4680                          # reg2bin(-1, 0)
EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0,
             0, 0, 0, 0, 0, 0, 0, 0])
NAME_MAX = 254


def reg2bin(beg, end):
    """SAM specification 5.3: the bin of the zero-based half-open interval [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def parse_cigar(text):
    """[(length, op letter)] of a printed CIGAR ("" and "*": none)"""
    out, num = [], ""
    if text in ("", "*"):
        return out
    for ch in text:
        if ch.isdigit() or (ch == "-" and not num):
            num += ch
        else:
            assert ch in CIGAR_OPS and num not in ("", "-"), text
            out.append((int(num), ch))
            num = ""
    assert num == "", text
    return out


def _ref_id(name, contigs):
    if name in ("*", ""):
        return -1
    names = [c[0] for c in contigs]
    return names.index(name) if name in names else -1


def _u32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


def encode_line(sam_line, contigs, md=False):
    """The record of one printed SAM line (without its newline).  contigs: [(name, length)] as the header
    lists them.  md: the batch was formatted with GWA_SAM_TAG_MD (an MD:Z the line carries is stored)."""
    f = sam_line.split("\t")
    assert len(f) >= 11, sam_line
    qname, flag, rname, pos, _mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if len(qname.encode()) > NAME_MAX:
        raise ValueError("a name of %d bytes" % len(qname.encode()))
    flag, pos, pnext, tlen = int(flag), int(pos), int(pnext), int(tlen)
    ref = _ref_id(rname, contigs)
    if rnext == "=":
        nref, npos = ref, pnext - 1
    elif rnext == "*":
        nref, npos = -1, -1
    else:
        nref, npos = _ref_id(rnext, contigs), pnext - 1
    ops = parse_cigar(cigar)
    reflen = sum(n for n, op in ops if op in "MDNX")
    beg = pos - 1
    if flag & 0x4 or beg < 0:
        bin_ = BIN_UNMAPPED
    else:
        bin_ = reg2bin(beg, beg + max(reflen, 1)) & 0xFFFF
    name = qname.encode() + b"\0"
    lseq = len(seq)
    packed = bytearray((lseq + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= BASE_CODE[ch] << (4 if i % 2 == 0 else 0)
    q = qual.encode("latin-1")
    quals = bytes((c - 33) & 0xFF for c in q) if len(q) == lseq else b"\xff" * lseq
    tags = b""
    for t in f[11:]:
        key, typ, val = t.split(":", 2)
        if key in ("NM", "X0"):
            assert typ == "i"
            tags += key.encode() + b"i" + struct.pack("<i", int(val))
        elif key == "XP" or (key == "MD" and md):
            assert typ == "Z"
            tags += key.encode() + b"Z" + val.encode() + b"\0"
        else:
            assert key == "MD", t
    body = (_u32(ref) + _u32(beg) + struct.pack("<BBHHHI", len(name), 1, bin_, len(ops), flag, lseq) + _u32(nref) +
            _u32(npos) + _u32(tlen) + name + b"".join(_u32(n << 4 | CIGAR_OPS.index(op)) for n, op in ops) +
            bytes(packed) + quals + tags)
    return _u32(len(body)) + body


def encode_text(sam_text, contigs, md=False):
    """the records of every line of a SAM text without header lines"""
    return b"".join(encode_line(l, contigs, md) for l in sam_text.split("\n")[:-1])


def header(contigs, text):
    """The uncompressed BAM header: magic, the header text, the contig table"""
    t = text.encode()
    out = b"BAM\1" + _u32(len(t)) + t + _u32(len(contigs))
    for name, length in contigs:
        n = name.encode() + b"\0"
        out += _u32(len(n)) + n + _u32(length)
    return out


def contigs_of(sam_header_text):
    """[(name, length)] of the @SQ lines"""
    out = []
    for l in sam_header_text.splitlines():
        if l.startswith("@SQ\tSN:"):
            name, ln = l[len("@SQ\tSN:"):].rsplit("\tLN:", 1)
            out.append((name, int(ln)))
    return out


# ---- decoding ----

def bgzf_blocks(data):
    """[(compressed size, inflated bytes)] of a run of BGZF blocks, each block checked (header, CRC32, ISIZE)"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        raw = zlib.decompress(data[at + 18:at + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        assert zlib.crc32(raw) == crc and len(raw) == isize
        out.append((bsize, raw))
        at += bsize
    assert at == len(data)
    return out


def inflate(data):
    return b"".join(raw for _, raw in bgzf_blocks(data))


def parse_header(raw):
    """(header text, [(name, length)], offset of the first record) of uncompressed BAM bytes"""
    assert raw[:4] == b"BAM\1"
    lt = struct.unpack_from("<I", raw, 4)[0]
    text = raw[8:8 + lt].decode()
    at = 8 + lt
    nref = struct.unpack_from("<I", raw, at)[0]
    at += 4
    contigs = []
    for _ in range(nref):
        ln = struct.unpack_from("<I", raw, at)[0]
        name = raw[at + 4:at + 4 + ln]
        assert name.endswith(b"\0") and b"\0" not in name[:-1]
        lref = struct.unpack_from("<I", raw, at + 4 + ln)[0]
        contigs.append((name[:-1].decode(), lref))
        at += 8 + ln
    return text, contigs, at


def records(raw, at=0):
    """the records of raw[at:], one bytes object each (block_size included)"""
    out = []
    while at < len(raw):
        n = struct.unpack_from("<I", raw, at)[0]
        assert at + 4 + n <= len(raw), "a record runs past the data"
        out.append(raw[at:at + 4 + n])
        at += 4 + n
    return out


def render(rec, contigs):
    """One record as a SAM line.  Where BAM cannot carry the text: an empty CIGAR, SEQ or QNAME prints "*",
    QUAL prints "*" when 0xFF, RNEXT prints "=" when both contig names are equal and not "*"."""
    ref, pos, lname, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 4)
    at = 36
    name = rec[at:at + lname]
    assert name.endswith(b"\0")
    at += lname
    cig = ""
    for _ in range(ncig):
        v = struct.unpack_from("<I", rec, at)[0]
        cig += "%d%s" % (v >> 4, CIGAR_OPS[v & 15])
        at += 4
    seq = ""
    for i in range(lseq):
        b = rec[at + (i >> 1)]
        seq += BASE_OF[b >> 4 if i % 2 == 0 else b & 15]
    if lseq % 2:
        assert rec[at + (lseq >> 1)] & 15 == 0, "the unused low nibble is not 0"
    at += (lseq + 1) // 2
    q = rec[at:at + lseq]
    at += lseq
    qual = "*" if lseq == 0 or all(c == 0xFF for c in q) else bytes((c + 33) & 0xFF for c in q).decode("latin-1")
    tags = []
    while at < len(rec):
        key, typ = rec[at:at + 2].decode(), chr(rec[at + 2])
        at += 3
        if typ == "i":
            tags.append("%s:i:%d" % (key, struct.unpack_from("<i", rec, at)[0]))
            at += 4
        else:
            assert typ == "Z", typ
            end = rec.index(b"\0", at)
            tags.append("%s:Z:%s" % (key, rec[at:end].decode()))
            at = end + 1
    assert at == len(rec)
    rname = contigs[ref][0] if ref >= 0 else "*"
    rnext = contigs[nref][0] if nref >= 0 else "*"
    if rnext == rname and rnext != "*":
        rnext = "="
    cols = [name[:-1].decode() or "*", str(flag), rname, str(pos + 1), str(mapq), cig or "*", rnext, str(npos + 1),
            str(tlen), seq or "*", qual] + tags
    return "\t".join(cols)


def normalise(sam_line):
    """A printed line as render() gives its record back: "*" for an empty QNAME, CIGAR or SEQ; an empty RNAME
    / RNEXT is "*"; RNEXT "=" when it names RNAME's contig; PNEXT 0 next to RNEXT "*"; QUAL "*" when its
    length is not SEQ's."""
    f = sam_line.split("\t")
    seq = f[9]
    if len(f[10]) != len(seq):
        f[10] = "*"
    if seq == "":
        f[9], f[10] = "*", "*"
    if f[0] == "":
        f[0] = "*"
    if f[5] == "":
        f[5] = "*"
    if f[2] == "":
        f[2] = "*"
    if f[6] == "":
        f[6] = "*"
    if f[6] == "*":
        f[7] = "0"
    elif f[6] == f[2]:
        f[6] = "="
    elif f[6] == "=" and f[2] == "*":
        f[6] = "*"
    return "\t".join(f)


def decode_file(data):
    """(header text, contigs, [SAM line]) of a whole BAM file (with its EOF marker)"""
    assert data.endswith(EOF), "no EOF marker"
    raw = inflate(data)
    text, contigs, at = parse_header(raw)
    return text, contigs, [render(r, contigs) for r in records(raw, at)]
