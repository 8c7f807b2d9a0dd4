"""A plain restatement of the sorted-BAM contract of include/gwa.h in Python, over bam_ref's decoded records:
the sort key and the stable order, the virtual offsets of a stream cut into 65 280-byte slices, the .bai
(SAM specification section 5.2: bins by reg2bin, chunks, the pseudo-bin 37450, the 16 kb linear index) and a
region query through an index (reg2bins, the linear index's lower bound, chunks read with zlib).  Written from
the rule and the specification's tables, not from csrc/bam_sort_core.h.  Shared by test_bam_sort_host.py (CPU)
and test_gpu_bam_sort.py."""
import struct
import zlib

import bam_ref

SLICE = 65280
MAX_END = 1 << 29
PSEUDO_BIN = 37450
NO_REF_KEY = 0xFFFFFFFF00000000
HD_LINE = "@HD\tVN:1.6\tSO:coordinate\n"
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


def fields(rec):
    """(refID, pos, flag, reflen) of one record (block_size included)"""
    ref, pos, lname, _mapq, _bin, ncig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    reflen = 0
    for i in range(ncig):
        v = struct.unpack_from("<I", rec, 36 + lname + 4 * i)[0]
        if v & 15 in REF_OPS:
            reflen += v >> 4
    return ref, pos, flag, reflen


def key(rec):
    ref, pos, _, _ = fields(rec)
    if ref == -1:
        return NO_REF_KEY
    return (ref & 0xFFFFFFFF) << 32 | ((pos & 0xFFFFFFFF) ^ 0x80000000)


def interval(rec):
    """(beg, end) of an indexed record"""
    _, pos, _, reflen = fields(rec)
    beg = max(pos, 0)
    return beg, min(max(pos + max(reflen, 1), beg + 1), MAX_END)


def sort_records(records):
    """the records (a list of bytes) stably sorted by key"""
    return sorted(records, key=key)  # (Python's sort is stable)


def sorted_header(contigs, sam_header_text):
    return bam_ref.header(contigs, HD_LINE + sam_header_text)


def block_starts(block_sizes, h):
    out, at = [], h
    for s in block_sizes:
        out.append(at)
        at += s
    return out + [at]


def voffset(u, starts):
    return starts[u // SLICE] << 16 | u % SLICE


def build_bai(records, n_ref, block_sizes, h):
    """The .bai of the sorted records whose stream starts at file offset h and was compressed into blocks of
    block_sizes bytes (one per slice)."""
    starts = block_starts(block_sizes, h)
    refs = [dict(bins={}, order=[], first=None, last=None, mapped=0, unmapped=0, recs=[]) for _ in range(n_ref)]
    no_coor, u = 0, 0
    for rec in records:
        a, u = u, u + len(rec)
        ref, _pos, flag, _ = fields(rec)
        if ref == -1:
            no_coor += 1
            continue
        assert 0 <= ref < n_ref
        beg, end = interval(rec)
        refs[ref]["recs"].append((bam_ref.reg2bin(beg, end), beg, end, voffset(a, starts), voffset(u, starts), flag))
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for r in refs:
        if not r["recs"]:
            out += struct.pack("<ii", 0, 0)
            continue
        bins, prev = {}, None
        for b, beg, end, vb, ve, flag in r["recs"]:
            if b == prev:
                bins[b][-1][1] = ve
            else:
                bins.setdefault(b, []).append([vb, ve])
            prev = b
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b]))
            for vb, ve in bins[b]:
                out += struct.pack("<QQ", vb, ve)
        mapped = sum(1 for x in r["recs"] if not x[5] & 0x4)
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, r["recs"][0][3], r["recs"][-1][4], mapped, len(r["recs"]) - mapped)
        n_intv = ((max(x[2] for x in r["recs"]) - 1) >> 14) + 1
        lin = [None] * n_intv
        for _b, beg, end, vb, _ve, _f in r["recs"]:
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                if lin[w] is None or vb < lin[w]:
                    lin[w] = vb
        for w in range(n_intv - 2, -1, -1):
            if lin[w] is None:
                lin[w] = lin[w + 1]
        lin = [0 if v is None else v for v in lin]
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in lin)
    return out + struct.pack("<Q", no_coor)


def parse_bai(data):
    """([(bins {bin: [(beg, end)]}, linear [ioffset])] per contig, n_no_coor)"""
    assert data[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", data, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
        n_intv = struct.unpack_from("<i", data, at)[0]
        at += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, data, at))
        at += 8 * n_intv
        refs.append((bins, lin))
    no_coor = struct.unpack_from("<Q", data, at)[0]
    assert at + 8 == len(data)
    return refs, no_coor


def reg2bins(beg, end):
    """SAM specification 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class _Reader:
    """sequential reads at virtual offsets of a BGZF file"""

    def __init__(self, data):
        self.data, self.cache = data, {}

    def block(self, coff):
        if coff not in self.cache:
            d = self.data
            assert d[coff:coff + 4] == b"\x1f\x8b\x08\x04", coff
            bsize = struct.unpack_from("<H", d, coff + 16)[0] + 1
            self.cache[coff] = (bsize, zlib.decompress(d[coff + 18:coff + bsize - 8], -15))
        return self.cache[coff]

    def seek(self, voff):
        self.coff, self.uoff = voff >> 16, voff & 0xFFFF
        self._norm()

    def _norm(self):
        while self.coff < len(self.data):
            bsize, raw = self.block(self.coff)
            if self.uoff < len(raw):
                return
            self.coff, self.uoff = self.coff + bsize, self.uoff - len(raw)

    def tell(self):
        return self.coff << 16 | self.uoff

    def read(self, n):
        out = b""
        while n:
            _bsize, raw = self.block(self.coff)
            part = raw[self.uoff:self.uoff + n]
            assert part, "read past the file's end"
            out += part
            n -= len(part)
            self.uoff += len(part)
            self._norm()
        return out


def query(file_bytes, bai, ref, frm, to):
    """the records of contig ref overlapping [frm, to), found through the index, in file order"""
    refs, _ = parse_bai(bai)
    bins, lin = refs[ref]
    if not lin:
        min_off = 0
    else:
        min_off = lin[min(max(frm, 0) >> 14, len(lin) - 1)]
    chunks = sorted(c for b in reg2bins(max(frm, 0), to) if b in bins and b != PSEUDO_BIN for c in bins[b] if c[1] > min_off)
    rd, out, seen = _Reader(file_bytes), [], set()
    for vb, ve in chunks:
        rd.seek(vb)
        while rd.tell() < ve:
            at = rd.tell()
            size = struct.unpack("<I", rd.read(4))[0]
            rec = struct.pack("<I", size) + rd.read(size)
            if at in seen:
                continue
            seen.add(at)
            r, _pos, _flag, _ = fields(rec)
            beg, end = interval(rec)
            if r == ref and beg < to and end > frm:
                out.append((at, rec))
    return [rec for _, rec in sorted(out)]


def brute_force(records, ref, frm, to):
    out = []
    for rec in records:
        if fields(rec)[0] == ref:
            beg, end = interval(rec)
            if beg < to and end > frm:
                out.append(rec)
    return out


def check_file(data, header_bytes, stream):
    """the file's structure: BGZF(header) + BGZF(stream) + EOF, each text one block per 65 280-byte slice;
    returns (H, the compressed sizes of the stream's blocks)"""
    assert data.endswith(bam_ref.EOF)
    blocks = bam_ref.bgzf_blocks(data[:-len(bam_ref.EOF)])
    nh = -(-len(header_bytes) // SLICE)
    ns = -(-len(stream) // SLICE)
    assert len(blocks) == nh + ns, (len(blocks), nh, ns)
    assert b"".join(raw for _, raw in blocks[:nh]) == header_bytes
    assert b"".join(raw for _, raw in blocks[nh:]) == stream
    for part, text in ((blocks[:nh], header_bytes), (blocks[nh:], stream)):
        assert [len(raw) for _, raw in part] == [min(SLICE, len(text) - i) for i in range(0, len(text), SLICE)]
    return sum(s for s, _ in blocks[:nh]), [s for s, _ in blocks[nh:]]
