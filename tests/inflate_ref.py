"""Inputs of the BGZF decoder's tests (helper of tests/test_inflate_host.py and tests/test_gpu_inflate.py;
no test of its own): BGZF members built with zlib and framed by hand, and malformed members whose deflate
payloads are written bit by bit.

A member is at most 65 536 bytes (BSIZE is 16 bits), so a payload is at most 65 510: combinations of a text
and an encoder that give more (65 536 bytes stored need 65 546) cannot be framed and are left out; stored
blocks in sequence are covered by level 0 with flushes instead.
"""
import random
import struct
import zlib

import bgzf_ref

MAX_PAYLOAD = 65536 - 26
LENGTHS = (0, 1, 2, 3, 257, 258, 259, 65279, 65280, 65281, 65535, 65536)
# status codes of csrc/inflate_core.h
(OK, BLOCK_TYPE, STORED_LEN, TRUNCATED, COUNTS, CL_CODE, REPEAT, NO_EOB, CODE_SET, BAD_CODE, DISTANCE, LENGTH,
 CRC) = range(13)

ENCODERS = {
    "l0": (0, zlib.Z_DEFAULT_STRATEGY),
    "l1": (1, zlib.Z_DEFAULT_STRATEGY),
    "l6": (6, zlib.Z_DEFAULT_STRATEGY),
    "l9": (9, zlib.Z_DEFAULT_STRATEGY),
    "fixed": (6, zlib.Z_FIXED),
    "huff": (6, zlib.Z_HUFFMAN_ONLY),
    "rle": (6, zlib.Z_RLE),
}


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=(), flush=zlib.Z_FULL_FLUSH):
    """raw deflate of data; cuts: positions after which the stream is flushed (a new deflate block starts)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = b"", 0
    for cut in cuts:
        out += c.compress(data[at:cut]) + c.flush(flush)
        at = cut
    return out + c.compress(data[at:]) + c.flush()


def frame(payload, crc, isize, extra=b""):
    """a BGZF member around a deflate payload; extra: subfields put before BC"""
    xlen = len(extra) + 6
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536, "a member is at most 65536 bytes"
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", total - 1) +
            payload + struct.pack("<II", crc, isize))


def member(data, payload=None, **kw):
    return frame(deflate(data) if payload is None else payload, zlib.crc32(data), len(data), **kw)


def fits(payload):
    return len(payload) <= MAX_PAYLOAD


# ---- texts -----------------------------------------------------------------------------------------------

def low_entropy(n, seed=3):
    rng = random.Random(seed)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randint(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b" " if rng.random() < 0.8 else b"\n")
    return bytes(out[:n])


def fibonacci_bytes(seed=9, crowd=246):
    """the construction of tests/test_bgzf_host.py, restated: 246 byte values once each, the other ten with
    Fibonacci-like counts starting at their sum, so that the literal tree is 16 deep before the limit of 15
    and 15-bit codes appear"""
    rng = random.Random(seed)
    w = [crowd, 2 * crowd]
    while len(w) < 256 - crowd:
        w.append(w[-1] + w[-2])
    vals = list(range(256))
    rng.shuffle(vals)
    pool = list(vals[:crowd])
    for v, c in zip(vals[crowd:], w):
        pool += [v] * c
    rng.shuffle(pool)
    return bytes(pool)


def fastq_text(n_rec, seed=11):
    rng = random.Random(seed)
    out = []
    for i in range(n_rec):
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        q = "".join(rng.choices("IHGFEDCBA@?>=", [2 ** (12 - k) for k in range(13)], k=100))
        out.append("@read%d/1\n%s\n+\n%s\n" % (i, seq, q))
    return "".join(out).encode()


def sam_text(n, seed=5):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        out.append("read%d\t%d\tchr%d\t%d\t255\t100M\t*\t0\t0\t%s\t%s\tNM:i:%d\n"
                   % (i, rng.choice((0, 16)), rng.randint(1, 22), rng.randint(1, 10 ** 8), seq, "I" * 100, rng.randint(0, 3)))
    return "".join(out).encode()


_TEXTS = None


def texts():
    global _TEXTS
    if _TEXTS is None:
        _TEXTS = _texts()
    return _TEXTS


def _texts():
    rng = random.Random(23)
    d = {"one_byte": b"x" * 65536}
    for p in (1, 2, 3, 63, 64, 65, 257, 258, 259):
        pat = bytes(rng.randrange(97, 123) for _ in range(p))
        d["period%d" % p] = (pat * (5000 // p + 2))[:5000]
    pat = bytes(rng.randrange(97, 123) for _ in range(40))
    d["dist32768"] = bytes(rng.randrange(33, 91) for _ in range(50)) + pat + b"Z" * (32768 - 40) + pat + b"tail"
    d["fibonacci"] = fibonacci_bytes()
    d["random"] = bytes(rng.getrandbits(8) for _ in range(20000))
    d["sam"] = sam_text(200)
    d["fastq"] = fastq_text(250)
    return d


_WELL = None


def well_formed():
    """[(name, text, BGZF bytes)]: single members, then inputs of several members"""
    global _WELL
    if _WELL is not None:
        return _WELL
    out = []
    le = low_entropy(65536)
    for n in LENGTHS:
        for enc, (level, strategy) in ENCODERS.items():
            p = deflate(le[:n], level, strategy)
            if fits(p):
                out.append(("len%d_%s" % (n, enc), le[:n], member(le[:n], p)))
    for name, t in texts().items():
        for enc in ("l1", "l6", "l9", "fixed", "huff", "rle") if name != "random" else ("l0", "l6"):
            level, strategy = ENCODERS[enc]
            p = deflate(t, level, strategy)
            if fits(p):
                out.append(("%s_%s" % (name, enc), t, member(t, p)))
    # several deflate blocks in one member: an empty stored block in mid-stream (sync and full flush), a
    # non-final first block, stored blocks in sequence
    t = low_entropy(30000, seed=8)
    for enc in ("l0", "l6", "fixed"):
        level, strategy = ENCODERS[enc]
        for fl, fname in ((zlib.Z_FULL_FLUSH, "full"), (zlib.Z_SYNC_FLUSH, "sync")):
            out.append(("blocks_%s_%s" % (enc, fname), t, member(t, deflate(t, level, strategy, (1, 10000, 10000, 29999), fl))))
    # several members in one input: EOF markers in the middle and at the end, a subfield before BC
    parts = [le[:1000], b"", texts()["fastq"][:40000], le[:65536], b"", b"z"]
    multi = b"".join(bgzf_ref.EOF if not x else member(x, extra=b"XY\x03\0abc" if k == 2 else b"") for k, x in enumerate(parts))
    out.append(("multi", b"".join(parts), multi))
    out.append(("eof_only", b"", bgzf_ref.EOF))
    out.append(("nothing", b"", b""))
    _WELL = out
    return out


# ---- hand-built bit streams -------------------------------------------------------------------------------

class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):  # least significant bit first, as deflate packs header fields and extra bits
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.v |= value << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):  # a Huffman code: most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self, pad=0):
        return self.v.to_bytes((self.n + 7) // 8, "little") + b"\0" * pad


def canonical(lens):
    """symbol -> (code, length) of the canonical Huffman code with these lengths (lengths of 0: no code)"""
    code, out = 0, {}
    for length in range(1, 16):
        for s in sorted(lens):
            if lens[s] == length:
                out[s] = (code, length)
                code += 1
        code <<= 1
    return out


def fixed_lit(b, s):
    if s < 144:
        return b.code(0x30 + s, 8)
    if s < 256:
        return b.code(0x190 + s - 144, 9)
    if s < 280:
        return b.code(s - 256, 7)
    return b.code(0xc0 + s - 280, 8)


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_header(hlit, hdist, cl_lens, seq):
    """BFINAL 1, BTYPE 2, the counts as given (HLIT and HDIST as the header's field values), the
    code-length code, then seq: (symbol, extra value) pairs in that code"""
    b = Bits().put(1, 1).put(2, 2).put(hlit, 5).put(hdist, 5)
    hclen = max(CL_ORDER.index(s) for s in cl_lens) + 1 if cl_lens else 4
    hclen = max(hclen, 4)
    b.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        b.put(cl_lens.get(s, 0), 3)
    codes = canonical(cl_lens)
    extra = {16: 2, 17: 3, 18: 7}
    for s, x in seq:
        b.code(*codes[s])
        if s in extra:
            b.put(x, extra[s])
    return b


def lens_seq(lens, n):
    """lengths 0 / 1 / 2 of symbols 0..n-1, one code-length symbol each"""
    return [(lens.get(i, 0), 0) for i in range(n)]


def malformed():
    """[(name, BGZF bytes, the decoder's status code)] for one member each; the walk accepts them all"""
    out = []

    def add(name, payload, code, text=b"", crc=None, isize=None, pad=8):
        payload = payload.bytes(pad) if isinstance(payload, Bits) else payload
        out.append((name, frame(payload, zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize), code))

    add("btype3", Bits().put(1, 1).put(3, 2), BLOCK_TYPE)
    add("stored_len_nlen", Bits().put(1, 1).put(0, 2).align().put(5, 16).put(5, 16), STORED_LEN, text=b"\0" * 5)
    add("stored_len_past_payload", Bits().put(1, 1).put(0, 2).align().put(100, 16).put(100 ^ 0xffff, 16), TRUNCATED, text=b"\0" * 100)
    for v in (30, 31):
        add("hlit%d" % v, Bits().put(1, 1).put(2, 2).put(v, 5).put(0, 5).put(0, 4), COUNTS)
        add("hdist%d" % v, Bits().put(1, 1).put(2, 2).put(0, 5).put(v, 5).put(0, 4), COUNTS)
    add("cl_code_incomplete", dynamic_header(0, 0, {0: 2, 1: 2}, []), CL_CODE)
    add("cl_code_oversubscribed", dynamic_header(0, 0, {0: 1, 1: 1, 2: 1}, []), CL_CODE)
    add("repeat16_first", dynamic_header(0, 0, {16: 1, 0: 1}, [(16, 0)]), REPEAT)
    add("repeat_past_end", dynamic_header(0, 0, {18: 1, 0: 1}, [(18, 127), (18, 127)]), REPEAT)
    add("lit_oversubscribed", dynamic_header(0, 0, {0: 1, 1: 1}, lens_seq({0: 1, 1: 1, 256: 1}, 258)), CODE_SET)
    add("lit_incomplete", dynamic_header(0, 0, {0: 1, 2: 1}, lens_seq({0: 2, 256: 2}, 258)), CODE_SET)
    add("dist_incomplete", dynamic_header(0, 1, {0: 1, 1: 2, 2: 2}, lens_seq({0: 1, 256: 1, 257: 2, 258: 2}, 259)), CODE_SET)
    add("no_end_of_block", dynamic_header(0, 0, {0: 1, 1: 1}, lens_seq({0: 1, 1: 1}, 258)), NO_EOB)
    for s in (286, 287):
        b = fixed_lit(Bits().put(1, 1).put(1, 2), 97)
        add("fixed_lit%d" % s, fixed_lit(b, s).code(0, 5), BAD_CODE, text=b"aaaa")
    for s in (30, 31):
        b = fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257)
        add("fixed_dist%d" % s, fixed_lit(b.code(s, 5), 256), BAD_CODE, text=b"aaaa")
    b = fixed_lit(fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 97), 98), 257)
    add("distance_past_start", fixed_lit(b.code(2, 5), 256), DISTANCE, text=b"ababa")
    # (zeros follow the payload: seven of them are the fixed code of end-of-block, two past the end)
    add("payload_ends_in_a_code", fixed_lit(Bits().put(1, 1).put(1, 2), 97), TRUNCATED, text=b"a", pad=0)
    t = low_entropy(300, seed=6)
    add("one_byte_longer", deflate(t), LENGTH, text=t[:-1])
    add("one_byte_shorter", deflate(t), LENGTH, text=t + b"x")
    add("wrong_crc", deflate(t), CRC, text=t, crc=zlib.crc32(t) ^ 1)
    return out


def one_per_code():
    """twelve malformed members, one per status code"""
    seen, out = set(), []
    for name, data, code in malformed():
        if code not in seen:
            seen.add(code)
            out.append((name, data, code))
    assert sorted(seen) == list(range(1, 13))
    return out


def header_faults():
    """[(name, bytes, a part of the message)]: inputs the member walk refuses"""
    good = member(b"hello")
    eof = bgzf_ref.EOF
    no_bc = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"XY\x02\0\0\0" + b"\x03\0" + bytes(8)
    plain_gzip = b"\x1f\x8b\x08\0\0\0\0\0\0\xff\x03\0" + bytes(8)
    small = bytearray(eof)
    small[16:18] = struct.pack("<H", 24)  # BSIZE + 1 = 25 < 18 + 8
    past = bytearray(good)
    past[16:18] = struct.pack("<H", len(good) + 3)
    big = frame(deflate(b""), 0, 65537)
    return [
        ("bad_magic", good + b"\x1f\x8c" + good[2:], "member 1 at byte %d: no gzip magic" % len(good)),
        ("no_bc_subfield", eof + no_bc, "member 1 at byte 28: no BC subfield"),
        ("no_extra_field", plain_gzip, "member 0 at byte 0: no extra field"),
        ("bsize_below_minimum", bytes(small), "member 0 at byte 0: BSIZE + 1 = 25"),
        ("bsize_past_input", good + bytes(past), "member 1 at byte %d: the member runs past" % len(good)),
        ("isize_65537", good + good + big, "member 2 at byte %d: ISIZE 65537" % (2 * len(good))),
    ]


# ---- read files ---------------------------------------------------------------------------------------------

def cut_members(text, seed=1, lo=300, hi=4000, eof=True, level=6):
    """text as a BGZF file whose members hold lo..hi text bytes each (records straddle them)"""
    rng = random.Random(seed)
    out, at = [], 0
    while at < len(text):
        n = rng.randint(lo, hi)
        out.append(member(text[at:at + n], deflate(text[at:at + n], level)))
        at += n
    return b"".join(out) + (bgzf_ref.EOF if eof else b"")
