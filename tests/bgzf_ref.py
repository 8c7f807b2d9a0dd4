"""The BGZF contract of include/gwa.h restated with zlib (helper of tests/test_bgzf_host.py and
tests/test_gpu_bgzf.py; no test of its own).

blocks(data) walks the members of a BGZF byte string and checks each one: the 18 header bytes with
BSIZE + 1 the member's size, a payload that is one final deflate block inflating to exactly ISIZE bytes
with nothing left over, CRC32, and ISIZE = 65 280 for every block but the last of a run (a run ends
where a block is shorter: each batch of a pipeline run is its own run).  It returns the slices.
yardstick(text, strategy) is what zlib level 6 with that strategy makes of the same 65 280-byte cuts,
26 bytes of BGZF framing per block included.
"""
import struct
import zlib

SLICE = 65280
MAX_BLOCK = SLICE + 31
HEADER = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0])
EOF = HEADER + bytes([0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def members(data):
    """(header-checked) members of data as (payload, crc, isize)"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == HEADER, "bad BGZF header at %d" % at
        (bsize,) = struct.unpack_from("<H", data, at + 16)
        size = bsize + 1
        assert at + size <= len(data), "member at %d runs past the end" % at
        assert 26 <= size <= MAX_BLOCK
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        out.append((data[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def blocks(data, runs=False):
    """the slices of every block of data, each checked against the contract; runs=True allows several
    runs of blocks (a short block may be followed by more)"""
    slices = []
    ms = members(data)
    for k, (payload, crc, isize) in enumerate(ms):
        assert payload, "empty payload"
        assert payload[0] & 1, "BFINAL is not set on the first deflate block"
        assert (payload[0] >> 1) & 3 in (0, 2), "neither stored nor dynamic Huffman"
        d = zlib.decompressobj(-15)
        text = d.decompress(payload)
        assert d.eof and not d.unused_data and not d.unconsumed_tail, "payload is not exactly one deflate stream"
        assert len(text) == isize and 0 < isize <= SLICE
        assert zlib.crc32(text) == crc
        if not runs and k + 1 < len(ms):
            assert isize == SLICE, "a short block inside a run"
        slices.append(text)
    return slices


def stored_count(data):
    return sum(1 for payload, _, _ in members(data) if (payload[0] >> 1) & 3 == 0)


def yardstick(text, strategy):
    total = 0
    for at in range(0, len(text), SLICE):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(text[at:at + SLICE]) + c.flush()) + 26
    return total
