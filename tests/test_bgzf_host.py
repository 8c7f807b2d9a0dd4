"""The BGZF encoder (csrc/bgzf_core.h) on the CPU: tests/bgzf_host.cpp, a program of its own built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, replays the device kernel's lanes
phase by phase.  Every output is checked against the contract of include/gwa.h as tests/bgzf_ref.py
restates it with zlib, and must inflate to the input.  The inputs are the smallest at which the encoder
can go wrong; tests/test_gpu_bgzf.py compares the device kernel with this build on the same inputs
(INPUTS).  The two size conditions are derived from zlib in the test, not measured on the encoder.  No GPU."""
import math
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

import bgzf_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

SLICE = bgzf_ref.SLICE
LANES, SEG = 1024, 64  # bgzf_core.h kLanes (strip length), kSeg (positions per lane in CRC and emission)
A1 = bytes(range(97, 123))           # pattern alphabet
A2 = bytes(range(33, 91))            # filler alphabet, disjoint from A1


def low_entropy(n, seed=3):
    rng = random.Random(seed)
    words = [bytes(rng.choice(A1) for _ in range(rng.randint(2, 9))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b" " if rng.random() < 0.8 else b"\n")
    return bytes(out[:n])


def filler(n, rng):
    return bytes(rng.choice(A2) for _ in range(n))


def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence B(k, n) (Lyndon words): every n-gram once"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def fibonacci_bytes(seed=9, crowd=246):
    """all 256 byte values: 246 once each, the other ten with Fibonacci-like counts starting at their sum
    (246, 492, 738, 1230, ...), so that the literal tree is a chain on top of the crowd's subtree: 16 deep
    before the limit of 15, with the matches the encoder finds in it"""
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


def dyadic_bytes(seed=10):
    """255 byte values with counts 16 * 2^(11 - L), where the number of values per L is Fibonacci-like
    (1, 1, 2, 3, 5, 8, 13, 21 for L = 2..9): the code lengths' own histogram is then skewed, and the
    code-length code's tree is 8 deep before its limit of 7"""
    rng = random.Random(seed)
    counts = {2: 1, 3: 1, 4: 2, 5: 3, 6: 5, 7: 8, 8: 13, 9: 21, 10: 151, 11: 50}
    vals = list(range(256))
    rng.shuffle(vals)
    pool, i = [], 0
    for length, c in counts.items():
        for _ in range(c):
            pool += [vals[i]] * (16 * 2 ** (11 - length))
            i += 1
    rng.shuffle(pool)
    return bytes(pool)


def sam_lines(n, const_q, seed=5):
    """n synthetic 100 bp SAM lines; qualities constant I or from a skewed 13-symbol alphabet"""
    rng = random.Random(seed)
    qa, w = "IHGFEDCBA@?>=", [2 ** (12 - i) for i in range(13)]
    out = []
    for i in range(n):
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        q = "I" * 100 if const_q else "".join(rng.choices(qa, w, k=100))
        out.append("read%d\t%d\tchr%d\t%d\t255\t100M\t*\t0\t0\t%s\t%s\tNM:i:%d\tX0:i:1\n"
                   % (i, rng.choice((0, 16)), rng.randint(1, 22), rng.randint(1, 10 ** 8), seq, q, rng.randint(0, 3)))
    return "".join(out).encode()


def repeat_at(pattern_len, dist, rng, between=None):
    """filler, a seeded pattern, filler, the pattern again `dist` bytes after its first start, filler;
    between: one byte value to fill the gap with (the encoder keeps one candidate per hash value, the
    latest: varied filler over tens of kilobytes would displace the pattern's)"""
    p = bytes(rng.choice(A1) for _ in range(pattern_len))
    assert dist >= pattern_len
    gap = filler(dist - pattern_len, rng) if between is None else between * (dist - pattern_len)
    return filler(50, rng) + p + gap + p + filler(50, rng)


def periodic(period, n, rng):
    p = bytes(rng.choice(A1) for _ in range(period))
    return (p * (n // period + 1))[:n]


def INPUTS():
    """name -> bytes: the inputs of the host test, shared with the device test"""
    rng = random.Random(17)
    le = low_entropy(2 * SLICE + 1)
    d = {"len%d" % n: le[:n] for n in (1, 2, 3, 4, 5, SEG - 1, SEG, SEG + 1, LANES - 1, LANES, LANES + 1,
                                        2 * LANES - 1, 2 * LANES + 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1)}
    d["one_byte"] = b"x" * SLICE
    d["no_repeat"] = bytes(48 + s for s in de_bruijn(40, 3))  # 64 000 bytes, every 3-gram once
    d["fibonacci"] = fibonacci_bytes()
    d["dyadic"] = dyadic_bytes()
    d["random_slice"] = bytes(rng.getrandbits(8) for _ in range(SLICE))
    d["random_70000"] = bytes(rng.getrandbits(8) for _ in range(70000))
    for n in (3, 4, 10, 11, 18, 19, 257, 258):
        d["repeat%d" % n] = repeat_at(n, 1500 + n, rng)
    d["run1000"] = filler(30, rng) + b"q" * 1000 + filler(30, rng)
    for dist in (1, 4, 5):
        d["dist%d" % dist] = filler(20, rng) + periodic(dist, 3000, rng) + filler(20, rng)
    for dist in (24577, 32768, 32769):
        d["dist%d" % dist] = repeat_at(40, dist, rng, between=b"Z")
    # a repeat lying across the cut: the second slice may not reach back into the first
    p = bytes(rng.choice(A1) for _ in range(200))
    d["across_cut"] = filler(60000, rng) + p + filler(SLICE - 60000 - 200 - 100, rng) + p + filler(3000, rng) + p + filler(100, rng)
    # more matches than the compact list holds: 6-byte words of a 100-word dictionary
    words = [bytes(rng.choice(A1) for _ in range(6)) for _ in range(100)]
    d["many_matches"] = b"".join(rng.choice(words) for _ in range(SLICE // 6))
    return d


@pytest.fixture(scope="module")
def bgzf_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_host")
    exe = d / "bgzf_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-I", CSRC] + SAN + ["-o", str(exe), os.path.join(HERE, "bgzf_host.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    count = [0]

    def run(data, prefixes=None):
        count[0] += 1
        src, dst = d / ("in%d" % count[0]), d / ("out%d" % count[0])
        src.write_bytes(data)
        env = dict(os.environ)
        env.update({"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
        args = [str(exe)] + (["-p", str(prefixes)] if prefixes is not None else []) + [str(src), str(dst)]
        r = subprocess.run(args, capture_output=True, env=env, timeout=600)
        err = r.stderr.decode(errors="replace")
        for tag in ("Sanitizer", "runtime error"):
            assert tag not in err, err[-6000:]
        assert r.returncode == 0, (r.returncode, err[-4000:])
        nblocks, stored = (int(x) for x in r.stdout.split())
        return dst.read_bytes(), nblocks, stored

    return run


@pytest.fixture(scope="module")
def inputs():
    return INPUTS()


def check(data, out):
    slices = bgzf_ref.blocks(out)
    assert b"".join(slices) == data
    assert len(slices) == math.ceil(len(data) / SLICE)
    return slices


def test_empty_input_gives_no_block(bgzf_host):
    assert bgzf_host(b"") == (b"", 0, 0)


def test_every_input_round_trips(bgzf_host, inputs):
    for name, data in inputs.items():
        out, nblocks, stored = bgzf_host(data)
        try:
            check(data, out)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        assert nblocks == math.ceil(len(data) / SLICE), name
        assert stored == bgzf_ref.stored_count(out), name


def test_lengths_1_to_3000(bgzf_host):
    data = low_entropy(3000, seed=4)
    out, _, _ = bgzf_host(data, prefixes=3000)
    at = 0
    for n in range(3001):
        (size,) = struct.unpack_from("<I", out, at)
        blk = out[at + 4:at + 4 + size]
        at += 4 + size
        if n == 0:
            assert size == 0
        else:
            assert bgzf_ref.blocks(blk) == [data[:n]], n
    assert at == len(out)


def deflate_header(out):
    """(BTYPE, HLIT, HDIST) of the first block's payload"""
    bits = int.from_bytes(out[18:22], "little")
    return (bits >> 1) & 3, ((bits >> 3) & 31) + 257, ((bits >> 8) & 31) + 1


def test_one_repeated_byte(bgzf_host, inputs):
    out, _, stored = bgzf_host(inputs["one_byte"])
    btype, hlit, hdist = deflate_header(out)
    # one literal, then matches of distance 1: literals x and end-of-block, length codes, one distance code
    assert (btype, hdist, stored) == (2, 1, 0) and len(out) < 200


def test_no_match_has_no_distance_code(bgzf_host, inputs):
    data = inputs["no_repeat"]
    assert len({data[i:i + 3] for i in range(len(data) - 2)}) == len(data) - 2
    out, _, stored = bgzf_host(data)
    btype, hlit, hdist = deflate_header(out)
    assert (btype, hlit, hdist, stored) == (2, 257, 1, 0)
    assert len(out) < 0.72 * len(data)  # 40 symbols: 5.3 bits each


def test_incompressible_input_is_stored(bgzf_host, inputs):
    for name, nb in (("random_slice", 1), ("random_70000", 2)):
        out, nblocks, stored = bgzf_host(inputs[name])
        assert (nblocks, stored) == (nb, nb)
        sizes = [len(p) + 26 for p, _, _ in bgzf_ref.members(out)]
        assert max(sizes) <= SLICE + 31 and sizes[0] == SLICE + 31


def test_matches_are_used(bgzf_host, inputs):
    """a found match shortens the block: 258 repeated bytes cost a few bytes, not 258 literals"""
    for n in (19, 257, 258):
        data = inputs["repeat%d" % n]
        out, _, _ = bgzf_host(data)
        rng = random.Random(1)
        other = bytes(rng.choice(A1) for _ in range(n))
        cut = len(data) - 50 - n
        lone, _, _ = bgzf_host(data[:cut] + other + data[cut + n:])
        assert len(out) < len(lone) - n // 4, n
    out, _, _ = bgzf_host(inputs["dist32768"])
    far, _, _ = bgzf_host(inputs["dist32769"])
    assert len(out) < len(far) - 10  # distance 32 768 is a match, 32 769 is not
    out, _, _ = bgzf_host(inputs["run1000"])
    assert len(out) < 26 + 60 + 60


@pytest.fixture(scope="module")
def sam_texts():
    return {False: sam_lines(20000, False), True: sam_lines(20000, True)}


def test_size_on_sam_text_with_skewed_qualities(bgzf_host, sam_texts):
    text = sam_texts[False]
    out, _, stored = bgzf_host(text)
    check(text, out)
    y = bgzf_ref.yardstick(text, zlib.Z_HUFFMAN_ONLY)
    print("skewed qualities: %d -> %d bytes, %.3f of the Z_HUFFMAN_ONLY yardstick %d" % (len(text), len(out), len(out) / y, y))
    assert stored == 0 and len(out) <= 1.10 * y


def test_size_on_sam_text_with_constant_qualities(bgzf_host, sam_texts):
    text = sam_texts[True]
    out, _, stored = bgzf_host(text)
    check(text, out)
    y = bgzf_ref.yardstick(text, zlib.Z_HUFFMAN_ONLY)
    print("constant qualities: %d -> %d bytes, %.3f of the Z_HUFFMAN_ONLY yardstick %d" % (len(text), len(out), len(out) / y, y))
    assert stored == 0 and len(out) <= 0.85 * y


def test_two_runs_give_equal_bytes(bgzf_host, inputs, sam_texts):
    for data in (inputs["across_cut"], inputs["many_matches"], sam_texts[False][:3 * SLICE + 77]):
        assert bgzf_host(data)[0] == bgzf_host(data)[0]
