"""The coordinate sort, the run sorter and the .bai writer on the CPU: tests/bam_sort_host.cpp, a program of its
own built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, runs the host build of the
batch sort (csrc/bam_sort_core.h), the sorter (csrc/bam_sorter.cpp) and the index over records that
bam_ref.encode_line makes from hand-written lines on three contigs, one of them without any record.  The sorted
stream, the file and the .bai must equal tests/bai_ref.py's byte for byte (include/gwa.h "Sorted BAM").  No GPU."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import bai_ref
import bam_ref
import test_bam_host as BH
import test_md_host as MH

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = MH.CSRC
CXX = MH.CXX
SLICE = bai_ref.SLICE

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

CONTIGS = [("c1", 1 << 29), ("c2", 300000), ("c3", 1000)]  # c3 never has a record


def cigar_for(reflen):
    """M elements spanning reflen bases (an element's length has 28 bits)"""
    out = ""
    while reflen > 0:
        n = min(reflen, 200000000)
        out += "%dM" % n
        reflen -= n
    return out


def line(name, flag, rname, pos1, cigar, lseq):
    return "%s\t%d\t%s\t%d\t1\t%s\t*\t0\t0\t%s\t%s" % (name, flag, rname, pos1, cigar, "A" * lseq, "I" * lseq)


def rec(name, flag, rname, pos, cigar, lseq, contigs=CONTIGS):
    """pos: the record's 0-based pos"""
    return bam_ref.encode_line(line(name, flag, rname, pos + 1, cigar, lseq), contigs)


def sized(size, pos, rname="c2"):
    """a mapped record of exactly `size` bytes at pos"""
    for nl in range(1, 12):
        for l in range(1, size):
            if 36 + nl + 1 + 4 + (l + 1) // 2 + l == size:
                r = rec("n" * nl, 0, rname, pos, "%dM" % l, l)
                assert len(r) == size
                return r
    raise AssertionError(size)


def big_case():
    """[(run id, [record])]: every special position of the issue in one stream of several blocks"""
    rng = random.Random(11)
    recs = []
    for flag, beg, reflen in BH._bin_cases():  # bins at every level's edge, pos -1 and -5, FLAG 0x4
        recs.append(rec("b%d" % len(recs), flag, "c1", beg, cigar_for(reflen), 20))
    recs += [rec("p0", 0, "c2", 0, "30M", 30), rec("pm1", 0, "c2", -1, "30M", 30), rec("pm6", 16, "c2", -6, "30M", 30),
             rec("pm6b", 0, "c2", -6, "", 10)]
    recs += [rec("u4", 4, "c2", 100, "50M", 50), rec("u4b", 0x4 | 0x1 | 0x8, "c1", 7000, "", 33)]  # FLAG 0x4 with coordinates
    for pos in (0, -1, 5, 123456, -7, 2147483647):  # refID -1 with assorted pos: all last, in input order
        recs.append(rec("s%d" % len(recs), 4, "*", pos, "", 40))
    recs += [rec("w", 0, "c2", 16380, "100M", 100), rec("w2", 0, "c2", 16383, "1M", 1), rec("w3", 0, "c2", 16384, "1M", 1)]
    recs += [rec("gap", 0, "c2", 200000, "50M", 50)]  # empty windows between 32768 + and 196608
    recs += [rec("clip", 0, "c1", (1 << 29) - 10, "100M", 100), rec("clip2", 0, "c1", (1 << 29) - 1, "5M2D5M", 10)]
    recs += [rec("cig", 0, "c2", 900, "5S10M2I3D4N6=7X2H", 34)]
    for i in range(5):  # a tie group
        recs.append(rec("tie%d" % i, 16 * (i % 2), "c2", 500, "%dM" % (20 + i), 20 + i))
    for i in range(900):
        l = rng.randrange(30, 260)
        c = rng.choice(("c1", "c2", "c2"))
        pos = rng.randrange(0, 40000) if c == "c2" else rng.choice((rng.randrange(0, 1 << 20), rng.randrange(0, (1 << 29) - 300)))
        recs.append(rec("f%d" % i, rng.choice((0, 16)), c, pos, "%dM" % l, l))
    rng.shuffle(recs)
    runs, at, rid = [], 0, 0
    while at < len(recs):
        n = rng.choice((1, 50, 200, 400))
        runs.append((rid, recs[at:at + n]))
        at += n
        rid += 1 + rng.randrange(3)  # (ids need not be dense)
    return runs


def edge_case(total_extra):
    """records on c2 in ascending pos whose stream is 65 280 bytes (+ total_extra), the first 652 of 100 bytes
    and one of 80 ending exactly on the slice edge"""
    recs = [sized(100, 10 * i) for i in range(652)] + [sized(80 + total_extra, 7000)]
    return recs


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sort_host")
    exe = d / "bam_sort_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-pthread", "-DGWA_BAM_SORT_HOST_ONLY", "-I", CSRC] + MH.SAN + [
        "-o", str(exe), os.path.join(HERE, "bam_sort_host.cpp"), os.path.join(CSRC, "bam_sorter.cpp"), os.path.join(CSRC, "sam.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    count = [0]

    def run(runs, order=None, contigs=CONTIGS, mem=1 << 30, tmp=False, part=256, index=True, raw=None):
        """runs: [(id, [record])] (raw: {id: bytes} replaces a run's file).  Returns dict(rc, out, bam, bai,
        sorted {id: bytes}, keys {id: [int]}, tmp_left)"""
        count[0] += 1
        w = d / ("w%d" % count[0])
        w.mkdir()
        (w / "contigs").write_text("".join("%s %d\n" % c for c in contigs))
        tdir = w / "tmp"
        tdir.mkdir()
        args = []
        for rid, recs in (runs if order is None else [runs[i] for i in order]):
            f = w / ("run%d" % rid)
            f.write_bytes(raw[rid] if raw and rid in raw else b"".join(recs))
            args.append("%d:%s" % (rid, f))
        env = dict(os.environ)
        env.update({"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
        r = subprocess.run([str(exe), str(w / "contigs"), str(mem), str(tdir) if tmp else "-", str(part), str(w / "o.bam"),
                            str(w / "o.bai") if index else "-"] + args, capture_output=True, env=env, timeout=300)
        err = r.stderr.decode(errors="replace")
        for tag in ("Sanitizer", "runtime error"):
            assert tag not in err, err[-6000:]
        assert r.returncode in (0, 3), (r.returncode, err[-4000:])
        res = dict(rc=r.returncode, out=r.stdout.decode(), tmp_left=sorted(os.listdir(tdir)), sorted={}, keys={})
        if r.returncode == 0:
            res["bam"] = (w / "o.bam").read_bytes()
            res["bai"] = (w / "o.bai").read_bytes() if index else None
            for rid, _ in runs:
                res["sorted"][rid] = (w / ("run%d.sorted" % rid)).read_bytes()
                k = (w / ("run%d.keys" % rid)).read_bytes()
                res["keys"][rid] = list(struct.unpack("<%dQ" % (len(k) // 8), k))
        return res

    return run


def expect(runs, contigs=CONTIGS):
    """(sorted stream, its records) by bai_ref: the input-order stream is run-id order, then file order"""
    allrecs = [r for _, recs in sorted(runs, key=lambda x: x[0]) for r in recs]
    srt = bai_ref.sort_records(allrecs)
    return b"".join(srt), srt


def check(res, runs, contigs=CONTIGS):
    """file, stream and index against bai_ref; returns (stream, sorted records, block sizes)"""
    assert res["rc"] == 0, res["out"]
    stream, srt = expect(runs, contigs)
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    hdr = bai_ref.sorted_header(contigs, text)
    h, sizes = bai_ref.check_file(res["bam"], hdr, stream)
    if res["bai"] is not None:
        want = bai_ref.build_bai(srt, len(contigs), sizes, h)
        assert res["bai"].hex() == want.hex()
    for rid, recs in runs:  # the batch sort of every run
        s = bai_ref.sort_records(recs)
        assert res["sorted"][rid] == b"".join(s)
        assert res["keys"][rid] == [bai_ref.key(r) for r in s]
    ht, hc, lines = bam_ref.decode_file(res["bam"])
    assert ht == bai_ref.HD_LINE + text and hc == contigs and len(lines) == len(srt)
    return stream, srt, sizes


@pytest.fixture(scope="module")
def big(host):
    runs = big_case()
    return runs, host(runs)


def test_big_case_equals_the_restatement_and_covers_its_claims(big):
    runs, res = big
    stream, srt, sizes = check(res, runs)
    assert len(sizes) >= 3
    keys = [bai_ref.key(r) for r in srt]
    assert keys == sorted(keys)
    assert max(keys.count(k) for k in set(keys)) >= 3
    # equal keys keep input order: the tie group by name order within (run id, file order)
    order = [r for _, recs in sorted(runs, key=lambda x: x[0]) for r in recs]
    ties = [r for r in srt if b"tie" in r[36:42]]
    assert len(ties) == 5 and ties == [r for r in order if b"tie" in r[36:42]]
    # a record straddling a slice edge; refID -1 last; pos -6 before pos -1 before pos 0
    at, straddle = 0, 0
    for r in srt:
        straddle += at // SLICE != (at + len(r) - 1) // SLICE
        at += len(r)
    assert straddle >= 1
    n_star = sum(1 for r in srt if bai_ref.fields(r)[0] == -1)
    assert n_star == 6 and all(bai_ref.fields(r)[0] == -1 for r in srt[-6:])
    c2 = [bai_ref.fields(r)[1] for r in srt if bai_ref.fields(r)[0] == 1]
    assert c2[:5] == [-6, -6, -1, 0, c2[4]] and c2[4] >= 0
    refs, no_coor = bai_ref.parse_bai(res["bai"])
    assert no_coor == 6 and refs[2] == ({}, []) and bai_ref.PSEUDO_BIN in refs[0][0] and bai_ref.PSEUDO_BIN in refs[1][0]
    assert len(refs[0][1]) == ((1 << 29) - 1 >> 14) + 1  # `end` clipped at 2^29
    assert {0, 1, 9, 73, 585, 4681} <= set(refs[0][0])  # bins of every level
    lin = refs[1][1]
    assert len(lin) == (200049 >> 14) + 1 and lin[3] == lin[12] and lin[2] != lin[3]  # the gap takes the next window's
    mapped, unmapped = refs[1][0][bai_ref.PSEUDO_BIN][1]
    assert unmapped == 1 and mapped == sum(1 for r in srt if bai_ref.fields(r)[0] == 1) - 1
    # every query through the index returns the brute-force set
    rng = random.Random(5)
    for ref, frm, to in [(0, 0, 1 << 29), (1, 0, 1), (1, 16383, 16385), (1, 50000, 190000), (2, 0, 1000), (0, (1 << 29) - 5, 1 << 29)] + \
            [(1, a, a + rng.randrange(1, 3000)) for a in (rng.randrange(0, 41000) for _ in range(20))]:
        got = bai_ref.query(res["bam"], res["bai"], ref, frm, to)
        assert got == bai_ref.brute_force(srt, ref, frm, to), (ref, frm, to)


def test_run_order_memory_limit_spilling_and_part_size_change_nothing(host, big):
    runs, res = big
    n = len(runs)
    rng = random.Random(3)
    shuffled = list(range(n))
    rng.shuffle(shuffled)
    for kw in (dict(order=list(range(n))[::-1]), dict(order=shuffled), dict(mem=0, tmp=True), dict(part=1),
               dict(mem=30000, tmp=True, part=1, order=shuffled)):
        other = host(runs, **kw)
        assert other["rc"] == 0, other["out"]
        assert other["bam"] == res["bam"] and other["bai"] == res["bai"], kw
        assert other["tmp_left"] == [], kw
        stats = other["out"].split()
        if kw.get("mem") == 0:
            assert int(stats[4]) == int(stats[3]) == n  # every run spilled
        elif "mem" in kw:
            assert 0 < int(stats[4]) < n
        else:
            assert int(stats[4]) == 0
    # one batch holding everything: the same stream (the batch size does not matter)
    one = [(0, [r for _, recs in sorted(runs, key=lambda x: x[0]) for r in recs])]
    assert host(one)["bam"] == res["bam"]


def test_memory_limit_without_a_tmp_dir_fails(host, big):
    runs, _ = big
    res = host(runs, mem=1000)
    assert res["rc"] == 3 and "mem_bytes 1000" in res["out"] and "no tmp_dir" in res["out"]
    first = [recs for _, recs in runs if sum(map(len, recs)) > 1000][0]
    assert "of %d bytes" % sum(map(len, first)) in res["out"]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_zero_one_and_two_records(host, n):
    recs = [rec("a", 0, "c2", 70, "10M", 10), rec("b", 0, "c1", 70, "10M", 10)][:n]
    runs = [(0, recs)] if n else []
    res = host(runs)
    stream, srt, sizes = check(res, runs)
    assert len(sizes) == (1 if n else 0)
    if n == 0:
        assert res["bai"] == b"BAI\1" + struct.pack("<i", 3) + b"\0" * 24 + b"\0" * 8
    if n == 2:
        assert srt == recs[::-1]
    # an empty run next to the others changes nothing
    assert host(runs + [(9, [])])["bam"] == res["bam"]


def test_all_keys_equal_keep_input_order(host):
    runs = [(i, [rec("k%d_%d" % (i, j), 16 * (j % 2), "c2", 40, "%dM" % (5 + j), 5 + j) for j in range(4)]) for i in range(3)]
    res = host(runs, order=[2, 0, 1])
    _, srt, _ = check(res, runs)
    assert srt == [r for _, recs in runs for r in recs]


@pytest.mark.parametrize("extra", [0, 1])
def test_a_stream_of_exactly_one_slice_and_one_byte_more(host, extra):
    recs = edge_case(extra)
    assert sum(map(len, recs)) == SLICE + extra
    runs = [(0, recs[300:]), (1, recs[:300])]
    res = host(runs)
    stream, srt, sizes = check(res, runs)
    assert len(sizes) == 1 + extra and len(stream) == SLICE + extra


def test_a_record_ending_on_a_slice_edge_and_one_straddling_it(host):
    recs = edge_case(0) + [sized(130, 20000 + i) for i in range(600)]  # (the next 16 kb window: another bin)
    runs = [(0, recs[::2]), (1, recs[1::2])]
    res = host(runs, part=1)
    stream, srt, sizes = check(res, runs)
    ends, at = [], 0
    for r in srt:
        at += len(r)
        ends.append(at)
    assert SLICE in ends and 2 * SLICE not in ends and len(sizes) == 3
    # the end offset of the record on the edge is the next block, offset 0
    h = len(res["bam"]) - 28 - sum(sizes)
    refs, _ = bai_ref.parse_bai(res["bai"])
    assert refs[1][0][4681] == [(h << 16, (h + sizes[0]) << 16)] and refs[1][0][4682][0][0] == (h + sizes[0]) << 16
    assert host(runs)["bam"] == res["bam"]


def test_a_contig_longer_than_the_index_covers(host):
    contigs = [("long", (1 << 29) + 1), ("c2", 5000)]
    runs = [(0, [rec("a", 0, "c2", 70, "10M", 10, contigs), rec("b", 0, "long", 1 << 29, "10M", 10, contigs)])]
    res = host(runs, contigs=contigs)
    assert res["rc"] == 3 and "long" in res["out"] and str((1 << 29) + 1) in res["out"] and str(1 << 29) in res["out"]
    res = host(runs, contigs=contigs, index=False)
    check(res, runs, contigs)


def test_malformed_records_are_refused_with_index_and_offset(host):
    good = [rec("a", 0, "c2", 70, "10M", 10), rec("bb", 0, "c1", 5, "12M", 12), rec("c", 0, "c2", 1, "8M", 8)]
    at2 = len(good[0]) + len(good[1])
    whole = b"".join(good)
    short = bytearray(good[1])
    short[0:4] = struct.pack("<I", 31)
    name = bytearray(good[1])
    name[12] = 200  # l_read_name runs past the record
    cases = [
        (whole[:-3], "BAM record 2 at byte %d: " % at2, "past the data's end"),
        (whole + b"\x01\x02", "BAM record 3 at byte %d: " % len(whole), "ends 2 bytes before"),
        (good[0] + bytes(short) + good[2], "BAM record 1 at byte %d: " % len(good[0]), "block_size 31"),
        (good[0] + bytes(name) + good[2], "BAM record 1 at byte %d: " % len(good[0]), "read name"),
    ]
    for data, where, what in cases:
        res = host([(0, good)], raw={0: data})
        assert res["rc"] == 3 and where in res["out"] and what in res["out"], res["out"]
        assert res["tmp_left"] == []
