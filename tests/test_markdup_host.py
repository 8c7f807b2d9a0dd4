"""Duplicate marking on the CPU (include/gwa.h "Duplicate marking"): tests/markdup_host.cpp, a program of its own
built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, runs the host build of the
per-record logic and of both passes (csrc/bam_dup_core.h) and the run sorter with the option
(csrc/bam_sorter.cpp) over the hand-written streams of tests/markdup_cases.py.  End keys, scores, pairing and the
per-run entries must equal tests/markdup_ref.py's; the marked file and its .bai must equal, byte for byte,
tests/bai_ref.py's over the records that markdup_ref marked.  No GPU."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import bai_ref
import bam_ref
import markdup_cases as MC
import markdup_ref as MR
import test_md_host as MH

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = MH.CSRC
CXX = MH.CXX
SLICE = bai_ref.SLICE
CONTIGS = MC.CONTIGS

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("markdup_host")
    exe = d / "markdup_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-pthread", "-DGWA_BAM_SORT_HOST_ONLY", "-I", CSRC] + MH.SAN + [
        "-o", str(exe), os.path.join(HERE, "markdup_host.cpp"), os.path.join(CSRC, "bam_sorter.cpp"), os.path.join(CSRC, "sam.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    count = [0]

    def run(runs, order=None, mem=1 << 30, tmp=False, part=256, mode="1"):
        """runs: [(id, [record])].  Returns dict(rc, out, bam, bai, own {id: [(endKey, score, pairs)]},
        dup {id: [(endKey, mateKey, score, leader)]}, stats, dstats, tmp_left)"""
        count[0] += 1
        w = d / ("w%d" % count[0])
        w.mkdir()
        (w / "contigs").write_text("".join("%s %d\n" % c for c in CONTIGS))
        tdir = w / "tmp"
        tdir.mkdir()
        args = []
        for rid, recs in (runs if order is None else [runs[i] for i in order]):
            f = w / ("run%d" % rid)
            f.write_bytes(b"".join(recs))
            args.append("%d:%s" % (rid, f))
        env = dict(os.environ)
        env.update({"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
        r = subprocess.run([str(exe), str(w / "contigs"), str(mem), str(tdir) if tmp else "-", str(part), str(w / "o.bam"),
                            str(w / "o.bai"), mode] + args, capture_output=True, env=env, timeout=300)
        err = r.stderr.decode(errors="replace")
        for tag in ("Sanitizer", "runtime error"):
            assert tag not in err, err[-6000:]
        assert r.returncode in (0, 3), (r.returncode, err[-4000:])
        res = dict(rc=r.returncode, out=r.stdout.decode(), tmp_left=sorted(os.listdir(tdir)), own={}, dup={})
        if r.returncode == 0:
            res["bam"] = (w / "o.bam").read_bytes()
            res["bai"] = (w / "o.bai").read_bytes()
            for rid, _ in runs:
                res["own"][rid] = list(struct.iter_unpack("<QIB", (w / ("run%d.own" % rid)).read_bytes()))
                res["dup"][rid] = list(struct.iter_unpack("<QQII", (w / ("run%d.dup" % rid)).read_bytes()))
            lines = res["out"].split("\n")
            res["stats"] = [int(x) for x in lines[0].split()[1:]]
            res["dstats"] = dict(zip(MR.STAT_NAMES, (int(x) for x in lines[1].split()[1:])))
        return res

    return run


def expected_file_parts(runs, marked=True):
    """(sorted stream, sorted records, markdup_ref's result): the input-order stream is run-id order"""
    ordered = sorted(runs, key=lambda x: x[0])
    out, ref = MR.mark(ordered)
    allrecs = [r for _, recs in (out if marked else ordered) for r in recs]
    srt = bai_ref.sort_records(allrecs)
    return b"".join(srt), srt, ref


def check(res, runs, marked=True):
    """per-record logic, per-run entries, stats, file and index against the restatements"""
    assert res["rc"] == 0, res["out"]
    stream, srt, ref = expected_file_parts(runs, marked)
    for rid, recs in runs:
        own = res["own"][rid]
        assert len(own) == len(recs)
        for i, r in enumerate(recs):
            k = MR.end_key(r)
            assert own[i][0] == (MR.NO_KEY if k is None else k), (rid, i)
            assert own[i][1] == (MR.own_score(r) & 0xFFFFFFFF if k is not None else 0), (rid, i)
            assert own[i][2] == (1 if i + 1 < len(recs) and MR.is_pair(r, recs[i + 1]) else 0), (rid, i)
        assert res["dup"][rid] == ref["dupinfo"][rid], rid
    if marked:
        assert res["dstats"] == ref["stats"]
    else:
        assert not any(res["dstats"].values())
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    h, sizes = bai_ref.check_file(res["bam"], bai_ref.sorted_header(CONTIGS, text), stream)
    assert res["bai"].hex() == bai_ref.build_bai(srt, len(CONTIGS), sizes, h).hex()
    return stream, srt, ref


def by_name(ref, runs):
    """{read name: template} of an analysis whose names are unique per template"""
    recs = dict(runs)
    return {MR.name(recs[t["run"]][t["first"]])[:-1].decode(): t for t in ref["templates"]}


def test_u5_by_hand():
    for r, u5 in MC.u5_by_hand():
        assert MR.u5(r) == u5
        ref, _, _, _, flag, _ = MR.head(r)
        assert MR.end_key(r) == ref << 33 | ((u5 + (1 << 31)) & 0xFFFFFFFF) << 1 | (flag >> 4 & 1)


def test_u5_on_both_strands_and_every_cigar_shape(host):
    runs = MC.u5_case()
    _, srt, ref = check(host(runs), runs)
    t = by_name(ref, runs)
    assert t["indelB"]["dup"] and t["indelB"]["why"] == "frag" and not t["indelA"]["dup"]
    recs = runs[0][1]
    assert MR.head(recs[-3])[1] != MR.head(recs[-2])[1]  # (their pos differ)
    keys = [MR.end_key(r) for r in recs]
    assert len(set(keys)) > len(MC.U5_CIGARS)  # (the shapes do give different keys)


def test_quality_sums_at_every_offset_and_length(host):
    runs = MC.qual_case()
    check(host(runs), runs)
    recs = [r for _, rs in runs for r in rs]
    starts = set()
    for r in recs:
        _, _, lname, ncig, _, lseq = MR.head(r)
        if lseq:
            starts.add((36 + lname + 4 * ncig + (lseq + 1) // 2) % 16)
    assert starts == set(range(16))
    assert {MR.head(r)[5] for r in recs} >= {0, 1, 15, 16, 17, 255, 256, 257, 512}
    assert any(MR.own_score(r) == 0 and MR.head(r)[5] > 0 for r in recs)
    # 14 and 0xFF count nothing, 15 and 93 count
    assert MR.own_score(MC.rec("a", 0, "c2", 5, "6M", bytes([14, 15, 93, 94, 0xFF, 16]))) == 15 + 93 + 16


def test_pairing(host):
    runs = MC.pairing_case()
    _, _, ref = check(host(runs), runs)
    members = {rid: [t["members"] for t in ref["templates"] if t["run"] == rid] for rid, _ in runs}
    for rid in (0, 1, 2, 3):
        assert members[rid] == [[0], [1]], rid
    assert members[4] == [[0, 1]] and members[5] == [[0, 1]]
    cls = {rid: [t["cls"] for t in ref["templates"] if t["run"] == rid] for rid, _ in runs}
    assert cls[4] == ["frag"] and cls[5] == [None]
    assert members[6] == [[0], [1], [2], [3]]
    assert members[7] == [[0], [1]] and members[8] == [[0], [1]]  # the cut pair: two templates
    assert members[9] == [[0, 1]] and cls[9] == ["pair"]
    assert members[10] == [] and members[11] == [[0]] and members[12] == [[0, 1]]
    assert members[13] == [[0, 1], [2, 3], [4], [5], [6], [7], [8], [9], [10, 11], [12]]


def test_decisions(host):
    runs = MC.decision_case()
    res = host(runs)
    _, srt, ref = check(res, runs)
    t = by_name(ref, runs)
    dup = lambda n: (t[n]["dup"], t[n]["why"])
    assert dup("g2_0") == (True, "pair") and not t["g2_1"]["dup"]
    assert [t["g5_%d" % i]["dup"] for i in range(5)] == [True, True, False, True, True]
    assert not t["fr"]["dup"] and not t["rf"]["dup"]
    assert not t["sw1"]["dup"] and dup("sw2") == (True, "pair")
    assert not t["tie_a"]["dup"] and t["tie_b"]["dup"]
    assert not t["xt_0"]["dup"] and t["xt_1"]["dup"] and t["xt_3"]["dup"]
    assert not t["clip_a"]["dup"] and t["clip_b"]["dup"]
    assert [t["eq_%d" % i]["dup"] for i in range(3)] == [True, False, True]
    assert t["eq_0"]["sig"][0] == t["eq_0"]["sig"][1]
    assert dup("fa") == (True, "frag") and not t["fb"]["dup"] and dup("fc") == (True, "frag") and not t["fd"]["dup"]
    assert all(dup("pe_f%d" % i) == (True, "pair end") for i in (1, 2, 3))
    assert t["half"]["cls"] == "frag" and dup("half") == (True, "frag") and not t["plain"]["dup"] and t["plain2"]["dup"]
    for n in ("star", "star2", "sec", "sup", "unm", "other"):
        assert not t[n]["dup"], n
    # only participating records carry the flag: the unmapped mate of `half` does not
    flagged = {bam_ref.render(r, CONTIGS).split("\t")[0]: int(bam_ref.render(r, CONTIGS).split("\t")[1]) for r in srt
               if MR.head(r)[4] & 0x400}
    assert "half" in flagged and flagged["half"] & 0x40 and len([r for r in srt if MR.name(r) == b"half\0" and MR.head(r)[4] & 0x400]) == 1
    # runs added in reversed and shuffled id order: the same bytes
    for order in ([4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        other = host(runs, order=order)
        assert other["bam"] == res["bam"] and other["bai"] == res["bai"] and other["dstats"] == res["dstats"]


def test_sorter_marked_file_in_memory_spilled_and_shuffled(host):
    runs = MC.world_case()
    res = host(runs)
    _, srt, ref = check(res, runs)
    assert ref["stats"]["dup_pair_templates"] >= 3 and ref["stats"]["dup_frag_templates"] >= 3
    assert sum(t["why"] == "pair end" for t in ref["templates"]) >= 3
    assert sum(len(r) for r in srt) > 2 * SLICE
    n = len(runs)
    shuffled = list(range(n))
    random.Random(3).shuffle(shuffled)
    for kw in (dict(mem=0, tmp=True), dict(order=shuffled), dict(part=1), dict(mem=30000, tmp=True, part=1, order=shuffled[::-1])):
        other = host(runs, **kw)
        assert other["rc"] == 0, other["out"]
        assert other["bam"] == res["bam"] and other["bai"] == res["bai"] and other["dstats"] == res["dstats"], kw
        assert other["tmp_left"] == [], kw
        if kw.get("mem") == 0:
            assert other["stats"][2] == other["stats"][1] == n  # every run spilled
    # one run holding everything: the same marks (pairs are never cut here: the batch size does not matter)
    one = [(0, [r for _, recs in sorted(runs, key=lambda x: x[0]) for r in recs])]
    assert host(one)["bam"] == res["bam"]


def test_option_off_gives_the_unmarked_bytes_and_late_setting_fails(host):
    runs = MC.decision_case()
    off = host(runs, mode="0")
    check(off, runs, marked=False)
    assert off["bam"] != host(runs)["bam"]
    late = host(runs, mode="late")
    assert late["rc"] == 3 and "gwa_bam_sorter_set_markdup" in late["out"] and "before the first run" in late["out"]


@pytest.mark.parametrize("kw", [dict(), dict(mem=0, tmp=True)])
def test_flag_byte_on_the_first_and_the_last_byte_of_a_part(host, kw):
    runs, starts = MC.edge_case()
    res = host(runs, part=1, **kw)
    stream, srt, ref = check(res, runs)
    assert starts[0] + 19 == SLICE and (starts[1] + 19) % SLICE == SLICE - 1
    at, hit = 0, 0
    for r in srt:
        if at in starts:
            assert MR.head(r)[4] & 0x400 and MR.name(r) in (b"d1\0", b"d2\0")
            hit += 1
        at += len(r)
    assert hit == 2 and ref["stats"]["dup_records"] == 2
    assert host(runs)["bam"] == res["bam"]
