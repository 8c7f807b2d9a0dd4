"""Duplicate marking on the device (include/gwa.h "Duplicate marking": gwa_bam_records_dupinfo,
gwa_batch_results_bam_dupinfo, gwa_bam_sorter_set_markdup, gwa_pipeline_set_markdup, align --markdup).

The per-run kernel's entries and the device resolve are compared with tests/markdup_ref.py (a restatement of the
rule in Python) and with the host build (device -1) on the hand-written streams of tests/markdup_cases.py, and
on aligned batches.  Two worlds of about 600 templates over test_gpu_bam_sort's genome -- single reads, and
pairs with half-unmappable ones, a third of them copies of earlier templates under new names and other
qualities -- go through the sorter, the pipeline and the command line: every variant must give, byte for byte,
the file and the .bai that tests/bai_ref.py gives for the records markdup_ref marked."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import bai_ref  # noqa: E402
import bam_ref  # noqa: E402
import markdup_cases as MC  # noqa: E402
import markdup_ref as MR  # noqa: E402
import test_gpu_bam as B  # noqa: E402
import test_gpu_bam_sort as S  # noqa: E402
import test_gpu_bgzf as Z  # noqa: E402
import test_gpu_md as M  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 97


@pytest.fixture(scope="module")
def world():
    w = S.World()
    assert [n for n, _ in w.contig_table[:3]] == [n for n, _ in MC.CONTIGS]  # (the cases' refIDs name its contigs)
    yield w
    w.fm.close()


def stats_of(st):
    return {n: getattr(st, n) for n in MR.STAT_NAMES}


def sorter_file(world, tmp_path, feed, device=None, **kw):
    """header + a marking sorter fed by feed(sorter) + EOF: (file bytes, bai bytes, markdup stats, sorter stats)"""
    s = gwa.BamSorter(world.fm, device=device, markdup=True, **kw)
    try:
        feed(s)
        _, data, bai, st = S.finish(world, s, tmp_path)
        return data, bai, stats_of(s.markdup_stats()), st
    finally:
        s.close()


def expected(world, runs):
    """(file bytes, bai bytes, sorted marked records, markdup_ref's result) for runs [(id, [record])]"""
    out, ref = MR.mark(sorted(runs, key=lambda x: x[0]))
    want = bai_ref.sort_records([r for _, recs in out for r in recs])
    stream = b"".join(want)
    hdr = bai_ref.sorted_header(world.contig_table, world.fm.samHeader())
    data = gwa.bgzf_compress(hdr) + (gwa.bgzf_compress(stream) if stream else b"") + gwa.BGZF_EOF
    h, sizes = bai_ref.check_file(data, hdr, stream)
    return data, bai_ref.build_bai(want, len(world.contig_table), sizes, h), want, ref


HAND_CASES = {"u5": MC.u5_case, "qual": MC.qual_case, "pairing": MC.pairing_case, "decision": MC.decision_case,
              "edge": lambda: MC.edge_case()[0], "world": MC.world_case}


@pytest.mark.parametrize("case", list(HAND_CASES))
def test_hand_written_streams_entries_and_marked_file(world, tmp_path, case):
    runs = HAND_CASES[case]()
    data, bai, want, ref = expected(world, runs)
    for rid, recs in runs:
        if not recs:
            continue
        blob = b"".join(recs)
        got = gwa.bam_records_dupinfo(blob, device=0)
        assert got == ref["dupinfo"][rid], (case, rid)
        assert gwa.bam_records_dupinfo(blob, device=-1) == got

    def feed(s):
        for rid, recs in runs[::-1]:
            s.add_records(rid, b"".join(recs))

    d_dev, b_dev, st_dev, _ = sorter_file(world, tmp_path, feed)
    assert st_dev == ref["stats"]
    assert (d_dev, b_dev.hex()) == (data, bai.hex())
    d_host, b_host, st_host, _ = sorter_file(world, tmp_path, feed, device=-1)
    assert (d_host, b_host, st_host) == (d_dev, b_dev, st_dev)
    if case == "decision":
        assert ref["stats"]["dup_pair_templates"] >= 10 and ref["stats"]["dup_frag_templates"] >= 7
    # the option off: the unmarked bytes
    s = gwa.BamSorter(world.fm)
    try:
        for rid, recs in runs:
            s.add_records(rid, b"".join(recs))
        stream, _, _, _ = S.finish(world, s, tmp_path)
        assert not any(stats_of(s.markdup_stats()).values())
    finally:
        s.close()
    assert stream == b"".join(bai_ref.sort_records([r for _, recs in sorted(runs, key=lambda x: x[0]) for r in recs]))


def test_set_markdup_after_an_add_fails_and_the_timed_kernel_counts(world):
    recs = MC.decision_case()[0][1]
    s = gwa.BamSorter(world.fm)
    try:
        s.add_records(0, b"".join(recs))
        with pytest.raises(gwa.GwaError, match="gwa_bam_sorter_set_markdup.*before the first run"):
            s.set_markdup(True)
    finally:
        s.close()
    n, ms = gwa.bam_markdup_timed(b"".join(recs), device=0, repeat=2)
    assert n == len(recs) and ms > 0
    with pytest.raises(gwa.GwaError, match="BAM record 1 at byte"):
        gwa.bam_records_dupinfo(recs[0] + recs[1][:-1], device=0)


def check_batch(b):
    """the batch's entries, in sorted order, against the restatement over its unsorted records"""
    recs = bam_ref.records(b.results_bam_records())
    srt, keys = b.results_bam_sorted()
    got = b.results_bam_dupinfo()
    info = MR.analyse([(0, recs)])["dupinfo"][0] if recs else []
    order = sorted(range(len(recs)), key=lambda i: bai_ref.key(recs[i]))  # (stable)
    assert got == [info[i] for i in order]
    assert b.results_bam_sorted() == (srt, keys)  # the sort's own results stay as they were
    if recs:
        assert gwa.bam_records_dupinfo(b"".join(recs), device=-1) == info
    return recs, got


@pytest.mark.parametrize("md", [False, True])
@pytest.mark.parametrize("case", ["besthit", "allhits", "s2", "sf", "pairs"])
def test_batch_entries(world, case, md):
    if case == "pairs":
        b = B.pair_batch(world, md)
    else:
        b = gwa.Batch(world.fm, gwa.AlignmentConfig(mdTag=md, **B.CASES[case][0]), reads=world.case_reads(case))
    try:
        b.run()
        recs, got = check_batch(b)
    finally:
        b.close()
    assert len(recs) >= 200 and any(k != MR.NO_KEY for k, _, _, _ in got) and any(k == MR.NO_KEY for k, _, _, _ in got)
    if case == "pairs":
        assert sum(m != MR.NO_KEY for _, m, _, _ in got) >= 100  # pair templates with both mates participating
    if case == "s2":
        assert any(m != MR.NO_KEY for _, m, _, _ in got)  # the pieces of a split read are a pair


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_long_reads(world, n):
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=5.0, reportType="allhits"), reads=world.case_reads("allhits")[5:5 + n])
    try:
        b.run()
        check_batch(b)
    finally:
        b.close()
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0), pair_blobs=(Z.blobs(world.m1[:n]), Z.blobs(world.m2[:n])))
    try:
        b.run()
        check_batch(b)
    finally:
        b.close()
    if n == 1:
        s = world.seqs[0]
        b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0, mdTag=True), reads=[("L", s[700:1212], "F" * 300 + "#" * 212)])
        try:
            b.run()
            recs, got = check_batch(b)
            assert len(recs) == 1 and got[0][2] == 300 * (ord("F") - 33)
        finally:
            b.close()


# ---- the two worlds of templates ----

def make_templates(seqs, kind, seed):
    """(mates 1, mates 2 or None): about 600 templates, a third of them copies of earlier ones under new names
    and with other qualities; kind "single": reads of 100 bases; "pairs": mates of 100 bases from fragments of
    250-350, one pair in five with a random second mate"""
    rng = random.Random(seed)
    srcs, m1, m2 = [], [], []
    for i in range(600):
        if srcs and rng.random() < 0.34:
            src = rng.choice(srcs)
            if kind == "pairs" and not src[4] and rng.random() < 0.3:
                src = src[:4] + (True,)  # the copy of a pair loses its second mate: a fragment at the pair's end
        else:
            c = rng.randrange(3)
            f = rng.randrange(250, 351)
            src = (c, rng.randrange(0, len(seqs[c]) - f), f, rng.random() < 0.5, kind == "pairs" and rng.random() < 0.2)
            if "N" in seqs[c][src[1]:src[1] + f]:
                continue
        srcs.append(src)
        c, a, f, flip, half = src
        frag = seqs[c][a:a + f]
        x, y = frag[:100], M.revcomp(frag[f - 100:])
        if half:
            y = "".join(rng.choice("ACGT") for _ in range(100))
        if flip and kind == "single":
            x = M.revcomp(x)
        if rng.random() < 0.3:
            q1 = q2 = "I" * 100  # (score ties)
        else:
            q1, q2 = ("".join(rng.choice("#+05:?DI") for _ in range(100)) for _ in range(2))
        if flip and kind == "pairs":
            x, y, q1, q2 = y, x, q2, q1
        m1.append(("t%d" % i, x, q1))
        m2.append(("t%d" % i, y, q2))
    return (m1, None) if kind == "single" else (m1, m2)


class Templates:
    def __init__(self, world, kind):
        self.kind = kind
        self.m1, self.m2 = make_templates(world.seqs, kind, 31 if kind == "single" else 32)
        cfg = gwa.AlignmentConfig(k=2.0)
        self.batches = []
        for at in range(0, len(self.m1), BATCH):
            if kind == "single":
                b = gwa.Batch(world.fm, cfg, reads=self.m1[at:at + BATCH])
            else:
                b = gwa.Batch(world.fm, cfg, pair_blobs=(Z.blobs(self.m1[at:at + BATCH]), Z.blobs(self.m2[at:at + BATCH])))
            b.run()
            self.batches.append(b)
        self.runs = [(i, bam_ref.records(b.results_bam_records())) for i, b in enumerate(self.batches)]
        self.data, self.bai, self.want, self.ref = expected(world, self.runs)

    def close(self):
        for b in self.batches:
            b.close()


@pytest.fixture(scope="module", params=["single", "pairs"])
def temps(world, request):
    t = Templates(world, request.param)
    yield t
    t.close()


def test_the_reference_result_holds_every_class(temps):
    """on markdup_ref's result alone: the worlds cannot pass vacuously"""
    ts = temps.ref["templates"]
    groups = {}
    for t in ts:
        if t["cls"]:
            groups.setdefault((t["cls"], t["sig"]), []).append(t)
    cross = sum(1 for g in groups.values() if any(t["dup"] for t in g) and len({t["run"] for t in g}) > 1)
    ties = sum(1 for g in groups.values() if len(g) > 1 and sorted(t["score"] for t in g)[-1] == sorted(t["score"] for t in g)[-2])
    assert sum(t["why"] == "frag" for t in ts) >= 3 and cross >= 3 and ties >= 3
    if temps.kind == "pairs":
        assert sum(t["why"] == "pair" for t in ts) >= 3 and sum(t["why"] == "pair end" for t in ts) >= 3
        assert sum(t["cls"] == "frag" and len(t["members"]) == 2 for t in ts) >= 3  # half-mapped pairs
    assert len(ts) >= 550 and len(temps.runs) >= 6
    assert sum(1 for r in temps.want if MR.head(r)[4] & 0x400) == temps.ref["stats"]["dup_records"] >= 20


def test_sorter_over_batches_reversed_shuffled_and_spilled(world, temps, tmp_path):
    n = len(temps.batches)
    order = list(range(n))
    random.Random(4).shuffle(order)
    spill = tmp_path / "spill"
    spill.mkdir()
    for feed_order, kw in ((list(range(n))[::-1], {}), (order, dict(tmp_dir=str(spill), mem=20000))):
        def feed(s):
            for i in feed_order:
                s.add_batch(i, temps.batches[i])
        data, bai, st, sst = sorter_file(world, tmp_path, feed, **kw)
        assert st == temps.ref["stats"]
        assert (data, bai.hex()) == (temps.data, temps.bai.hex()), kw
        if kw:
            assert sst.spilled_runs >= n - 2 and os.listdir(spill) == []
    # the same records through the host build, and unmarked without the option
    def feed_records(s):
        for rid, recs in temps.runs:
            s.add_records(rid, b"".join(recs))
    data, bai, st, _ = sorter_file(world, tmp_path, feed_records, device=-1)
    assert (data, bai, st) == (temps.data, temps.bai, temps.ref["stats"])


def test_pipeline_and_cli(world, temps, tmp_path, capsys):
    f1, f2 = tmp_path / "t_1.fq", tmp_path / "t_2.fq"
    Z.write_fastq(f1, temps.m1)
    if temps.m2:
        Z.write_fastq(f2, temps.m2)
    hdr = gwa.bgzf_compress(world.fm.bam_header(sorted=True))
    spill = tmp_path / "spill"
    spill.mkdir()

    def run(pipe, **sort):
        path = tmp_path / "p.bam"
        with open(path, "wb") as f, open(str(path) + ".bai", "wb") as fb:
            f.write(hdr)
            f.flush()
            pipe.set_sort(index=fb.fileno(), **sort)
            pipe.set_markdup(True)
            if temps.m2:
                pipe.align_pair_files(str(f1), str(f2), f.fileno())
            else:
                pipe.align_file(str(f1), f.fileno())
            os.write(f.fileno(), gwa.BGZF_EOF)
        return path.read_bytes(), open(str(path) + ".bai", "rb").read(), stats_of(pipe.markdup_stats())

    for batch_reads, workers in ((BATCH, 1), (BATCH, 3), (1024, 3)):
        pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=batch_reads, workers_per_device=workers, output="bam")
        try:
            assert run(pipe) == (temps.data, temps.bai, temps.ref["stats"]), (batch_reads, workers)
            if workers == 3 and batch_reads == BATCH:
                assert run(pipe, tmp_dir=str(spill), mem=20000) == (temps.data, temps.bai, temps.ref["stats"])
                assert pipe.sort_stats().spilled_runs >= 3 and os.listdir(spill) == []
        finally:
            pipe.close()
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=BATCH, output="bam")
    try:
        with pytest.raises(gwa.GwaError, match="gwa_pipeline_set_markdup.*sorts"):
            pipe.set_markdup(True)
    finally:
        pipe.close()
    # the command line
    import gwa_cli
    ref = tmp_path / "ref.fa"
    ref.write_text(world.fasta)
    files = [str(f1)] + ([str(f2)] if temps.m2 else [])
    base = ["align", "-r", str(ref), "-k", "2", "--batch", str(BATCH)]
    out = tmp_path / "cli.bam"
    assert gwa_cli.main(base + ["--bam", "--sort", "--index", "--markdup", "--timing", "-o", str(out)] + files) == 0
    err = capsys.readouterr().err
    st = temps.ref["stats"]
    assert "[gwa] markdup: %d templates (%d pair, %d fragment), duplicates: %d pair and %d fragment templates, %d records" % (
        st["templates"], st["pair_templates"], st["frag_templates"], st["dup_pair_templates"], st["dup_frag_templates"],
        st["dup_records"]) in err
    data, bai = out.read_bytes(), open(str(out) + ".bai", "rb").read()
    assert (data, bai) == (temps.data, temps.bai)
    rng = random.Random(6)
    hits = 0
    for _ in range(12):
        r = rng.randrange(3)
        a = rng.randrange(0, world.contig_table[r][1])
        got = bai_ref.query(data, bai, r, a, a + 2000)
        assert got == bai_ref.brute_force(temps.want, r, a, a + 2000)
        hits += any(MR.head(x)[4] & 0x400 for x in got)
    assert hits >= 1
    if temps.kind == "single":  # the refusals, and a failing run leaves no index
        for extra, msg in ((["--bam", "--markdup", "-o", str(tmp_path / "x.bam")], "--markdup needs --bam --sort"),
                           (["--sort", "--markdup", "-o", str(tmp_path / "x.sam")], "--sort needs --bam")):
            assert gwa_cli.main(base + extra + files) == 1
            assert msg in capsys.readouterr().err
        bad = tmp_path / "bad.fq"
        Z.write_fastq(bad, temps.m1[:5] + [("k" * 255,) + temps.m1[5][1:]] + temps.m1[6:10])
        assert gwa_cli.main(base + ["--bam", "--sort", "--index", "--markdup", "-o", str(tmp_path / "bad.bam"), str(bad)]) == 1
        assert "has a name of 255 bytes" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "bad.bam") + ".bai")
