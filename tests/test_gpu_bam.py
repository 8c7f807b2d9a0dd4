"""BAM records built on the device (include/gwa.h GWA_OUT_BAM, gwa_batch_results_bam_records / _bam,
gwa_bam_header; gwa_cli align --bam).

A record is a function of the printed SAM line, so every case compares the device's records, byte for byte,
with tests/bam_ref.py's encoding of the SAM text the same batch prints (the text itself is held to the oracle
by the other GPU tests).  The world is the small one of tests/test_gpu_md.py (its generators, imported): a
9.5 kb genome of three contigs, 600 reads of 40-300 bp (the 300 bp reads the oracle aligns under a case's
options, as there), 240 pairs; added here are an empty, a one-base, an all-N and a lowercase read, a batch
without qualities and a batch where every third read has none.  Each case asserts on the plain text that the
lines it is for are there: a split-record pair, an S inside a CIGAR, POS <= 0, an unmapped and a
reverse-strand line (-m sf and -s 0 report no split chains: they print neither of the first two, and a line
over a contig's end stands in for POS <= 0)."""
import io
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import bam_ref  # noqa: E402
import test_gpu_bgzf as Z  # noqa: E402
import test_gpu_md as M  # noqa: E402

pytestmark = pytest.mark.gpu

SLICE = 65280
# case: gwa options, the oracle's options (to find the 300 bp reads it aligns), split chains reported
CASES = {
    "besthit": (dict(k=2.0), dict(k=2.0), True),
    "allhits": (dict(k=5.0, reportType="allhits"), dict(k=5.0, report_type=1), True),
    "s0": (dict(k=2.0, numSplitAlowed=0), dict(k=2.0, num_split=0), False),
    "s2": (dict(k=2.0, numSplitAlowed=2), dict(k=2.0, num_split=2), True),
    "sf": (dict(k=5.0, strategy="sf"), dict(k=5.0, strategy=1), False),
}


class World(M.World):
    def __init__(self):
        super().__init__()
        s = self.seqs[0]
        self.extra = [("e0", "", ""), ("one", "A", "I"), ("star", "C", "*"), ("allN", "N" * 50, "5" * 50),
                      ("lower", s[100:164].lower(), "J" * 64), ("odd", s[200:241], "!" + "~" * 39 + "!")]
        self.contig_table = [(n, len(x)) for n, x in zip(self.names, self.seqs)]
        self._kept, self._out = {}, {}

    def case_reads(self, case):
        """the case's reads: the extras and the generated reads, without the 300 bp, empty and one-base reads on
        which the oracle throws under the case's options"""
        if case not in self._kept:
            cfg = self.O.OrcConfig.default(**CASES[case][1])
            keep = []
            for r in self.extra + self.reads:
                if len(r[1]) > 223 or len(r[1]) < 2:  # (-m sf: the reference throws on an empty read)
                    try:
                        self.oi.align([r], cfg)
                    except RuntimeError:
                        continue
                keep.append(r)
            self._kept[case] = keep
        return self._kept[case]

    def outputs(self, case, md):
        """(SAM text, BAM records) of one batch of the case, computed once"""
        if (case, md) not in self._out:
            b = gwa.Batch(self.fm, gwa.AlignmentConfig(mdTag=md, **CASES[case][0]), reads=self.case_reads(case))
            try:
                b.run()
                rec = b.results_bam_records()
                sam = b.results()[0]
                assert b.results_bam_records() == rec  # (a SAM formatting in between changes nothing)
            finally:
                b.close()
            self._out[(case, md)] = (sam, rec)
        return self._out[(case, md)]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.fm.close()


def check(world, sam, rec, md):
    want = bam_ref.encode_text(sam, world.contig_table, md=md)
    if rec != want:  # name the first differing line
        got = bam_ref.records(rec)
        for line, g in zip(sam.split("\n"), got):
            assert g.hex() == bam_ref.encode_line(line, world.contig_table, md=md).hex(), line
        assert len(got) == sam.count("\n")
    assert rec == want
    for line, g in zip(sam.split("\n"), bam_ref.records(rec)):
        assert bam_ref.render(g, world.contig_table) == bam_ref.normalise(line)


@pytest.mark.parametrize("md", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_single_end_records(world, case, md):
    sam, rec = world.outputs(case, md)
    have = M.claims(sam, world.contigs)
    need = {"unmapped", "reverse"} | ({"split", "midS", "pos<=0"} if CASES[case][2] else set())
    assert need <= have and have & {"pos<=0", "past end"}, (case, sorted(have))
    assert {len(r[1]) for r in world.case_reads(case)} >= {40, 41, 50, 64, 100, 129, 300} | (set() if case == "sf" else {0, 1})
    assert ("\tMD:Z:" in sam) == md
    check(world, sam, rec, md)


def test_no_qualities_and_a_qual_null_mix(world):
    reads = world.case_reads("besthit")
    for pick in (lambda i, r: (r[0], r[1], None), lambda i, r: (r[0], r[1], None if i % 3 == 0 else r[2])):
        b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0), reads=[pick(i, r) for i, r in enumerate(reads)])
        try:
            b.run()
            sam, rec = b.results()[0], b.results_bam_records()
        finally:
            b.close()
        quals = [l.split("\t")[10] for l in sam.splitlines()]
        assert quals.count("*") >= len(reads) // 3
        check(world, sam, rec, False)


def pair_batch(world, md):
    return gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0, mdTag=md), pair_blobs=(Z.blobs(world.m1), Z.blobs(world.m2)))


@pytest.mark.parametrize("md", [False, True])
def test_paired_records(world, md):
    text = gwa.PairedEndAligner(world.fm, gwa.AlignmentConfig(k=2.0, mdTag=md)).align_pairs(world.m1, world.m2)
    have = M.claims(text, world.contigs)
    assert {"reverse", "unmapped", "mate unmapped"} <= have, sorted(have)
    # pairs whose second mate is found by the rescue only: unmapped as a single-end read at this k
    lone = gwa.aligner(world.fm, gwa.AlignmentConfig(k=2.0)).align_batch(
        [world.m2[i] for i in range(1, M.N_PAIRS, 6)] + [world.m1[i] for i in range(1, M.N_PAIRS, 6)])
    lone = {l.split("\t")[0] for l in lone.splitlines() if int(l.split("\t")[1]) & 0x4}
    assert [l for l in text.splitlines() if l.split("\t")[0] in lone and int(l.split("\t")[1]) & 0x2], "no rescued mate"
    b = pair_batch(world, md)
    try:
        b.run()
        rec = b.results_bam_records()
        assert b.results()[0] == text
    finally:
        b.close()
    assert rec.count(b"MDZ") > 0 if md else True
    check(world, text, rec, md)


def test_both_write_paths_and_determinism(world, monkeypatch):
    """a 1 KiB stage (most workgroups write directly), no deferral (every lane packs its own fields), and the
    default: three equal byte streams; formatting twice gives the same bytes"""
    case, md = "allhits", True
    want = world.outputs(case, md)[1]
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(mdTag=md, **CASES[case][0]), reads=world.case_reads(case))
    try:
        b.run()
        assert b.results_bam_records() == want and b.results_bam_records() == want
        assert b.format_bam() == len(want)
        st = b.stats()
        assert st.bam_bytes == len(want) and st.bam_ms > 0
        for env in (("GWA_SAM_STAGE", "1024"), ("GWA_SAM_DEFER", "0")):
            monkeypatch.setenv(*env)
            assert b.results_bam_records() == want, env
            monkeypatch.delenv(env[0])
    finally:
        b.close()
    b = pair_batch(world, md)
    try:
        b.run()
        want = b.results_bam_records()
        for env in (("GWA_SAM_STAGE", "1024"), ("GWA_SAM_DEFER", "0")):
            monkeypatch.setenv(*env)
            assert b.results_bam_records() == want, env
            monkeypatch.delenv(env[0])
    finally:
        b.close()


def test_results_bam_blocks(world):
    """the compressed form: one block per 65 280 bytes of records, the host encoder's bytes"""
    for case, paired in (("allhits", False), (None, True), ("bd", False)):
        if paired:
            b = pair_batch(world, False)
        elif case == "bd":
            b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0, strategy="bd"), reads=world.case_reads("besthit"))
        else:
            b = gwa.Batch(world.fm, gwa.AlignmentConfig(**CASES[case][0]), reads=world.case_reads(case))
        try:
            b.run()
            rec = b.results_bam_records()
            z = b.results_bam()
            blocks = bam_ref.bgzf_blocks(z)
            assert b"".join(raw for _, raw in blocks) == rec
            assert len(blocks) == math.ceil(len(rec) / SLICE)
            assert z == gwa.bgzf_compress(rec)
            st = b.stats()
            assert (st.bgzf_blocks, st.bgzf_bytes, st.bam_bytes) == (len(blocks), len(z), len(rec))
            if case == "bd":
                assert rec == b"" and z == b""
            else:
                assert len(z) < len(rec)
            if case == "allhits":
                assert len(blocks) >= 2  # (records straddle a slice edge)
                with pytest.raises(gwa.GwaError):  # the last formatting was not gwa_batch_format's
                    b.sam_device()
        finally:
            b.close()


def test_header(world):
    hdr = world.fm.bam_header()
    assert hdr == bam_ref.header(world.contig_table, world.fm.samHeader())
    assert bam_ref.contigs_of(world.fm.samHeader()) == world.contig_table


def decode(world, body):
    """header + body + EOF as a file: its lines"""
    data = gwa.bgzf_compress(world.fm.bam_header()) + body + gwa.BGZF_EOF
    text, contigs, lines = bam_ref.decode_file(data)
    assert text == world.fm.samHeader() and contigs == world.contig_table
    return lines


def test_pipeline_bam_output(world, tmp_path):
    cfg = gwa.AlignmentConfig(k=2.0)
    reads = [r for r in world.case_reads("besthit") if r[0] != "star"]
    fq = tmp_path / "reads.fq"
    Z.write_fastq(fq, reads)
    f1, f2 = tmp_path / "m_1.fq", tmp_path / "m_2.fq"
    Z.write_fastq(f1, world.m1)
    Z.write_fastq(f2, world.m2)
    assert len(reads) % 97
    text_pipe = gwa.Pipeline([world.fm], cfg, batch_reads=97)
    try:
        plain = Z.run_to("file", tmp_path, lambda fd: text_pipe.align_file(str(fq), fd)).decode()
        plain_pairs = Z.run_to("file", tmp_path, lambda fd: text_pipe.align_pair_files(str(f1), str(f2), fd)).decode()
        assert plain.count("\n") >= len(reads) and plain_pairs.count("\n") == 2 * M.N_PAIRS
    finally:
        text_pipe.close()
    for workers, kinds in ((1, ("file", "append", "pipe")), (3, ("file", "pipe"))):
        pipe = gwa.Pipeline([world.fm], cfg, batch_reads=97, workers_per_device=workers, output="bam")
        try:
            for kind in kinds:
                z = Z.run_to(kind, tmp_path, lambda fd: pipe.align_file(str(fq), fd))
                assert decode(world, z) == [bam_ref.normalise(l) for l in plain.splitlines()], (workers, kind)
                assert bam_ref.inflate(z) == bam_ref.encode_text(plain, world.contig_table)
                # every batch is its own run of blocks: a short block at each batch end
                assert len(bam_ref.bgzf_blocks(z)) >= math.ceil(len(reads) / 97)
                assert pipe.stats().out_bytes == len(z)
            z = Z.run_to("file", tmp_path, lambda fd: pipe.align_pair_files(str(f1), str(f2), fd))
            assert decode(world, z) == [bam_ref.normalise(l) for l in plain_pairs.splitlines()]
            assert bam_ref.inflate(z) == bam_ref.encode_text(plain_pairs, world.contig_table)
            assert "\t" in pipe.align_batch(reads[:20])  # (the in-memory calls return text either way)
            # a pipeline is opened for BAM; set_output switches between the two forms of the text only
            with pytest.raises(gwa.GwaError, match="output=.bam"):
                pipe.set_output("bam")
            pipe.set_output("sam")
            assert Z.run_to("file", tmp_path, lambda fd: pipe.align_file(str(fq), fd)).decode() == plain
            # the C call takes the format at any time, and names it in the error for an unknown one
            L = gwa.lib()
            assert L.gwa_pipeline_set_output(pipe.h, 2) == 0
            z = Z.run_to("file", tmp_path, lambda fd: pipe.align_file(str(fq), fd))
            assert bam_ref.inflate(z) == bam_ref.encode_text(plain, world.contig_table)
            assert L.gwa_pipeline_set_output(pipe.h, 7) != 0
            assert "GWA_OUT_BAM = 2" in L.gwa_last_error().decode()
        finally:
            pipe.close()


def test_a_long_name_fails_the_batch(world):
    reads = list(world.case_reads("besthit")[:70])
    reads[66] = ("k" * 255, reads[66][1], reads[66][2])
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0), reads=reads)
    try:
        b.run()
        assert b.results()[0].count("k" * 255) >= 1  # (SAM carries the name)
        with pytest.raises(gwa.GwaError, match=r"BAM: read 66 has a name of 255 bytes \(at most 254"):
            b.results_bam_records()
        with pytest.raises(gwa.GwaError, match="read 66 has a name of 255 bytes"):
            b.results_bam()
    finally:
        b.close()
    reads[66] = ("k" * 254, reads[66][1], reads[66][2])
    b = gwa.Batch(world.fm, gwa.AlignmentConfig(k=2.0), reads=reads)
    try:
        b.run()
        check(world, b.results()[0], b.results_bam_records(), False)
    finally:
        b.close()


def test_cli_bam(tmp_path, capsys):
    """gwa_cli align --bam over tests/golden/fixtures/reads_c1.fq.snap: -o FILE decodes to what align prints as
    text, alone, with --md and as two shards concatenated; --bam --bgzf is refused; -m bd is header + EOF; -q;
    a 255-byte name fails with the message"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gwa_cli
    import snap_reads
    import synth
    codes, names, lengths = snap_reads.genome()
    ref = tmp_path / "ref.fa"
    ref.write_text(synth.fasta_text(codes, names, lengths))
    snap = os.path.join(HERE, "golden", "fixtures", "reads_c1.fq.snap")
    reads = list(gwa_cli.reads_of(snap))
    fq = tmp_path / "reads.fq"
    Z.write_fastq(fq, reads)
    base = ["align", "-r", str(ref), "-k", "2", "--batch", "64"]

    def text_of(extra, path):
        out = io.StringIO()
        assert gwa_cli.align(gwa_cli.build_parser().parse_args(base + extra + [path]), out=out) == len(reads)
        return out.getvalue()

    def lines_of(data, plain):
        text, contigs, lines = bam_ref.decode_file(data)
        hdr = "".join(l + "\n" for l in plain.splitlines() if l.startswith("@"))
        assert text == hdr and contigs == bam_ref.contigs_of(hdr)
        assert data.count(gwa.BGZF_EOF) == 1
        return lines

    for md in ([], ["--md"]):
        plain = text_of(md, snap)
        want = [bam_ref.normalise(l) for l in plain.splitlines() if not l.startswith("@")]
        out = tmp_path / "x.bam"
        assert gwa_cli.main(base + md + ["--bam", "-o", str(out), snap]) == 0
        assert lines_of(out.read_bytes(), plain) == want
        assert any("MD:Z:" in l for l in want) == bool(md)
    plain = text_of([], snap)
    want = [bam_ref.normalise(l) for l in plain.splitlines() if not l.startswith("@")]
    # shards of the plain file
    parts = []
    for r in (0, 1):
        out = tmp_path / ("s%d.bam" % r)
        assert gwa_cli.main(base + ["--bam", "--shard", "%d/2" % r, "-o", str(out), str(fq)]) == 0
        parts.append(out.read_bytes())
    assert not parts[0].endswith(gwa.BGZF_EOF) and parts[1].endswith(gwa.BGZF_EOF)
    assert lines_of(parts[0] + parts[1], plain) == want
    # --bam --bgzf
    assert gwa_cli.main(base + ["--bam", "--bgzf", "-o", str(tmp_path / "no.bam"), snap]) == 1
    assert "--bam and --bgzf" in capsys.readouterr().err
    # -m bd: the header and the EOF marker
    out = io.BytesIO()
    gwa_cli.align(gwa_cli.build_parser().parse_args(base + ["--bam", "-m", "bd", snap]), out=out)
    assert lines_of(out.getvalue(), plain) == []
    fm_hdr = bam_ref.header(bam_ref.contigs_of(plain), "".join(l + "\n" for l in plain.splitlines() if l.startswith("@")))
    assert out.getvalue() == gwa.bgzf_compress(fm_hdr) + gwa.BGZF_EOF
    # -q: one query, one batch; the text run through -o FILE
    out = io.BytesIO()
    ns = gwa_cli.build_parser().parse_args(["align", "-r", str(ref), "-k", "2", "--bam", "-q", reads[0][1]])
    assert gwa_cli.align(ns, out=out) == 1
    tout = tmp_path / "q.sam"
    assert gwa_cli.main(["align", "-r", str(ref), "-k", "2", "-q", reads[0][1], "-o", str(tout)]) == 0
    qtext = tout.read_text()
    assert qtext.startswith("@SQ") and qtext.splitlines()[-1].startswith("read\t")
    assert lines_of(out.getvalue(), qtext) == [bam_ref.normalise(l) for l in qtext.splitlines() if not l.startswith("@")]
    # a name that does not fit a record
    bad = tmp_path / "bad.fq"
    Z.write_fastq(bad, reads[:5] + [("k" * 255, reads[5][1], reads[5][2])] + reads[6:10])
    assert gwa_cli.main(base + ["--bam", "-o", str(tmp_path / "bad.bam"), str(bad)]) == 1
    assert "BAM: read 5 has a name of 255 bytes" in capsys.readouterr().err
