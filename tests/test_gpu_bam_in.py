"""BAM files as read input, records decoded on the device (include/gwa.h "BAM input"; csrc/bam_in.hip; format 2
of csrc/record_stream.cpp behind gwa_pipeline_align_file / _pair_files and `align reads.bam`).

The kernels' correctness test is equality with the host build of the same decoder and with the pure-Python
reference tests/ubam_ref.py, on the cases tests/test_bam_in_host.py runs through that build under
sanitizers.  The pipeline rests on the equivalence rule: aligning a BAM file gives, byte for byte, the output
of aligning ubam_ref.reads_of(its records) handed over in memory, and for files where every record has a
quality also that of the equivalent FASTQ file.  The world is that of tests/test_gpu_inflate.py: a 50 kb
genome, 400 reads of 100 bp and 400 pairs, the BAM cut into BGZF members of 300-4 000 bytes and read in
65 536-byte chunks; a quarter of the records are stored reverse-strand, a few secondary records are
interspersed, and one variant has records without a quality."""
import io
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import synth  # noqa: E402
import ubam_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the decoder ---------------------------------------------------------------------------------------------

def test_device_decode_equals_host_and_reference():
    cases = U.cases()
    for name, data in cases:
        dev = gwa.bam_reads_decode(data, device=0)
        assert dev == U.reads_of(data), name
        assert dev == gwa.bam_reads_decode(data, device=-1), name
    whole = b"".join(c[1] for c in cases)  # one launch, records at every alignment
    assert gwa.bam_reads_decode(whole, device=0) == U.reads_of(whole)
    assert gwa.bam_reads_decode(b"", device=0) == []


def test_malformed_records_fail_as_in_the_host_build():
    """(after the well-formed cases above: tests run in the file's order)"""
    for name, data, msg in U.malformed():
        msgs = []
        for device in (-1, 0):
            with pytest.raises(gwa.GwaError) as e:
                gwa.bam_reads_decode(data, device=device)
            msgs.append(str(e.value))
        assert msgs == [msg, msg], name
    # two bad records in one call: the lowest is reported
    bad = U.record("b", "ACGTACGTACGTACGTACGT", bytes([0] * 19 + [200]))
    good = U.read_record("g", "ACGT", "IIII")
    data = good + bad + good * 300 + U.record(b"x", "AC", "II", nul=False)
    for device in (-1, 0):
        with pytest.raises(gwa.GwaError, match="BAM record 1 at byte %d: quality byte 19 is 200" % len(good)):
            gwa.bam_reads_decode(data, device=device)
    # a well-formed call in the same process afterwards
    assert gwa.bam_reads_decode(good * 3, device=0) == [("g", "ACGT", "IIII")] * 3
    n, ms = gwa.bam_reads_decode_timed(U.random_records(500), device=0, repeat=2)
    assert n == len(U.reads_of(U.random_records(500))) and ms > 0


# ---- the pipeline --------------------------------------------------------------------------------------------

def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _records(reads, rng, flag=4, no_qual=0.0, secondary=True):
    """the reads as records: a quarter stored reverse-strand, secondary records in between"""
    out = []
    for i, (name, seq, qual) in enumerate(reads):
        if secondary and i % 37 == 5:
            out.append(U.read_record("sec%d" % i, seq[:50], None, 0x100 | (flag & ~4)))
        q = None if rng.random() < no_qual else qual
        out.append(U.read_record(name, seq, q, flag | (0x10 if rng.random() < 0.25 else 0),
                                 cigar=[(100 << 4)] * rng.randrange(3), tags=b"RGZgrp\0"[:rng.randrange(8)]))
    return b"".join(out)


class World:
    def __init__(self, d):
        codes, names, lengths = synth.genome([("chr1", 30000), ("chr2", 20000)], 1)
        self.fasta = synth.fasta_text(codes, names, lengths)
        seqs, rn = synth.reads(codes, lengths, 400, 100, 2)
        strs = synth.to_strings(seqs)
        rng = random.Random(4)
        q = lambda: "".join(rng.choice("IHGF@+5") for _ in range(100))  # noqa: E731
        reads = [(rn[i], strs[i], q()) for i in range(400)]
        contigs = ["".join(x.split("\n")[1:]) for x in self.fasta.split(">")[1:]]
        m1, m2 = [], []
        for i in range(400):
            g = contigs[i % 2]
            p = rng.randrange(0, len(g) - 320)
            m1.append(("p%d/1" % i, g[p:p + 100], q()))
            m2.append(("p%d/2" % i, _revcomp(g[p + 200:p + 300]), q()))
        self.reads, self.m1, self.m2 = reads, m1, m2
        self.dir = d
        cs = list(zip(names, [int(x) for x in lengths]))
        text = "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in cs)
        self.recs = {
            "reads": _records(reads, rng),
            "reads_nq": _records(reads, rng, no_qual=0.05),
            "m_1": _records(m1, rng, 0x4D),
            "m_2": _records(m2, rng, 0x8D),
            "inter": b"".join(_records([a], rng, 0x4D, secondary=(i % 50 == 3)) + _records([b], rng, 0x8D, secondary=False)
                              for i, (a, b) in enumerate(zip(m1, m2))),
        }
        for k, (name, r) in enumerate(self.recs.items()):
            (d / (name + ".bam")).write_bytes(U.bam_file(r, text, cs, seed=40 + k, eof=(k != 2)))
        for name, rs in (("reads", reads), ("m_1", m1), ("m_2", m2), ("inter", [x for ab in zip(m1, m2) for x in ab])):
            (d / (name + ".fq")).write_bytes(U.fastq_of(rs))
        (d / "ref.fa").write_text(self.fasta)
        self.fm = gwa.FMIndexOnGenome.buildFromFasta(self.fasta, device=0)

    def path(self, name, ext=".bam"):
        return str(self.dir / (name + ext))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    os.environ["GWA_PIPE_CHUNK"] = "65536"
    w = World(tmp_path_factory.mktemp("bam_in"))
    yield w
    w.fm.close()
    os.environ.pop("GWA_PIPE_CHUNK", None)
    os.environ.pop("GWA_BGZF_INPUT", None)


def _to_file(tmp_path, call, name="out.sam"):
    path = tmp_path / name
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        call(fd)
    finally:
        os.close(fd)
    return path.read_bytes()


def test_world_is_what_the_docstring_says(world):
    for name in ("reads", "reads_nq"):
        assert [r[:2] for r in U.reads_of(world.recs[name])] == [r[:2] for r in world.reads]
    assert U.reads_of(world.recs["reads"]) == world.reads
    assert sum(1 for r in U.reads_of(world.recs["reads_nq"]) if r[2] is None) >= 5
    w = U.walk(world.recs["reads"])
    assert 60 < sum(1 for _, f in w if f & 0x10) < 160 and sum(1 for _, f in w if f & 0x100) >= 8
    assert U.reads_of(world.recs["inter"]) == [x for ab in zip(world.m1, world.m2) for x in ab]


@pytest.mark.parametrize("batch", [64, 1 << 20])
def test_pipeline_aligns_a_bam_file(world, tmp_path, batch):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=batch)
    try:
        fq = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", ".fq"), fd))
        assert fq.count(b"\n") >= 400
        n = []
        bam = _to_file(tmp_path, lambda fd: n.append(pipe.align_file(world.path("reads"), fd)))
        st = pipe.stats()
        assert n == [400] and st.reads == 400 and st.inflate_blocks > 20
        assert bam == fq
        assert bam.decode() == pipe.align_batch(U.reads_of(world.recs["reads"]))
        nq = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads_nq"), fd))
        assert nq.decode() == pipe.align_batch(U.reads_of(world.recs["reads_nq"]))
        assert nq != fq and b"\t*\t" in nq
    finally:
        pipe.close()


def test_pipeline_bam_through_zlib_md_and_bgzf(world, tmp_path):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0, mdTag=True), batch_reads=64)
    try:
        fq = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", ".fq"), fd))
        assert b"MD:Z:" in fq
        os.environ["GWA_BGZF_INPUT"] = "0"
        try:
            z = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads"), fd))
        finally:
            del os.environ["GWA_BGZF_INPUT"]
        assert z == fq and pipe.stats().inflate_blocks == 0
        pipe.set_output("bgzf")
        a = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads"), fd))
        b = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", ".fq"), fd))
        assert a == b and gwa.bgzf_decompress(a, device=0) == fq
    finally:
        pipe.close()


@pytest.mark.parametrize("batch", [64, 1 << 20])
def test_pipeline_aligns_bam_pairs(world, tmp_path, batch):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=batch)
    try:
        fq = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1", ".fq"), world.path("m_2", ".fq"), fd))
        assert fq.count(b"\n") == 800
        assert fq.decode() == pipe.align_pairs(U.reads_of(world.recs["m_1"]), U.reads_of(world.recs["m_2"]))
        two = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1"), world.path("m_2"), fd))
        assert two == fq
        inter = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("inter"), None, fd))
        assert inter == fq
        mixed = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1"), world.path("m_2", ".fq"), fd))
        assert mixed == fq
        mixed = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1", ".fq"), world.path("m_2"), fd))
        assert mixed == fq
        named = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("inter"), None, fd, check_names=True))
        assert named == fq
        named = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1"), world.path("m_2"), fd, check_names=True))
        assert named == fq
    finally:
        pipe.close()


def test_pipeline_refuses_wrong_pairs_and_bad_records(world, tmp_path):
    rng = random.Random(9)
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=64)
    try:
        # pair 150's second record is flagged as a first mate, pair 300's too: the lowest is named
        recs = b"".join(_records([a], rng, 0x4D, secondary=False) + _records([b], rng, 0x4D if i in (150, 300) else 0x8D, secondary=False)
                        for i, (a, b) in enumerate(zip(world.m1, world.m2)))
        (tmp_path / "flags.bam").write_bytes(U.bam_file(recs, seed=3))
        with pytest.raises(gwa.GwaError, match=r"the records of pair 150 carry FLAG (77|93) and (77|93): an interleaved BAM"):
            _to_file(tmp_path, lambda fd: pipe.align_pair_files(str(tmp_path / "flags.bam"), None, fd))
        # an odd count
        (tmp_path / "odd.bam").write_bytes(U.bam_file(_records(world.m1[:33], rng, 0x4D, secondary=False)))
        with pytest.raises(gwa.GwaError, match="odd number of reads"):
            _to_file(tmp_path, lambda fd: pipe.align_pair_files(str(tmp_path / "odd.bam"), None, fd))
        # mate names that differ
        m2 = list(world.m2)
        m2[77] = ("q77/2",) + m2[77][1:]
        (tmp_path / "names.bam").write_bytes(U.bam_file(_records(m2, rng, 0x8D), seed=5))
        with pytest.raises(gwa.GwaError, match="the mate names of pair 77 differ: 'p77/1' and 'q77/2'"):
            _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1"), str(tmp_path / "names.bam"), fd, check_names=True))
        # a record with a bad quality byte, behind secondary records: index and offset of the file's stream
        recs = world.recs["reads"]
        w = U.walk(recs)
        k = [i for i, (_, f) in enumerate(w) if not f & 0x100][250]
        at = w[k][0]
        bad = bytearray(recs)
        lname, ncig = bad[at + 12], int.from_bytes(bad[at + 16:at + 18], "little")
        bad[at + 36 + lname + 4 * ncig + 50 + 7] = 99
        header = len(U.bam_bytes(b""))
        (tmp_path / "qual.bam").write_bytes(U.bam_file(bytes(bad), seed=6))
        with pytest.raises(gwa.GwaError) as e:
            _to_file(tmp_path, lambda fd: pipe.align_file(str(tmp_path / "qual.bam"), fd))
        assert "qual.bam: BAM record %d at byte %d: quality byte 7 is 99" % (k, header + at) in str(e.value)
        # and a well-formed run afterwards
        assert _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads"), fd)).count(b"\n") >= 400
    finally:
        pipe.close()


# ---- the CLI -------------------------------------------------------------------------------------------------

def _cli(world, extra, paths, binary=False):
    import gwa_cli
    out = io.BytesIO() if binary else io.StringIO()
    argv = ["align", "-r", str(world.dir / "ref.fa"), "-k", "2", "--batch", "97"] + extra + paths
    n = gwa_cli.align(gwa_cli.build_parser().parse_args(argv), out=out)
    return n, out.getvalue()


def test_cli_aligns_bam_files(world):
    n, plain = _cli(world, [], [world.path("reads", ".fq")])
    assert n == 400 and plain.startswith("@SQ")
    assert _cli(world, [], [world.path("reads")]) == (400, plain)
    pairs = _cli(world, ["--interleaved"], [world.path("inter", ".fq")])
    assert pairs[0] == 400
    assert _cli(world, ["--interleaved"], [world.path("inter")]) == pairs
    assert _cli(world, [], [world.path("m_1"), world.path("m_2")]) == pairs


def test_cli_sorted_bam_and_index_from_bam_input(world, tmp_path):
    import gwa_cli
    outs = []
    for k, src in enumerate((world.path("reads", ".fq"), world.path("reads"))):
        o = str(tmp_path / ("out%d.bam" % k))
        argv = ["align", "-r", str(world.dir / "ref.fa"), "-k", "2", "--batch", "97", "--bam", "--sort", "--index", "-o", o, src]
        with open(o, "wb") as f:
            assert gwa_cli.align(gwa_cli.build_parser().parse_args(argv), out=f) == 400
        outs.append((open(o, "rb").read(), open(o + ".bai", "rb").read()))
    assert outs[0] == outs[1] and len(outs[0][0]) > 1000 and outs[0][1][:4] == b"BAI\1"
