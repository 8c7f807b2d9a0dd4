"""BGZF output compressed on the device (include/gwa.h gwa_bgzf_compress, gwa_batch_results_bgzf,
gwa_pipeline_set_output; gwa_cli align --bgzf).

The kernel's correctness test is byte equality with the host build of the same encoder on every input of
tests/test_bgzf_host.py (which checks that build against the contract with zlib).  Batches, pipeline runs
and the CLI are checked against the contract (tests/bgzf_ref.py) and against their own plain SAM output.
The world is the small one of tests/test_gpu_md.py (its generators, imported): a 9.5 kb genome, reads of
40-129 bp, 240 pairs."""
import ctypes
import gzip
import io
import math
import os
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import bgzf_ref  # noqa: E402
import test_bgzf_host as H  # noqa: E402
import test_gpu_md as M  # noqa: E402

pytestmark = pytest.mark.gpu

SLICE = bgzf_ref.SLICE
LENS = (40, 64, 100, 129)


def test_device_equals_host():
    inputs = dict(H.INPUTS())
    inputs["empty"] = b""
    inputs["sam_skewed"] = H.sam_lines(900, False)   # 3 full slices and a short one
    inputs["sam_constant"] = H.sam_lines(300, True)
    for name, data in inputs.items():
        dev = gwa.bgzf_compress(data, device=0)
        assert dev == gwa.bgzf_compress(data), name
    assert gwa.bgzf_compress(b"", device=0) == b""
    buf = ctypes.create_string_buffer(28)
    assert gwa.lib().gwa_bgzf_eof(buf) == 0 and buf.raw == gwa.BGZF_EOF == bgzf_ref.EOF


class World:
    def __init__(self):
        self.seqs = M.make_genome()
        self.fasta = "".join(">%s\n%s\n" % (n, s) for (n, _), s in zip(M.LENGTHS, self.seqs))
        self.reads = M.make_reads(self.seqs, M.N_READS, lens=LENS)
        self.many = M.make_reads(self.seqs, 800, lens=LENS, seed=M.SEED + 5)  # ~150 KB of SAM: three blocks
        self.m1, self.m2 = M.make_pairs(self.seqs, M.N_PAIRS)
        self.fm = gwa.FMIndexOnGenome.buildFromFasta(self.fasta, device=0)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.fm.close()


def blobs(reads):
    names, seqs, quals = zip(*reads)
    nb, no = gwa._pack(names)
    sb, so = gwa._pack(seqs)
    qb, qo = gwa._pack(quals)
    return nb, no, sb, so, qb, qo


BATCHES = {
    "bsf_k2_three_blocks": (dict(k=2.0), "many"),
    "sf_k5": (dict(k=5.0, strategy="sf"), "reads"),
    "bsf_k5_allhits": (dict(k=5.0, reportType="allhits"), "reads"),
    "bsf_k2_md": (dict(k=2.0, mdTag=True), "reads"),
    "pairs": (dict(k=2.0), None),
    "bd_header_only": (dict(k=2.0, strategy="bd"), "reads"),
}


@pytest.mark.parametrize("case", list(BATCHES))
def test_batch_results_bgzf(world, case):
    opts, which = BATCHES[case]
    cfg = gwa.AlignmentConfig(**opts)
    if which is None:
        b = gwa.Batch(world.fm, cfg, pair_blobs=(blobs(world.m1), blobs(world.m2)))
    else:
        b = gwa.Batch(world.fm, cfg, reads=getattr(world, which))
    try:
        b.run()
        sam = b.results()[0].encode()
        z = b.results_bgzf()
        assert b"".join(bgzf_ref.blocks(z)) == sam
        st = b.stats()
        nb = math.ceil(len(sam) / SLICE)
        assert (st.bgzf_blocks, st.bgzf_bytes) == (nb, len(z)) and st.bgzf_stored == 0
        assert b.format_bgzf() == len(z)
        assert b.stats().bgzf_blocks == nb
        assert b.results_bgzf() == z  # the same text gives the same bytes
        if case == "bsf_k2_three_blocks":
            assert nb >= 3 and len(z) < len(sam)
        if case == "bd_header_only":
            assert sam == b"" and z == b""
        if case == "bsf_k2_md":
            assert b"MD:Z:" in sam
        # the plain text is still there for gwa_batch_sam_copy after a BGZF formatting
        if sam:
            assert bytes(b.sam_device().cpu().numpy().tobytes()) == sam
    finally:
        b.close()


def write_fastq(path, reads):
    path.write_text("".join("@%s\n%s\n+\n%s\n" % r for r in reads))


def run_to(kind, tmp_path, call):
    """call(fd) writes to a regular file, an O_APPEND descriptor or a pipe; the bytes written"""
    if kind == "pipe":
        r, w = os.pipe()
        got = []
        t = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
        t.start()
        try:
            call(w)
        finally:
            os.close(w)
            t.join()
        return got[0]
    path = tmp_path / ("out_%s" % kind)
    if path.exists():
        path.unlink()
    flags = os.O_WRONLY | os.O_CREAT | (os.O_APPEND if kind == "append" else 0)
    fd = os.open(str(path), flags, 0o644)
    try:
        call(fd)
    finally:
        os.close(fd)
    return path.read_bytes()


def test_pipeline_bgzf_output(world, tmp_path):
    cfg = gwa.AlignmentConfig(k=2.0)
    fq = tmp_path / "reads.fq"
    write_fastq(fq, world.reads)
    f1, f2 = tmp_path / "m_1.fq", tmp_path / "m_2.fq"
    write_fastq(f1, world.m1)
    write_fastq(f2, world.m2)
    plain = plain_pairs = None
    for batch_reads, kinds in ((97, ("file", "append", "pipe")), (600, ("file",))):
        pipe = gwa.Pipeline([world.fm], cfg, batch_reads=batch_reads)
        try:
            if plain is None:
                plain = run_to("file", tmp_path, lambda fd: pipe.align_file(str(fq), fd))
                plain_pairs = run_to("file", tmp_path, lambda fd: pipe.align_pair_files(str(f1), str(f2), fd))
                assert plain.count(b"\n") >= len(world.reads) and plain_pairs.count(b"\n") == 2 * M.N_PAIRS
            pipe.set_output("bgzf")
            for kind in kinds:
                z = run_to(kind, tmp_path, lambda fd: pipe.align_file(str(fq), fd))
                assert gzip.decompress(z) == plain, (batch_reads, kind)
                slices = bgzf_ref.blocks(z, runs=True)
                assert len(slices) >= math.ceil(len(world.reads) / batch_reads)
                assert pipe.stats().out_bytes == len(z) < len(plain)
            z = run_to("file", tmp_path, lambda fd: pipe.align_pair_files(str(f1), str(f2), fd))
            assert gzip.decompress(z) == plain_pairs
            bgzf_ref.blocks(z, runs=True)
            assert "\t" in pipe.align_batch(world.reads[:20])  # (the in-memory calls return text either way)
            pipe.set_output("sam")
            assert run_to("file", tmp_path, lambda fd: pipe.align_file(str(fq), fd)) == plain
            assert pipe.stats().out_bytes == len(plain)
        finally:
            pipe.close()
    p2 = gwa.Pipeline([world.fm], cfg, batch_reads=97, output="bgzf")
    try:
        assert gzip.decompress(run_to("file", tmp_path, lambda fd: p2.align_file(str(fq), fd))) == plain
    finally:
        p2.close()


def test_unknown_output_format_is_rejected(world):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=97)
    try:
        L = gwa.lib()
        assert L.gwa_pipeline_set_output(pipe.h, 7) != 0
        assert L.gwa_last_error().decode().startswith("gwa_pipeline_set_output: unknown format 7")
        with pytest.raises(gwa.GwaError):
            pipe.set_output("bam")
    finally:
        pipe.close()


def test_cli_bgzf(tmp_path):
    """gwa_cli align --bgzf over tests/golden/fixtures/reads_c1.fq.snap: header, records, EOF marker; zcat of
    it is the plain run; two shards concatenated are one file with one EOF marker; -m bd is header + EOF"""
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
    write_fastq(fq, reads)

    def run(extra, path, binary=True):
        out = io.BytesIO() if binary else io.StringIO()
        argv = ["align", "-r", str(ref), "-k", "2", "--batch", "64"] + extra + [path]
        n = gwa_cli.align(gwa_cli.build_parser().parse_args(argv), out=out)
        return n, out.getvalue()

    n, plain = run([], snap, binary=False)
    assert n == len(reads) and plain.startswith("@SQ")
    n, z = run(["--bgzf"], snap)
    assert n == len(reads) and z.endswith(gwa.BGZF_EOF) and z.count(gwa.BGZF_EOF) == 1
    assert gzip.decompress(z).decode() == plain
    body = z[:-28]
    slices = bgzf_ref.blocks(body, runs=True)
    assert slices[0].startswith(b"@SQ") and len(slices) >= 1 + math.ceil(len(reads) / 64)
    # shards of the plain file
    parts = [run(["--bgzf", "--shard", "%d/2" % r], str(fq)) for r in (0, 1)]
    assert parts[0][0] + parts[1][0] == len(reads)
    cat = parts[0][1] + parts[1][1]
    assert cat.count(gwa.BGZF_EOF) == 1 and cat.endswith(gwa.BGZF_EOF) and not parts[0][1].endswith(gwa.BGZF_EOF)
    assert gzip.decompress(cat).decode() == plain
    # -m bd: the reference prints the header only
    n, z = run(["--bgzf", "-m", "bd"], snap)
    assert z.endswith(gwa.BGZF_EOF)
    assert gzip.decompress(z).decode() == "".join(l + "\n" for l in plain.splitlines() if l.startswith("@"))
    # -q: one query, no read file
    out = io.BytesIO()
    q = reads[0][1]
    ns = gwa_cli.build_parser().parse_args(["align", "-r", str(ref), "-k", "2", "--bgzf", "-q", q])
    assert gwa_cli.align(ns, out=out) == 1
    text = gzip.decompress(out.getvalue()).decode()
    assert text.startswith("@SQ") and text.splitlines()[-1].startswith("read\t") and out.getvalue().endswith(gwa.BGZF_EOF)
