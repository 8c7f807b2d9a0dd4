"""BGZF read files inflated on the device (include/gwa.h gwa_bgzf_decompress; csrc/inflate.hip; the BGZF
source of csrc/record_stream.cpp behind gwa_pipeline_align_file and `align reads.fastq.gz`).

The kernel's correctness test is equality with the host build of the same decoder -- bytes, and for
malformed members the error with its member index, status code and bit offset -- on the inputs of
tests/inflate_ref.py, which tests/test_inflate_host.py runs through that build under sanitizers.  The
pipeline and the CLI are checked against their own output for the plain file: a 50 kb genome and 400 reads
of 100 bp, the FASTQ cut into BGZF members of 300-4 000 text bytes and read in 65 536-byte chunks."""
import io
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "tools")]

import gwa  # noqa: E402
import inflate_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def test_device_equals_host_on_well_formed_input():
    cases = R.well_formed()
    for name, text, z in cases:
        dev = gwa.bgzf_decompress(z, device=0)
        assert dev == text, name
        assert dev == gwa.bgzf_decompress(z, device=-1), name
    # every member in one call: one kernel launch, texts at all alignments
    z = b"".join(c[2] for c in cases)
    text = b"".join(c[1] for c in cases)
    assert gwa.bgzf_decompress(z, device=0) == text == gwa.bgzf_decompress(z)


def test_device_round_trip_of_the_device_encoder():
    le = R.low_entropy(65536)
    for n in R.LENGTHS:
        assert gwa.bgzf_decompress(gwa.bgzf_compress(le[:n], device=0), device=0) == le[:n], n
    t = R.sam_text(2000)  # several full slices and a short one
    assert gwa.bgzf_decompress(gwa.bgzf_compress(t, device=0) + gwa.BGZF_EOF, device=0) == t


def test_malformed_members_fail_as_in_the_host_build():
    """(after the well-formed cases above: tests run in the file's order)"""
    good = R.member(R.low_entropy(300, seed=6))
    for name, z, code in R.one_per_code():
        data = good + z + good  # the malformed member is member 1
        msgs = []
        for device in (-1, 0):
            with pytest.raises(gwa.GwaError) as e:
                gwa.bgzf_decompress(data, device=device)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], name
        assert "BGZF member 1 at byte %d: " % len(good) in msgs[1] and msgs[1].endswith("(status %d)" % code), (name, msgs[1])
    for name, z, part in R.header_faults():
        with pytest.raises(gwa.GwaError) as e:
            gwa.bgzf_decompress(z, device=0)
        assert part in str(e.value), name
    # a well-formed call on the same process afterwards
    assert gwa.bgzf_decompress(good + gwa.BGZF_EOF, device=0) == R.low_entropy(300, seed=6)


# ---- the pipeline --------------------------------------------------------------------------------------------

def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class World:
    def __init__(self, d):
        codes, names, lengths = synth.genome([("chr1", 30000), ("chr2", 20000)], 1)
        self.fasta = synth.fasta_text(codes, names, lengths)
        seqs, rn = synth.reads(codes, lengths, 400, 100, 2)
        strs = synth.to_strings(seqs)
        rng = random.Random(4)
        q = lambda: "".join(rng.choice("IHGF@+5") for _ in range(100))  # noqa: E731
        self.fq = "".join("@%s\n%s\n+\n%s\n" % (rn[i], strs[i], q()) for i in range(400)).encode()
        contigs = ["".join(x.split("\n")[1:]) for x in self.fasta.split(">")[1:]]
        m1, m2 = [], []
        for i in range(400):
            g = contigs[i % 2]
            p = rng.randrange(0, len(g) - 320)
            m1.append("@p%d/1\n%s\n+\n%s\n" % (i, g[p:p + 100], q()))
            m2.append("@p%d/2\n%s\n+\n%s\n" % (i, _revcomp(g[p + 200:p + 300]), q()))
        self.files = {"reads": self.fq, "m_1": "".join(m1).encode(), "m_2": "".join(m2).encode(),
                      "inter": "".join(a + b for a, b in zip(m1, m2)).encode()}
        self.dir = d
        for k, (name, t) in enumerate(self.files.items()):
            (d / (name + ".fq")).write_bytes(t)
            (d / (name + ".fq.gz")).write_bytes(R.cut_members(t, seed=20 + k, eof=(k != 2)))
        (d / "ref.fa").write_text(self.fasta)
        self.fm = gwa.FMIndexOnGenome.buildFromFasta(self.fasta, device=0)

    def path(self, name, z=False):
        return str(self.dir / (name + (".fq.gz" if z else ".fq")))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    os.environ["GWA_PIPE_CHUNK"] = "65536"
    w = World(tmp_path_factory.mktemp("inflate"))
    yield w
    w.fm.close()
    os.environ.pop("GWA_PIPE_CHUNK", None)
    os.environ.pop("GWA_BGZF_INPUT", None)


def _to_file(tmp_path, call):
    path = tmp_path / "out.sam"
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        call(fd)
    finally:
        os.close(fd)
    return path.read_bytes()


@pytest.mark.parametrize("workers", [1, 3])
def test_pipeline_reads_a_bgzf_file(world, tmp_path, workers):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=97, workers_per_device=workers)
    try:
        plain = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads"), fd))
        st = pipe.stats()
        assert plain.count(b"\n") >= 400 and (st.inflate_blocks, st.in_bytes, st.inflate_s) == (0, 0, 0.0)
        z = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", True), fd))
        st = pipe.stats()
        assert z == plain
        assert st.inflate_blocks > 20 and st.in_bytes == os.path.getsize(world.path("reads", True))
        assert 0 < st.inflate_s <= st.read_s
        os.environ["GWA_BGZF_INPUT"] = "0"
        try:
            z = _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", True), fd))
        finally:
            del os.environ["GWA_BGZF_INPUT"]
        assert z == plain and pipe.stats().inflate_blocks == 0
    finally:
        pipe.close()


def test_pipeline_reads_bgzf_pair_files(world, tmp_path):
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=97)
    try:
        plain = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1"), world.path("m_2"), fd))
        assert plain.count(b"\n") == 800
        z = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("m_1", True), world.path("m_2", True), fd))
        assert z == plain and pipe.stats().inflate_blocks > 40
        assert _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("inter"), None, fd)) == plain
        z = _to_file(tmp_path, lambda fd: pipe.align_pair_files(world.path("inter", True), None, fd))
        assert z == plain and pipe.stats().inflate_blocks > 40
    finally:
        pipe.close()


def test_pipeline_reports_a_bad_member_of_the_file(world, tmp_path):
    z = bytearray(R.cut_members(world.fq, seed=31))
    ms = R.bgzf_ref.members(bytes(z))
    at = sum(len(p) + 26 for p, _, _ in ms[:5])
    z[at + 18 + len(ms[5][0])] ^= 1  # the CRC32 of member 5
    bad = tmp_path / "bad.fq.gz"
    bad.write_bytes(bytes(z))
    pipe = gwa.Pipeline([world.fm], gwa.AlignmentConfig(k=2.0), batch_reads=97)
    try:
        with pytest.raises(gwa.GwaError) as e:
            _to_file(tmp_path, lambda fd: pipe.align_file(str(bad), fd))
        assert "BGZF member 5 at byte %d: CRC32 mismatch" % at in str(e.value)
        assert _to_file(tmp_path, lambda fd: pipe.align_file(world.path("reads", True), fd)).count(b"\n") >= 400
    finally:
        pipe.close()


def test_cli_reads_bgzf_and_its_own_bgzf_output_decodes(world):
    import gwa_cli

    def run(extra, path, binary=False):
        out = io.BytesIO() if binary else io.StringIO()
        argv = ["align", "-r", str(world.dir / "ref.fa"), "-k", "2", "--batch", "97"] + extra + [path]
        n = gwa_cli.align(gwa_cli.build_parser().parse_args(argv), out=out)
        return n, out.getvalue()

    n, plain = run([], world.path("reads"))
    assert n == 400 and plain.startswith("@SQ")
    assert run([], world.path("reads", True)) == (400, plain)
    n, z = run(["--bgzf"], world.path("reads", True), binary=True)
    assert n == 400 and gwa.bgzf_decompress(z, device=0).decode() == plain
