"""Paired-end read files through the multi-device streaming pipeline (include/gwa.h
gwa_pipeline_align_pair_files / gwa_pipeline_align_pairs, gwa_cli align with two read files or
--interleaved), compared byte for byte with the oracle's Index.align_pairs: 100 bp mates from
synth.pairs_codes on a 100 kb two-contig synth.genome, every pair in every comparison.  The shapes are
the smallest at which the new code can go wrong: batch sizes that cut the chunks of two files with
different bytes per record (GWA_PIPE_CHUNK=4096, the carry paths), mate-1 texts of every length
mod 16 without a final newline (the second text segment's bounds and alignment), mixed containers,
interleaved input, unequal files, the mate-name check over more than two workgroups."""
import gzip
import io
import os
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tools"),
                os.path.join(HERE, "golden")]

import gwa  # noqa: E402
import gwa_cli  # noqa: E402

pytestmark = pytest.mark.gpu

NP = 600
K = 2.0


class _World:
    """one genome, its oracle index, two device handles on GPU 0 and the pairs, built once"""

    def __init__(self):
        import oracle as O
        import synth
        self.O = O
        self.codes, self.names, self.lengths = synth.genome([("chrA", 60000), ("chr2", 41000)], config_id=9)
        self.fasta = synth.fasta_text(self.codes, self.names, self.lengths)
        m1, m2 = synth.pairs_codes(self.codes, self.lengths, NP, config_id=16)
        self.s1, self.s2 = synth.to_strings(m1), synth.to_strings(m2)
        self.oi = O.Index.from_arrays(self.codes, self.names, self.lengths)
        self.fms = [gwa.FMIndexOnGenome.buildFromCodes(self.codes, self.names, self.lengths, device=0) for _ in range(2)]
        self._sam = {}

    def oracle(self, r1, r2, insert=(210, 390)):
        key = (tuple(r1), tuple(r2), insert)
        if key not in self._sam:
            self._sam[key] = self.oi.align_pairs(r1, r2, self.O.OrcConfig.default(k=K), insert[0], insert[1])
        return self._sam[key]

    def mates(self, n=NP, name1="q%d", name2="q%d", qual=True):
        q = "I" * 100 if qual else None
        return ([(name1 % i, self.s1[i], q) for i in range(n)], [(name2 % i, self.s2[i], q) for i in range(n)])

    def pipeline(self, batch, handles=1, workers=0):
        return gwa.Pipeline(self.fms[:handles], gwa.AlignmentConfig(k=K), batch_reads=batch, workers_per_device=workers)

    def close(self):
        for fm in self.fms:
            fm.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def fastq(recs):
    return "".join("@%s\n%s\n+\n%s\n" % r for r in recs).encode()


def fasta(recs):
    return "".join(">%s\n%s\n%s\n" % (r[0], r[1][:60], r[1][60:]) for r in recs).encode()


def run_files(pipe, tmp_path, p1, p2, **kw):
    out = tmp_path / "out.sam"
    with open(out, "wb") as f:
        n = pipe.align_pair_files(str(p1), None if p2 is None else str(p2), f.fileno(), **kw)
    return n, out.read_text()


# 1 ---- two plain FASTQ files, many chunks, every batch size ----

LONG1, SHORT2 = "m1_" + "x" * 31 + "%06d", "%02d"  # 40-B mate-1 names; 2-B mate-2 names (3 B from pair 100 on)


@pytest.mark.parametrize("handles,workers", [(1, 0), (2, 4)])
@pytest.mark.parametrize("batch", [1, 7, 61, 500])
def test_two_fastq_files_match_the_oracle(world, tmp_path, monkeypatch, batch, handles, workers):
    # the files' 4096-B chunks hold different record counts (254 against 213 B per record), and a batch
    # of 500 records (over 100 kB) outgrows the 8 kB of room before a chunk: the big-carry branch
    monkeypatch.setenv("GWA_PIPE_CHUNK", "4096")
    r1, r2 = world.mates(name1=LONG1, name2=SHORT2)
    assert len(r1[0][0]) == 40 and len(r2[0][0]) == 2
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "r_2.fq").write_bytes(fastq(r2))
    pipe = world.pipeline(batch, handles, workers)
    try:
        n, sam = run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / "r_2.fq")
        st = pipe.stats()
    finally:
        pipe.close()
    assert n == NP and st.reads == 2 * NP and st.batches == (NP + batch - 1) // batch
    assert sam == world.oracle(r1, r2)


# 2 ---- segment bounds and alignment ----

def _py_records(text):
    return list(gwa_cli.read_fastq(io.StringIO(text.decode(), newline=None)))


def test_second_segment_bounds_and_alignment(world, tmp_path):
    # 33 pairs of mixed read and name lengths; mate 1's text has no final newline, CRLF on every third
    # record, blank lines between some records and one empty read.  16 variants pad the first header's
    # description so that the mate-1 text length takes every residue mod 16: mate 2's text then starts
    # at every distance behind it, and a last line bounded by the whole buffer instead of its own
    # segment would run on into the padding or into mate 2's first header.
    lens, nlens = [1, 15, 16, 17, 33, 100], [1, 15, 16, 17, 40]
    alpha = "abcdefghijklmnopqrstuvwxyzABCDEFG"

    def mate(i, seqs, shift):
        m = lens[(i + shift) % 6]
        if i == 20 and shift == 0:
            m = 0  # the empty read
        return ((alpha[i] * nlens[(i + shift) % 5]), seqs[i][:m], "I" * m)

    r1 = [mate(i, world.s1, 0) for i in range(33)]
    r2 = [mate(i, world.s2, 2) for i in range(33)]
    exp = world.oracle(r1, r2)
    t2 = fastq(r2)
    seen = set()
    pipe = world.pipeline(10)
    try:
        for v in range(16):
            parts = []
            for i, (nm, sq, ql) in enumerate(r1):
                eol = "\r\n" if i % 3 == 1 else "\n"
                hdr = "@" + nm + (" " + "d" * v if i == 0 else "")
                parts.append(hdr + eol + sq + eol + "+" + eol + ql + eol)
                if i % 5 == 4:
                    parts.append("\n")
            t1 = "".join(parts).encode()
            assert t1.endswith(b"I\n")
            t1 = t1[:-1]  # no final newline
            seen.add(len(t1) % 16)
            assert _py_records(t1) == r1 and _py_records(t2) == r2
            (tmp_path / "v_1.fq").write_bytes(t1)
            (tmp_path / "v_2.fq").write_bytes(t2)
            n, sam = run_files(pipe, tmp_path, tmp_path / "v_1.fq", tmp_path / "v_2.fq")
            assert n == 33
            assert sam == exp, v
    finally:
        pipe.close()
    assert seen == set(range(16))


# 3 ---- mixed containers, FASTA mates ----

def test_mixed_containers_and_fasta_mates(world, tmp_path, monkeypatch):
    import make_snap
    monkeypatch.setenv("GWA_PIPE_CHUNK", "4096")
    r1, r2 = world.mates()
    with gzip.open(tmp_path / "r_1.fq.gz", "wb") as f:
        f.write(fastq(r1))
    (tmp_path / "r_2.fq.snap").write_bytes(make_snap.stream(fastq(r2), chunk=8192))
    a1, a2 = world.mates(qual=False)
    (tmp_path / "a_1.fa").write_bytes(fasta(a1))
    (tmp_path / "a_2.fasta").write_bytes(fasta(a2))
    pipe = world.pipeline(97, 2, 2)
    try:
        n, sam = run_files(pipe, tmp_path, tmp_path / "r_1.fq.gz", tmp_path / "r_2.fq.snap")
        assert n == NP and sam == world.oracle(r1, r2)
        n, sam = run_files(pipe, tmp_path, tmp_path / "a_1.fa", tmp_path / "a_2.fasta")  # QUAL "*"
        assert n == NP and sam == world.oracle(a1, a2)
        n, sam = run_files(pipe, tmp_path, tmp_path / "r_1.fq.gz", tmp_path / "a_2.fasta")
        assert n == NP and sam == world.oracle(r1, a2)
        n, sam = run_files(pipe, tmp_path, tmp_path / "a_1.fa", tmp_path / "r_2.fq.snap")
        assert n == NP and sam == world.oracle(a1, r2)
    finally:
        pipe.close()


# 4 ---- interleaved ----

def test_interleaved_file_equals_the_two_file_run(world, tmp_path, monkeypatch):
    monkeypatch.setenv("GWA_PIPE_CHUNK", "4096")
    r1, r2 = world.mates(name1=LONG1, name2=SHORT2)
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "r_2.fq").write_bytes(fastq(r2))
    inter = [r for pair in zip(r1, r2) for r in pair]
    (tmp_path / "i.fq").write_bytes(fastq(inter))
    (tmp_path / "odd.fq").write_bytes(fastq(inter[:-1]))
    a1, a2 = world.mates(qual=False)
    (tmp_path / "i.fa").write_bytes(fasta([r for pair in zip(a1, a2) for r in pair]))
    pipe = world.pipeline(61, 2, 2)
    try:
        n2, two = run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / "r_2.fq")
        n1, one = run_files(pipe, tmp_path, tmp_path / "i.fq", None)
        assert n1 == n2 == NP and pipe.stats().reads == 2 * NP
        assert one == two == world.oracle(r1, r2)
        n, sam = run_files(pipe, tmp_path, tmp_path / "i.fa", None)
        assert n == NP and sam == world.oracle(a1, a2)
        with pytest.raises(gwa.GwaError, match="odd number of reads"):  # 1199 records
            run_files(pipe, tmp_path, tmp_path / "odd.fq", None)
    finally:
        pipe.close()


# 5 ---- mate files of different lengths ----

def test_unequal_mate_files_fail(world, tmp_path, monkeypatch):
    # the missing / extra record is the last of 600: far behind the first 4096-B chunk
    monkeypatch.setenv("GWA_PIPE_CHUNK", "4096")
    r1, r2 = world.mates()
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "short_2.fq").write_bytes(fastq(r2[:-1]))
    (tmp_path / "long_2.fq").write_bytes(fastq(r2 + [("extra", world.s2[0], "I" * 100)]))
    for batch in (61, 100, 600):  # (100 and 600 divide the count: the longer file ends a slice later)
        pipe = world.pipeline(batch, 2, 2)
        try:
            for other in ("short_2.fq", "long_2.fq"):
                with pytest.raises(gwa.GwaError, match="the mate files hold different numbers of reads"):
                    run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / other)
                with pytest.raises(gwa.GwaError, match="the mate files hold different numbers of reads"):
                    run_files(pipe, tmp_path, tmp_path / other, tmp_path / "r_1.fq")
        finally:
            pipe.close()


def test_malformed_record_names_its_file(world, tmp_path):
    r1, r2 = world.mates(8)
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "bad_2.fq").write_bytes(fastq(r2[:5]) + b"@b\nACGT\n+\nIII\n" + fastq(r2[6:]))
    (tmp_path / "bad_2.fa").write_bytes(fasta(r2))
    pipe = world.pipeline(3)
    try:
        with pytest.raises(gwa.GwaError, match=r"bad_2\.fq: malformed FASTQ record"):
            run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / "bad_2.fq")
        with pytest.raises(gwa.GwaError, match=r"bad_2\.fq: malformed FASTQ record"):
            run_files(pipe, tmp_path, tmp_path / "bad_2.fq", tmp_path / "r_1.fq")
        with pytest.raises(gwa.GwaError, match=r"bad_2\.fq: malformed FASTQ record"):  # the host-parsed path
            run_files(pipe, tmp_path, tmp_path / "bad_2.fa", tmp_path / "bad_2.fq")
    finally:
        pipe.close()


def test_sf_and_bad_insert_range_are_refused(world, tmp_path):
    r1, r2 = world.mates(4)
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "r_2.fq").write_bytes(fastq(r2))
    pipe = gwa.Pipeline(world.fms[:1], gwa.AlignmentConfig(k=K, strategy="sf"), batch_reads=2)
    try:
        with pytest.raises(gwa.GwaError, match="-m bsf"):
            run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / "r_2.fq")
        with pytest.raises(gwa.GwaError, match="-m bsf"):
            pipe.align_pairs(r1, r2)
    finally:
        pipe.close()
    pipe = world.pipeline(2)
    try:
        for ins in ((-1, 300), (400, 300)):
            with pytest.raises(gwa.GwaError, match="bad insert-size range"):
                run_files(pipe, tmp_path, tmp_path / "r_1.fq", tmp_path / "r_2.fq", insert=ins)
            with pytest.raises(gwa.GwaError, match="bad insert-size range"):
                pipe.align_pairs(r1, r2, insert=ins)
    finally:
        pipe.close()


# 6 ---- the mate-name check ----

def test_mate_name_check(world, tmp_path):
    n = 520  # more than two workgroups of 256 pairs
    r1, r2 = world.mates(n, name1="q%d/1", name2="q%d/2")
    r1[5], r2[5] = ("/1",) + r1[5][1:], ("/2",) + r2[5][1:]          # a name that is just the suffix
    r1[6], r2[6] = ("same",) + r1[6][1:], ("same",) + r2[6][1:]      # no suffix at all
    r1[7], r2[7] = ("p7/2",) + r1[7][1:], ("p7/1",) + r2[7][1:]      # either digit on either mate
    exp = world.oracle(r1, r2)

    def write(m1, m2):
        (tmp_path / "n_1.fq").write_bytes(fastq(m1))
        (tmp_path / "n_2.fq").write_bytes(fastq(m2))

    def edited(recs, changes):
        out = list(recs)
        for i, name in changes.items():
            out[i] = (name,) + out[i][1:]
        return out

    pipe = world.pipeline(100, 2, 3)  # pairs 3 and 300 fall into different batches, on different workers
    try:
        write(r1, r2)
        got = run_files(pipe, tmp_path, tmp_path / "n_1.fq", tmp_path / "n_2.fq", check_names=True)
        assert got == (n, exp)  # (QNAME keeps the suffixes)
        cases = [({300: "zz300/2", 3: "zz3/2"}, 3, "q3/1", "zz3/2"),
                 ({519: "q51x/2"}, 519, "q519/1", "q51x/2"),       # the last byte only, in the last workgroup
                 ({257: "q2570/2"}, 257, "q257/1", "q2570/2"),     # the length only
                 ({257: "q25/2"}, 257, "q257/1", "q25/2"),
                 ({5: "/"}, 5, "/1", "/"),                         # ("/" has no suffix to remove)
                 ({6: "same/3"}, 6, "same", "same/3"),             # (only /1 and /2 are suffixes)
                 ({7: "p7/1/1"}, 7, "p7/2", "p7/1/1")]             # (one suffix is removed, not two)
        for changes, pair, n1, n2 in cases:
            m2 = edited(r2, changes)
            write(r1, m2)
            with pytest.raises(gwa.GwaError) as e:
                run_files(pipe, tmp_path, tmp_path / "n_1.fq", tmp_path / "n_2.fq", check_names=True)
            msg = str(e.value)
            assert "pair %d " % pair in msg and "'%s'" % n1 in msg and "'%s'" % n2 in msg, (changes, msg)
            # without the flag the same files align
            got = run_files(pipe, tmp_path, tmp_path / "n_1.fq", tmp_path / "n_2.fq")
            assert got == (n, world.oracle(r1, m2))
        # the check reads host-parsed (FASTA) batches as well
        a1, a2 = [(r[0], r[1], None) for r in r1], [(r[0], r[1], None) for r in edited(r2, {300: "zz/2", 3: "zz3/2"})]
        (tmp_path / "n_1.fa").write_bytes(fasta(a1))
        (tmp_path / "n_2.fa").write_bytes(fasta(a2))
        with pytest.raises(gwa.GwaError, match="pair 3 "):
            run_files(pipe, tmp_path, tmp_path / "n_1.fa", tmp_path / "n_2.fa", check_names=True)
    finally:
        pipe.close()


# 7 ---- O_APPEND and pipe output ----

def test_pairs_append_in_pair_order(world, tmp_path):
    r1, r2 = world.mates()
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "r_2.fq").write_bytes(fastq(r2))
    exp = world.oracle(r1, r2)
    out = tmp_path / "out.sam"
    out.write_bytes(b"@HD\tVN:1.0\n")
    pipe = world.pipeline(61, 2, 4)
    try:
        for _ in range(2):  # the second run appends after the first run's records
            with open(out, "ab") as f:
                assert pipe.align_pair_files(str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq"), f.fileno()) == NP
        assert out.read_text() == "@HD\tVN:1.0\n" + exp + exp
        rd, wr = os.pipe()
        got = []
        t = threading.Thread(target=lambda: got.append(os.fdopen(rd, "rb").read()))
        t.start()
        try:
            assert pipe.align_pair_files(str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq"), wr) == NP
        finally:
            os.close(wr)
            t.join()
        assert got[0].decode() == exp
    finally:
        pipe.close()


# 8 ---- in memory ----

def test_in_memory_pairs_over_two_handles(world):
    r1, r2 = world.mates()
    one = gwa.PairedEndAligner(world.fms[0], gwa.AlignmentConfig(k=K)).align_pairs(r1, r2)
    pipe = world.pipeline(97, 2, 3)
    try:
        assert pipe.align_pairs(r1, r2) == one == world.oracle(r1, r2)
        assert pipe.stats().reads == 2 * NP and pipe.stats().batches == 7
        narrow = gwa.PairedEndAligner(world.fms[0], gwa.AlignmentConfig(k=K), 295, 305).align_pairs(r1, r2)
        assert pipe.align_pairs(r1, r2, insert=(295, 305)) == narrow != one
        with pytest.raises(gwa.GwaError, match="different numbers of reads"):
            pipe.align_pairs(r1, r2[:-1])
    finally:
        pipe.close()


# 9 ---- the command line ----

def test_cli_pairs_go_through_the_pipeline(world, tmp_path):
    ref = tmp_path / "ref.fa"
    ref.write_text(world.fasta)
    r1, r2 = world.mates()
    (tmp_path / "r_1.fq").write_bytes(fastq(r1))
    (tmp_path / "r_2.fq").write_bytes(fastq(r2))
    (tmp_path / "i.fq").write_bytes(fastq([r for pair in zip(r1, r2) for r in pair]))
    exp = world.oi.sam_header() + world.oracle(r1, r2)
    base = ["align", "-r", str(ref), "-k", "2"]
    two = [str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")]

    def cli(args):
        out = io.StringIO()
        n = gwa_cli.align(gwa_cli.build_parser().parse_args(base + args), out=out)
        return n, out.getvalue()

    assert cli(["--devices", "0,0", "--batch", "97", "--workers", "2", "--check-mate-names"] + two) == (NP, exp)
    assert cli(["--interleaved", "--batch", "97", str(tmp_path / "i.fq")]) == (NP, exp)
    with open(tmp_path / "cli.sam", "w") as f:  # a real descriptor, --timing on
        ns = gwa_cli.build_parser().parse_args(base + ["--timing", "--batch", "250"] + two)
        assert gwa_cli.align(ns, out=f) == NP
    assert (tmp_path / "cli.sam").read_text() == exp
    assert cli(["--silent"] + two) == (NP, "")
    for bad in (["-m", "sf"] + two, ["--shard", "0/2"] + two, ["--shard", "0/2", "--interleaved", two[0]],
                ["--interleaved"] + two, ["--check-mate-names", two[0]]):
        with pytest.raises(gwa.GwaError):
            cli(bad)


def test_cli_failed_sync_wait_keeps_its_error(world, tmp_path):
    # a failing warm pass or sync wait used to end in the finally's unbound `mono0` (an UnboundLocalError
    # that hid the error and skipped pipe.close()); the error itself must come out
    ref = tmp_path / "ref.fa"
    ref.write_text(world.fasta)
    r1, _ = world.mates(4)
    (tmp_path / "r.fq").write_bytes(fastq(r1))
    ns = gwa_cli.build_parser().parse_args(["align", "-r", str(ref), "-k", "2", "--timing", "--sync",
                                            str(tmp_path / "no_such_dir") + ":2", str(tmp_path / "r.fq")])
    with pytest.raises(FileNotFoundError):
        gwa_cli.align(ns, out=io.StringIO())
