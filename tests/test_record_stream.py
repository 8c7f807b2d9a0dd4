"""The pipeline's HIP-free reader (genome-weaver-align_amd/csrc/record_stream.cpp) on the CPU: a
stand-alone program (tests/record_stream_zip.cpp) built here with the address and undefined-behaviour
sanitizers from record_stream.cpp, reads_io.cpp and snappy_stream.cpp zips two mate files -- or splits
an interleaved one -- into pair batches at chunk sizes from 64 B upward and batch sizes 1 / 7 / 500;
its slices are checked against this file's own split of the same texts, as are the errors for mate
files of different lengths and an odd interleaved file, and the carry paths with records larger than
a chunk (every chunk then carries; at 64-B chunks the carry outgrows the 128 B of room before a chunk,
the `carryLen > reserve` branch).  No sanitizer report may appear."""
import gzip
import io
import os
import random
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "genome-weaver-align_amd", "csrc")
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(HERE, "golden")]

import gwa_cli  # noqa: E402
import make_snap  # noqa: E402

CHUNKS = (64, 100, 257, 4096, 1 << 20)
BATCHES = (1, 7, 500)
N = 53


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the record-stream program"
    out = str(tmp_path_factory.mktemp("rs") / "record_stream_zip")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", os.path.join(HERE, "record_stream_zip.cpp"),
           os.path.join(CSRC, "record_stream.cpp"), os.path.join(CSRC, "reads_io.cpp"),
           os.path.join(CSRC, "snappy_stream.cpp"), "-lz", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


def _run(prog, chunk, batch, p1, p2=None):
    """-> (batches, error): batches = [(pairs, text1, starts1, text2, starts2)]"""
    cmd = [prog, str(chunk), str(batch), str(p1)] + ([str(p2)] if p2 is not None else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]
    out, err = [], None
    for line in r.stdout.splitlines():
        if line.startswith("E "):
            err = line[2:]
            continue
        f = line.split(" ")
        assert f[0] == "B" and len(f) == 8, line
        sl = []
        for k in (2, 5):
            text = bytes.fromhex(f[k + 1][1:])
            assert len(text) == int(f[k])
            sl += [text, None if f[k + 2] == "-" else [int(x) for x in f[k + 2].split(",")]]
        out.append((int(f[1]), sl[0], sl[1], sl[2], sl[3]))
    assert (err is not None) == (r.returncode == 3)
    return out, err


def _records(text, kind):
    f = io.StringIO(text.decode(), newline=None)
    return list(gwa_cli.read_fasta(f) if kind == "fasta" else gwa_cli.read_fastq(f))


def _fastq(n, name_len, seed, messy=False, first=0, lens=(1, 30, 100)):
    """FASTQ text of records first..first+n-1 with names of name_len bytes; messy: blank lines between
    some records and CRLF line ends on every third record (the framer's line-by-line path)"""
    rnd = random.Random(seed)
    out = []
    for i in range(first, first + n):
        m = rnd.choice(lens)
        name = ("r%d_" % i).ljust(name_len, "x")[:max(name_len, len("r%d_" % i))]
        seq = "".join(rnd.choice("ACGT") for _ in range(m))
        qual = "".join(rnd.choice("@+!I5") for _ in range(m))  # ('@' and '+' may start a quality line)
        eol = "\r\n" if messy and i % 3 == 0 else "\n"
        out.append("@%s d%s%s%s+%s%s%s" % (name, eol, seq, eol, eol, qual, eol))
        if messy and rnd.random() < 0.2:
            out.append("\n")
    return "".join(out).encode()


def _fasta(n, seed):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        seq = "".join(rnd.choice("ACGT") for _ in range(rnd.choice([1, 61, 130])))
        out.append(">f%d desc\n" % i + "".join(seq[a:a + 60] + "\n" for a in range(0, len(seq), 60)))
    return "".join(out).encode()


def _check_slices(batches, batch, recs1, recs2, kind1, kind2):
    """the pair batches hold the files' records in order, exactly `batch` pairs in all but the last"""
    n = len(recs1)
    assert [b[0] for b in batches] == [min(batch, n - a) for a in range(0, n, batch)]
    at = 0
    for pairs, t1, s1, t2, s2 in batches:
        for text, starts, recs, kind in ((t1, s1, recs1, kind1), (t2, s2, recs2, kind2)):
            assert _records(text, kind) == recs[at:at + pairs]
            if kind == "fastq":  # each start is its record's header line
                assert len(starts) == pairs and starts[0] == 0 and starts == sorted(set(starts))
                for k, s in enumerate(starts):
                    assert text[s:s + 1] == b"@" and (s == 0 or text[s - 1:s] in (b"\n", b"\r"))
                    assert _records(text[s:starts[k + 1] if k + 1 < pairs else len(text)], kind) == [recs[at + k]]
            else:
                assert starts is None
        at += pairs
    assert at == n


@pytest.mark.parametrize("messy", [False, True])
def test_two_files_zip_into_equal_batches(prog, tmp_path, messy):
    # 40-B names against 2-B names: the files' chunks hold different record counts
    t1, t2 = _fastq(N, 40, 1, messy), _fastq(N, 2, 2, messy)
    (tmp_path / "a_1.fq").write_bytes(t1)
    (tmp_path / "a_2.fq").write_bytes(t2)
    r1, r2 = _records(t1, "fastq"), _records(t2, "fastq")
    assert len(r1) == len(r2) == N
    for chunk in CHUNKS:
        for batch in BATCHES:
            got, err = _run(prog, chunk, batch, tmp_path / "a_1.fq", tmp_path / "a_2.fq")
            assert err is None, (chunk, batch, err)
            _check_slices(got, batch, r1, r2, "fastq", "fastq")
            if not messy:  # no blank lines: the slices tile each file byte for byte
                assert b"".join(b[1] for b in got) == t1 and b"".join(b[3] for b in got) == t2, (chunk, batch)


def test_records_larger_than_a_chunk_carry(prog, tmp_path):
    # every record (about 250 B) spans several 64-B chunks, and a batch of 500 leaves no chunk before
    # the last: the whole file is carried, far beyond the 128 B of room before a chunk
    t1, t2 = _fastq(9, 40, 3, lens=(100, 120)) + b"@last\nACGT\n+\nIIII", _fastq(9, 2, 4, lens=(100, 120)) + b"@l\nAC\n+\nII\n\n\n"
    assert min(len(x) for x in t1.split(b"@r")[1:]) > 64
    (tmp_path / "c_1.fq").write_bytes(t1)
    (tmp_path / "c_2.fq").write_bytes(t2)
    r1, r2 = _records(t1, "fastq"), _records(t2, "fastq")
    for batch in (1, 3, 500):
        got, err = _run(prog, 64, batch, tmp_path / "c_1.fq", tmp_path / "c_2.fq")
        assert err is None
        _check_slices(got, batch, r1, r2, "fastq", "fastq")
        assert b"".join(b[1] for b in got) == t1  # (a last line without its newline is kept as it is)


def test_compressed_and_fasta_mates(prog, tmp_path):
    t1, t2, t3 = _fastq(N, 40, 5), _fastq(N, 2, 6, messy=True), _fasta(N, 7)
    with gzip.open(tmp_path / "m_1.fq.gz", "wb") as f:
        f.write(t1)
    (tmp_path / "m_2.fq.snap").write_bytes(make_snap.stream(t2, chunk=1000))
    (tmp_path / "m_3.fa").write_bytes(t3)
    r1, r2, r3 = _records(t1, "fastq"), _records(t2, "fastq"), _records(t3, "fasta")
    for chunk in (64, 333, 4096):
        for batch in BATCHES:
            got, err = _run(prog, chunk, batch, tmp_path / "m_1.fq.gz", tmp_path / "m_2.fq.snap")
            assert err is None
            _check_slices(got, batch, r1, r2, "fastq", "fastq")
            got, err = _run(prog, chunk, batch, tmp_path / "m_3.fa", tmp_path / "m_1.fq.gz")
            assert err is None
            _check_slices(got, batch, r3, r1, "fasta", "fastq")


def test_interleaved_file_splits_and_odd_count_fails(prog, tmp_path):
    t = _fastq(2 * N, 9, 8, messy=True)
    (tmp_path / "i.fq").write_bytes(t)
    recs = _records(t, "fastq")
    odd = _fastq(2 * N - 1, 9, 8, messy=True)
    (tmp_path / "odd.fq").write_bytes(odd)
    for chunk in (64, 257, 1 << 20):
        for batch in BATCHES:
            got, err = _run(prog, chunk, batch, tmp_path / "i.fq")
            assert err is None
            assert [b[0] for b in got] == [min(batch, N - a) for a in range(0, N, batch)]
            at = 0
            for pairs, text, starts, t2, s2 in got:
                assert t2 == b"" and s2 is None and len(starts) == 2 * pairs
                assert _records(text, "fastq") == recs[at:at + 2 * pairs]
                at += 2 * pairs
            got, err = _run(prog, chunk, batch, tmp_path / "odd.fq")
            assert err is not None and "odd number of reads" in err
            assert sum(b[0] for b in got) <= N - 1


def test_mate_files_of_different_lengths_fail(prog, tmp_path):
    t1 = _fastq(N, 40, 1)
    (tmp_path / "a_1.fq").write_bytes(t1)
    (tmp_path / "short_2.fq").write_bytes(_fastq(N - 1, 2, 2))
    (tmp_path / "long_2.fq").write_bytes(_fastq(N + 1, 2, 2))
    (tmp_path / "much_2.fq").write_bytes(_fastq(N + 20, 2, 2))
    for other in ("short_2.fq", "long_2.fq", "much_2.fq"):
        for chunk in (64, 4096) if other != "much_2.fq" else (257,):
            for batch in BATCHES:
                for a, b in ((tmp_path / "a_1.fq", tmp_path / other), (tmp_path / other, tmp_path / "a_1.fq")):
                    got, err = _run(prog, chunk, batch, a, b)
                    assert err == "the mate files hold different numbers of reads", (other, chunk, batch, err)
                    assert sum(x[0] for x in got) <= N
