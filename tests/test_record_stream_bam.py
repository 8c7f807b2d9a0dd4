"""The framing of BAM read files by the pipeline's reader (csrc/record_stream.cpp, format 2) on the CPU:
tests/record_stream_bam.cpp, a program of its own built with the host compiler under AddressSanitizer +
UndefinedBehaviorSanitizer, reads files whose header (about 70 000 bytes of text) spans two 65 536-byte
chunks and whose records straddle BGZF members and chunks, and its slices are compared with
tests/ubam_ref.py: the count of reads, their starts, the skipped records, and where each slice stands in the
inflated stream.  No GPU."""
import gzip
import os
import shutil
import subprocess

import pytest

import bam_ref
import ubam_ref as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")

CONTIGS = [("chr1", 30000), ("chr2", 20000)]
TEXT = "@CO\t" + "x" * 69990 + "\n"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rsbam") / "record_stream_bam")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-pthread"] + SAN + [
        os.path.join(HERE, "record_stream_bam.cpp"), os.path.join(CSRC, "record_stream.cpp"),
        os.path.join(CSRC, "reads_io.cpp"), os.path.join(CSRC, "snappy_stream.cpp"), "-lz", "-o", out]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]

    def run(batch, mode, *paths, env=None):
        e = dict(os.environ, **ENV)
        e.update(env or {})
        r = subprocess.run([out, "65536", str(batch), mode] + [str(p) for p in paths], capture_output=True, env=e, timeout=300)
        err = r.stderr.decode(errors="replace")
        assert r.returncode in (0, 3) and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
        lines = r.stdout.decode().splitlines()
        errs = [x[2:] for x in lines if x.startswith("E ")]
        assert bool(errs) == (r.returncode == 3)
        kinds = [int(x) for x in lines[0].split()[1:]] if lines[0].startswith("K") else []  # (E alone: the open failed)
        fmts = [int(x) for x in lines[1].split()[1:]] if len(lines) > 1 and lines[1].startswith("F") else []
        batches = []
        for x in lines:
            if x.startswith("B "):
                f = x.split(" ")
                slices = []
                for k in range(2, len(f), 6):
                    fmt, rec, off, ln, hx, st = f[k:k + 6]
                    if fmt != "-":
                        slices.append((int(fmt), int(rec), int(off), bytes.fromhex(hx[1:]),
                                       [int(v) for v in st.split(",")] if st != "-" else []))
                        assert len(slices[-1][3]) == int(ln)
                batches.append((int(f[1]), slices))
        return kinds, fmts, batches, errs[0] if errs else None

    return run


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bams")
    recs = U.random_records(1500, seed=3)
    (d / "reads.bam").write_bytes(U.bam_file(recs, TEXT, CONTIGS, seed=4))
    return d, recs


def _check_slices(batches, recs, B, header):
    kept, n_all = U.kept_starts(recs)
    index_of = {at: k for k, (at, _) in enumerate(U.walk(recs))}
    assert len(kept) < n_all  # (some records are skipped)
    seen, reads = [], []
    for i, (n, slices) in enumerate(batches):
        (fmt, rec_index, byte_off, data, starts), = slices
        assert fmt == 2 and n == len(starts) and (n == B or i == len(batches) - 1) and n > 0
        at = byte_off - header
        assert recs[at:at + len(data)] == data
        assert starts[0] == 0 and rec_index == index_of[at]
        seen += [at + s for s in starts]
        reads += U.reads_of(data)
    assert seen == kept
    assert reads == U.reads_of(recs)


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_framing_with_a_header_spanning_two_chunks(prog, files, batch):
    d, recs = files
    header = len(bam_ref.header(CONTIGS, TEXT))
    assert 65536 < header < 2 * 65536 and header + len(recs) > 3 * 65536
    kinds, fmts, batches, err = prog(batch, "single", d / "reads.bam")
    assert (kinds, fmts, err) == ([3], [2], None)
    _check_slices(batches, recs, batch, header)


def test_framing_through_zlib_and_without_an_eof_marker(prog, files, tmp_path):
    d, recs = files
    header = len(bam_ref.header(CONTIGS, TEXT))
    kinds, fmts, batches, err = prog(64, "single", d / "reads.bam", env={"GWA_BGZF_INPUT": "0"})
    assert (kinds, fmts, err) == ([0], [2], None)
    _check_slices(batches, recs, 64, header)
    (tmp_path / "noeof.bam").write_bytes(U.bam_file(recs, "", [], seed=9, eof=False))
    kinds, fmts, batches, err = prog(64, "single", tmp_path / "noeof.bam")
    assert err is None
    _check_slices(batches, recs, 64, len(bam_ref.header([], "")))
    # no read at all: a header alone, and skipped records alone
    (tmp_path / "none.bam").write_bytes(U.bam_file(b"", TEXT, CONTIGS))
    assert prog(7, "single", tmp_path / "none.bam")[2:] == ([], None)
    (tmp_path / "skipped.bam").write_bytes(U.bam_file(dict(U.cases())["skip_all"]))
    assert prog(7, "single", tmp_path / "skipped.bam")[2:] == ([], None)


def test_interleaved_and_mate_files(prog, files, tmp_path):
    d, recs = files
    kept, _ = U.kept_starts(recs)
    # an even and an odd number of reads: the file as it is, and with one more read at its end
    extra = U.read_record("last", "ACGT", "IIII")
    even, odd = (recs, recs + extra) if len(kept) % 2 == 0 else (recs + extra, recs)
    (tmp_path / "even.bam").write_bytes(U.bam_file(even, TEXT, CONTIGS, seed=6))
    (tmp_path / "odd.bam").write_bytes(U.bam_file(odd, TEXT, CONTIGS, seed=7))
    n_even = len(U.kept_starts(even)[0])
    assert n_even % 2 == 0 and len(U.kept_starts(odd)[0]) % 2 == 1
    kinds, fmts, batches, err = prog(7, "inter", tmp_path / "even.bam")
    assert (kinds, fmts, err) == ([3], [2], None) and sum(n for n, _ in batches) == n_even // 2
    assert all(len(s) == 1 and len(s[0][4]) == 2 * n for n, s in batches)
    assert all(n == 7 for n, _ in batches[:-1])
    assert [r for _, s in batches for r in U.reads_of(s[0][3])] == U.reads_of(even)
    assert "odd number of reads" in prog(7, "inter", tmp_path / "odd.bam")[3]
    fq = U.fastq_of([(n, s, q or "I" * len(s)) for n, s, q in U.reads_of(recs)])
    (tmp_path / "m_2.fq").write_bytes(fq)
    kinds, fmts, batches, err = prog(7, "pair", d / "reads.bam", tmp_path / "m_2.fq")
    assert (kinds, fmts, err) == ([3, 0], [2, 1], None)
    assert sum(n for n, _ in batches) == len(kept) and all(s[0][0] == 2 and s[1][0] == 1 for _, s in batches)


def test_malformed_files(prog, files, tmp_path):
    d, recs = files
    raw = U.bam_bytes(recs, TEXT, CONTIGS)
    header = len(bam_ref.header(CONTIGS, TEXT))
    n_all = len(U.walk(recs))
    last = U.walk(recs)[-1][0]

    def err_of(name, data, z=True):
        p = tmp_path / name
        p.write_bytes(U.inflate_ref.cut_members(data, seed=2) if z else data)
        e = prog(64, "single", p)[3]
        assert e is not None and e.startswith(str(p) + ": "), e
        return e[len(str(p)) + 2:]

    assert "no BAM magic" in err_of("magic.bam", b"BAM\2" + raw[4:])
    assert "no BAM magic" in err_of("fastq.bam", b"@r\nACGT\n+\nIIII\n")
    assert err_of("header.bam", raw[:header - 5]) == "the BAM header is cut off by the end of the file (%d bytes)" % (header - 5)
    assert "the BAM header is cut off" in err_of("empty.bam", b"")
    bs = len(recs) - last - 4
    assert err_of("record.bam", raw[:-3]) == "BAM record %d at byte %d: block_size %d runs past the data's end (%d bytes)" % (
        n_all - 1, header + last, bs, len(raw) - 3)
    assert err_of("record2.bam", raw + b"\x01\x02") == \
        "BAM record %d at byte %d: the chain of block_size fields ends 2 bytes before the data's end" % (n_all, len(raw))
    bad = bytearray(raw)
    at = header + U.walk(recs)[700][0]
    bad[at:at + 4] = (31).to_bytes(4, "little")
    assert err_of("small.bam", bytes(bad)) == "BAM record 700 at byte %d: block_size 31 is below the 32 fixed bytes" % at
    e = err_of("gzip.bam", gzip.compress(raw), z=False)
    assert "not a BAM file: the first BGZF member is missing" in e
