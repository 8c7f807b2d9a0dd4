"""BAM as read input on the CPU (include/gwa.h "BAM input"): the host build of the decoder
(csrc/bam_in_core.h) against the pure-Python reference tests/ubam_ref.py.  tests/bam_in_host.cpp is a program
of its own, built with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer; every case's
records sit in a heap block of exactly their size there.  The library's gwa_bam_reads_decode(device < 0) and
gwa_bam_header_size are compared on the same cases.  tests/test_gpu_bam_in.py compares the kernels with both.
No GPU."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

import bam_ref
import ubam_ref as U

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}

needs_cxx = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_in")
    out = str(d / "bam_in_host")
    p = subprocess.run([CXX, "-std=c++17", "-O1", "-g"] + SAN + [os.path.join(HERE, "bam_in_host.cpp"), "-o", out],
                       capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]

    def run(inputs):
        path = d / "cases.bin"
        path.write_bytes(struct.pack("<I", len(inputs)) + b"".join(struct.pack("<Q", len(x)) + x for x in inputs))
        r = subprocess.run([out, str(path)], capture_output=True, env=dict(os.environ, **ENV), timeout=300)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
        res = []
        for line in r.stdout.decode("latin-1").splitlines():
            if line.startswith("C "):
                res.append([[], None])
            elif line.startswith("E "):
                res[-1][1] = line[2:]
            else:
                _, name, seq, qual = line.split(" ")
                unhex = lambda h: "" if h == "-" else bytes.fromhex(h).decode("latin-1")  # noqa: E731
                res[-1][0].append((unhex(name), "" if seq == "-" else seq, None if qual == "*" else unhex(qual)))
        assert len(res) == len(inputs)
        return res

    return run


@needs_cxx
def test_host_build_decodes_every_case_as_the_reference(host_prog):
    cases = U.cases()
    names = [c[0] for c in cases]
    for ln in U.LENGTHS:
        assert "len%d_flag4" % ln in names and "len%d_flag20" % ln in names
    res = host_prog([c[1] for c in cases])
    for (name, data), (reads, err) in zip(cases, res):
        assert err is None, (name, err)
        assert reads == U.reads_of(data), name
    # the packed SEQ stood at every offset mod 16
    offs = set()
    for name, data in cases:
        for at in U.kept_starts(data)[0]:
            offs.add((at + 36 + data[at + 12] + 4 * struct.unpack_from("<H", data, at + 16)[0]) % 16)
    assert offs == set(range(16))
    # all cases as one chain
    whole = b"".join(c[1] for c in cases)
    reads, err = host_prog([whole])[0]
    assert err is None and reads == U.reads_of(whole) and len(reads) > 1500


@needs_cxx
def test_host_build_words_every_malformed_input(host_prog):
    cases = U.malformed()
    assert len(cases) >= 8
    res = host_prog([c[1] for c in cases])
    for (name, data, msg), (_, err) in zip(cases, res):
        assert err == msg, name
        with pytest.raises(U.UbamError) as e:
            U.reads_of(data)
        assert str(e.value) == msg, name


# ---- the library's host path (no device is touched) --------------------------------------------------------

sys.path.insert(0, os.path.join(REPO, "genome-weaver-align_amd"))
import gwa  # noqa: E402


def test_library_host_decode_equals_the_reference():
    for name, data in U.cases():
        assert gwa.bam_reads_decode(data, device=-1) == U.reads_of(data), name
    for name, data, msg in U.malformed():
        with pytest.raises(gwa.GwaError) as e:
            gwa.bam_reads_decode(data, device=-1)
        assert str(e.value) == msg, name
    good = U.read_record("g", "ACGTN", "IIII!", 0x10)
    assert gwa.bam_reads_decode(good) == [("g", "ACGTN", "IIII!")]


def test_header_size():
    contigs = [("chr1", 30000), ("chr%d" % 2, 20000)]
    text = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:30000\n"
    recs = U.random_records(20)
    for tx, cs in (("", []), (text, contigs), ("x" * 70000, contigs)):
        raw = U.bam_bytes(recs, tx, cs)
        h = gwa.bam_header_size(raw)
        assert h == len(bam_ref.header(cs, tx)) == bam_ref.parse_header(raw)[2]
        assert gwa.bam_reads_decode(raw[h:]) == U.reads_of(recs)
        assert gwa.bam_header_size(raw[:h]) == h
        for cut in (0, 3, 7, h - 1):
            with pytest.raises(gwa.GwaError, match="end inside the header"):
                gwa.bam_header_size(raw[:cut])
    with pytest.raises(gwa.GwaError, match="no BAM magic"):
        gwa.bam_header_size(b"BAM\2" + bytes(20))
    with pytest.raises(gwa.GwaError, match="no BAM magic"):
        gwa.bam_header_size(b"@r0\nACGT\n+\nIIII\n")
