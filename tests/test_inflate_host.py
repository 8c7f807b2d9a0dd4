"""The BGZF decoder (csrc/inflate_core.h) on the CPU: tests/inflate_host.cpp, a program of its own built
with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, replays the device kernel's
lanes phase by phase over the inputs of tests/inflate_ref.py -- members zlib wrote with every strategy and
flush, the project's own encoder's output, and malformed members down to hand-written bit streams.  A
well-formed input must inflate to its text; a malformed one must end with a status, never with a sanitizer
report and never with status 0 and other bytes.  tests/record_stream_bgzf.cpp drives the pipeline's reader
over BGZF read files the same way.  tests/test_gpu_inflate.py compares the device kernel with this build
on the same inputs.  No GPU."""
import gzip
import os
import shutil
import struct
import subprocess

import pytest

import bgzf_ref
import inflate_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")


def _clean(r, ok=(0,)):
    err = r.stderr.decode(errors="replace")
    for tag in ("Sanitizer", "runtime error"):
        assert tag not in err, err[-6000:]
    assert r.returncode in ok, (r.returncode, err[-4000:])


@pytest.fixture(scope="module")
def inflate_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_host")
    exe = d / "inflate_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-I", CSRC] + SAN + ["-o", str(exe), os.path.join(HERE, "inflate_host.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]
    count = [0]

    def run(cases):
        """per case: ("text", bytes) | ("walk", message) | ("member", index, status code, payload bit)"""
        count[0] += 1
        src, dst = d / ("in%d" % count[0]), d / ("out%d" % count[0])
        src.write_bytes(struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(c)) + c for c in cases))
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, env=dict(os.environ, **ENV), timeout=600)
        _clean(r)
        o, at, res = dst.read_bytes(), 0, []
        while at < len(o):
            kind = o[at]
            at += 1
            if kind == 0:
                (n,) = struct.unpack_from("<Q", o, at)
                res.append(("text", o[at + 8:at + 8 + n]))
                at += 8 + n
            elif kind == 1:
                (n,) = struct.unpack_from("<I", o, at)
                res.append(("walk", o[at + 4:at + 4 + n].decode()))
                at += 4 + n
            else:
                idx, st = struct.unpack_from("<II", o, at)
                res.append(("member", idx, st & 0xff, st >> 8))
                at += 8
        assert len(res) == len(cases)
        return res

    return run


def test_encoders_give_the_intended_block_types():
    le = R.low_entropy(5000)
    want = {"l0": 0, "l1": 2, "l6": 2, "l9": 2, "fixed": 1, "huff": 2, "rle": 2}
    for enc, (level, strategy) in R.ENCODERS.items():
        assert (R.deflate(le, level, strategy)[0] >> 1) & 3 == want[enc], enc
    # a sync flush in mid-stream: the empty stored block 00 00 ff ff, and a first block that is not final
    p = R.deflate(le, 6, cuts=(2000,), flush=R.zlib.Z_SYNC_FLUSH)
    assert b"\x00\x00\xff\xff" in p and not p[0] & 1


def test_well_formed_inputs_inflate_to_their_text(inflate_host):
    cases = R.well_formed()
    names = {c[0] for c in cases}
    for n in R.LENGTHS:  # every length with at least the Huffman encoders (stored: where a member can hold it)
        for enc in ("l1", "l6", "l9", "fixed", "rle"):
            assert "len%d_%s" % (n, enc) in names
    assert "len65279_l0" in names and "len65536_huff" in names
    res = inflate_host([c[2] for c in cases])
    for (name, text, _), r in zip(cases, res):
        assert r[0] == "text", (name, r)
        assert r[1] == text, name


@pytest.fixture(scope="module")
def bgzf_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_enc")
    exe = d / "bgzf_host"
    cmd = [CXX, "-O1", "-g", "-std=c++17", "-I", CSRC] + SAN + ["-o", str(exe), os.path.join(HERE, "bgzf_host.cpp")]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]

    def run(name, data):
        src, dst = d / (name + ".in"), d / (name + ".out")
        src.write_bytes(data)
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, env=dict(os.environ, **ENV), timeout=600)
        _clean(r)
        return dst.read_bytes()

    return run


def test_the_projects_encoder_output_decodes_back(inflate_host, bgzf_host):
    from test_bgzf_host import INPUTS
    inputs = INPUTS()
    names = sorted(inputs)
    res = inflate_host([bgzf_host(n, inputs[n]) for n in names])
    for n, r in zip(names, res):
        assert r == ("text", inputs[n]), n


BASE = R.low_entropy(300, seed=6)


def test_payload_truncated_at_every_length(inflate_host):
    p = R.deflate(BASE)
    res = inflate_host([R.member(BASE, p[:k]) for k in range(len(p))])
    for k, r in enumerate(res):
        assert r[0] == "member" and r[1] == 0 and r[2] != 0, (k, r)
    assert inflate_host([R.member(BASE, p)]) == [("text", BASE)]


def test_single_bit_flips_never_give_other_bytes(inflate_host):
    p = R.deflate(BASE)
    assert len(p) >= 64
    flips = [bytes(b ^ (1 << (i & 7)) if j == i >> 3 else b for j, b in enumerate(p)) for i in range(64 * 8)]
    res = inflate_host([R.member(BASE, q) for q in flips])
    errors = 0
    for i, r in enumerate(res):
        if r[0] == "text":
            assert r[1] == BASE, "bit %d: status 0 with other bytes" % i
        else:
            assert r[0] == "member" and r[2] != 0, (i, r)
            errors += 1
    assert errors > 500  # (a flip may leave the text as it was; hardly any does)


def test_hand_built_streams_end_with_their_status(inflate_host):
    cases = R.malformed()
    res = inflate_host([c[1] for c in cases])
    for (name, _, code), r in zip(cases, res):
        assert r[0] == "member" and r[1] == 0 and r[2] == code, (name, code, r)
    assert len(R.one_per_code()) == 12
    # a malformed member between well-formed ones: its index is reported
    good = R.member(BASE)
    res = inflate_host([good + bgzf_ref.EOF + cases[-1][1] + good])
    assert res[0][:3] == ("member", 2, R.CRC)


def test_header_faults_are_found_by_the_walk(inflate_host):
    cases = R.header_faults()
    res = inflate_host([c[1] for c in cases])
    for (name, _, msg), r in zip(cases, res):
        assert r[0] == "walk" and msg in r[1], (name, r)


# ---- RecordStream with the BGZF source ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream_prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rsb") / "record_stream_bgzf")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-pthread"] + SAN + [
        os.path.join(HERE, "record_stream_bgzf.cpp"), os.path.join(CSRC, "record_stream.cpp"),
        os.path.join(CSRC, "reads_io.cpp"), os.path.join(CSRC, "snappy_stream.cpp"), "-lz", "-o", out]
    p = subprocess.run(cmd, capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-6000:]

    def run(batch, mode, *paths, env=None):
        e = dict(os.environ, **ENV)
        e.update(env or {})
        r = subprocess.run([out, "65536", str(batch), mode] + [str(p) for p in paths], capture_output=True, env=e, timeout=300)
        _clean(r, ok=(0, 3))
        lines = r.stdout.decode().splitlines()
        err = [x[2:] for x in lines if x.startswith("E ")]
        assert bool(err) == (r.returncode == 3)
        kinds = [int(x) for x in lines[0].split()[1:]] if lines and lines[0].startswith("K") else []
        return kinds, [x for x in lines if x.startswith("B ")], err[0] if err else None

    return run


def _fastq(n, seed, suffix):
    return R.fastq_text(n, seed).replace(b"/1\n", suffix + b"\n")


@pytest.fixture(scope="module")
def read_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads")
    t1, t2 = _fastq(400, 11, b"/1"), _fastq(400, 12, b"/2")
    r1, r2 = t1.split(b"@read")[1:], t2.split(b"@read")[1:]
    inter = b"".join(b"@read" + a + b"@read" + b for a, b in zip(r1, r2))
    files = {"a_1": t1, "a_2": t2, "inter": inter}
    for k, (name, t) in enumerate(files.items()):
        (d / (name + ".fq")).write_bytes(t)
        z = R.cut_members(t, seed=k + 1, eof=(k != 1))  # (the second mate file has no EOF marker)
        assert len(z) > 0 and len(t) > 65536  # several chunks of 65 536 bytes
        (d / (name + ".fq.gz")).write_bytes(z)
    return d, files


def test_bgzf_read_files_give_the_plain_files_slices(stream_prog, read_files):
    d, _ = read_files
    for batch in (1, 7, 400):
        for mode, names in (("single", ("a_1",)), ("pair", ("a_1", "a_2")), ("inter", ("inter",))):
            pk, plain, e1 = stream_prog(batch, mode, *[d / (n + ".fq") for n in names])
            zk, zipped, e2 = stream_prog(batch, mode, *[d / (n + ".fq.gz") for n in names])
            assert e1 is None and e2 is None, (e1, e2)
            assert set(pk) == {0} and set(zk) == {3}, (pk, zk)
            assert plain == zipped and len(plain) == -(-400 // batch), (batch, mode)
            # GWA_BGZF_INPUT=0: the same slices from zlib's reader
            gk, viaz, e3 = stream_prog(batch, mode, *[d / (n + ".fq.gz") for n in names], env={"GWA_BGZF_INPUT": "0"})
            assert e3 is None and set(gk) == {0} and viaz == plain


def test_a_plain_gzip_file_stays_on_the_zlib_path(stream_prog, read_files, tmp_path):
    d, files = read_files
    (tmp_path / "g.fq.gz").write_bytes(gzip.compress(files["a_1"]))
    kinds, got, err = stream_prog(7, "single", tmp_path / "g.fq.gz")
    assert err is None and kinds == [0]
    assert got == stream_prog(7, "single", d / "a_1.fq")[1]


def test_a_non_bgzf_member_in_mid_file_fails_with_its_offset(stream_prog, read_files, tmp_path):
    _, files = read_files
    t = files["a_1"]
    head = R.cut_members(t[:70000], seed=5, eof=False)
    bad = head + gzip.compress(t[70000:80000]) + R.cut_members(t[80000:], seed=6)
    (tmp_path / "bad.fq.gz").write_bytes(bad)
    n_head = len(bgzf_ref.members(head))
    kinds, got, err = stream_prog(7, "single", tmp_path / "bad.fq.gz")
    assert kinds == [3] and err is not None
    assert "BGZF member %d at byte %d: no extra field" % (n_head, len(head)) in err, err


def test_a_truncated_last_member_fails_with_its_offset(stream_prog, read_files, tmp_path):
    _, files = read_files
    z = R.cut_members(files["a_1"], seed=7, eof=False)
    ms = bgzf_ref.members(z)
    last = len(z) - (len(ms[-1][0]) + 26)
    (tmp_path / "cut.fq.gz").write_bytes(z[:-10])
    kinds, got, err = stream_prog(400, "single", tmp_path / "cut.fq.gz")
    assert kinds == [3] and err is not None
    assert "BGZF member %d at byte %d: the file ends inside the member" % (len(ms) - 1, last) in err, err
