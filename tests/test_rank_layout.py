"""The midpoint Occ-block layout (OccBlock, gwa_layout.h) on the CPU: tests/hostcore/rank_check.cpp
builds the host index of small texts in the flagged and in the forced plain mode and compares
rankOne / rankAll at every position, the clamp at N + 1, the has-N bits and kmerInterval with naive
counts over the BWT (see the program's header for the texts).  Built with the host compiler, once
plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer, and run as a program of its
own.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcore")
CSRC = os.path.join(os.path.dirname(HERE), "genome-weaver-align_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS"]

pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="no host C++ compiler")


def _build(out, extra):
    cmd = [CXX, "-O1", "-std=c++17", "-fopenmp", "-I", CSRC] + extra + [
        "-o", str(out), os.path.join(HC, "rank_check.cpp"), os.path.join(CSRC, "host_index.cpp")]
    subprocess.check_call(cmd)
    return str(out)


def _run(exe):
    env = dict(os.environ)
    env.update({"OMP_NUM_THREADS": "2", "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1",
                "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    p = subprocess.run([exe], capture_output=True, env=env, timeout=600)
    err = p.stderr.decode(errors="replace")
    for tag in ("Sanitizer", "runtime error"):
        assert tag not in err, err[-6000:]
    assert p.returncode == 0, (p.returncode, err[-4000:])
    out = p.stdout.decode()
    assert out.startswith("rank_check ok"), out
    return out


def test_rank_exhaustive_both_modes(tmp_path):
    out = _run(_build(tmp_path / "rank_check", []))
    # every kind of block was among the texts: no N, N in half 0 only, in half 1 only, in both
    kinds = [int(x) for x in out.strip().rsplit(":", 1)[1].split()]
    assert len(kinds) == 4 and min(kinds) > 0 and kinds[0] > sum(kinds[1:])


def _sanitizer_runtime(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.call([CXX] + SAN + ["-o", str(tmp_path / "probe"), str(src)], stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL) == 0


def test_rank_exhaustive_under_asan_ubsan(tmp_path):
    if not _sanitizer_runtime(tmp_path):
        pytest.skip("the toolchain has no AddressSanitizer / UBSan runtime")
    _run(_build(tmp_path / "rank_check_san", SAN))
