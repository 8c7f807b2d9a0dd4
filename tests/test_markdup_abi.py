"""The ctypes mirrors of the duplicate-marking structs have the C layout: gwa_markdup_stats_t through
test_abi_layout's generated C program, and the 24-byte entry of gwa_batch_results_bam_dupinfo as include/gwa.h
words it (u64, u64, u32, u32).  CPU only."""
import ctypes
import shutil

import pytest

import test_abi_layout as T

gwa = T.gwa


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_markdup_stats_layout(tmp_path, monkeypatch):
    monkeypatch.setattr(T, "PAIRS", [("gwa_markdup_stats_t", gwa.MarkdupStats)])
    T.test_ctypes_mirrors_match_c_layout(tmp_path)
    assert ctypes.sizeof(gwa.MarkdupStats) == 6 * 8 + 2 * 8


def test_dupinfo_entry_layout():
    c = gwa.BamDupInfo
    assert ctypes.sizeof(c) == 24
    assert [(n, getattr(c, n).offset, getattr(c, n).size) for n, _ in c._fields_] == [
        ("endKey", 0, 8), ("mateKey", 8, 8), ("score", 16, 4), ("leader", 20, 4)]
