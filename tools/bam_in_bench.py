"""Measurements of BAM as read input: the decode kernels over synthetic 100-bp records
resident in HBM (gwa_bam_reads_decode_timed) next to their memory floor, and the file-level rate of
`align reads.bam` against the same reads as a BGZF `.fastq.gz`, with the pipeline's stage times.

  python tools/bam_in_bench.py [--reads 1000000] [--genome 1000000] [--device 0] [--dir DIR]

Prints one JSON line.  The files are built with numpy (fixed-width records) and compressed on the device."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.dirname(os.path.abspath(__file__))]

import gwa  # noqa: E402
import synth  # noqa: E402

HBM_BYTES_PER_S = 8e12


def build(n, m, codes, lengths, rng):
    """(headerless BAM records, FASTQ text) of n reads of m bases (m even): a quarter stored reverse-strand"""
    seqs = synth.reads_codes(codes, lengths, n, m, 2)  # codes 0..3
    names = np.frombuffer(synth.name_blob(n)[0], dtype=np.uint8).reshape(n, 10)
    qual = rng.integers(2, 41, (n, m), dtype=np.uint8)
    rev = rng.random(n) < 0.25
    # FASTQ
    fq = np.empty((n, 1 + 10 + 1 + m + 3 + m + 1), dtype=np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1:11] = names
    fq[:, 11] = 10
    fq[:, 12:12 + m] = np.frombuffer(b"ACGT", dtype=np.uint8)[seqs]
    fq[:, 12 + m:15 + m] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    fq[:, 15 + m:15 + 2 * m] = qual + 33
    fq[:, 15 + 2 * m] = 10
    # BAM: the stored SEQ / QUAL of a reverse record are the reverse complement / the reverse
    st = np.where(rev[:, None], 3 - seqs[:, ::-1], seqs)
    sq = np.where(rev[:, None], qual[:, ::-1], qual)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[st]
    size = 36 + 11 + m // 2 + m
    rec = np.zeros((n, size), dtype=np.uint8)
    rec[:, 0:4] = np.frombuffer(np.uint32(size - 4).tobytes(), dtype=np.uint8)
    rec[:, 4:12] = 0xFF  # refID, pos -1
    rec[:, 12] = 11
    rec[:, 14:16] = np.frombuffer(np.uint16(4680).tobytes(), dtype=np.uint8)
    rec[:, 18] = np.where(rev, 4 | 16, 4)
    rec[:, 20:24] = np.frombuffer(np.uint32(m).tobytes(), dtype=np.uint8)
    rec[:, 24:32] = 0xFF
    rec[:, 36:46] = names
    rec[:, 47:47 + m // 2] = nib[:, 0::2] << 4 | nib[:, 1::2]
    rec[:, 47 + m // 2:] = sq
    return rec.tobytes(), fq.tobytes()


def header(names, lengths):
    import struct
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(names, lengths)).encode()
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(names))
    for n, l in zip(names, lengths):
        out += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", int(l))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ns = ap.parse_args()
    rng = np.random.default_rng(3)
    codes, names, lengths = synth.genome([("chr1", ns.genome * 6 // 10), ("chr2", ns.genome * 4 // 10)], 1)
    recs, fq = build(ns.reads, 100, codes, lengths, rng)
    res = {"reads": ns.reads, "record_bytes": len(recs)}
    n, ms = gwa.bam_reads_decode_timed(recs, device=ns.device, repeat=5)
    # read: the records once, their starts; written: two 112-byte slots and six field words per read
    moved = len(recs) + 8 * n + n * (2 * 112 + 6 * 8 + 1)
    res.update(decode_kernel_ms=round(ms, 4), decode_bytes_moved=moved, decode_floor_ms=round(moved / HBM_BYTES_PER_S * 1e3, 4))
    d = ns.dir or tempfile.mkdtemp(prefix="bam_in_bench")
    bam, gz = os.path.join(d, "reads.bam"), os.path.join(d, "reads.fastq.gz")
    with open(bam, "wb") as f:
        f.write(gwa.bgzf_compress(header(names, lengths) + recs, device=ns.device) + gwa.BGZF_EOF)
    with open(gz, "wb") as f:
        f.write(gwa.bgzf_compress(fq, device=ns.device) + gwa.BGZF_EOF)
    fm = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths, device=ns.device)
    pipe = gwa.Pipeline([fm], gwa.AlignmentConfig(k=2.0))
    sams = {}
    for rep in range(2):  # the first pass pins the buffers and warms the caches
        for key, path in (("bam", bam), ("fastq_gz", gz)):
            out = os.path.join(d, key + ".sam")
            fd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            t0 = time.perf_counter()
            got = pipe.align_file(path, fd)
            dt = time.perf_counter() - t0
            os.close(fd)
            st = pipe.stats()
            sams[key] = open(out, "rb").read()
            res[key] = {"reads": got, "file_bytes": os.path.getsize(path), "wall_s": round(dt, 4),
                        "reads_per_s": round(got / dt), "read_s": round(st.read_s, 4), "inflate_s": round(st.inflate_s, 4),
                        "frame_s": round(st.frame_s, 4), "setup_s": round(st.setup_s, 4),
                        "kernel_s": round(st.device_kernel_s[0], 4), "format_s": round(st.format_s, 4),
                        "write_s": round(st.write_s, 4)}
    res["sam_identical"] = sams["bam"] == sams["fastq_gz"]
    pipe.close()
    fm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
