"""What BGZF compression of the SAM text costs on the device (GPU box): one resident index, the C2 reads
(100 bp, 0-2 substitutions, constant qualities) in one batch, aligned once; then gwa_batch_format and
gwa_batch_format_bgzf alternately.  Prints format_ms of the plain formatting, format_ms + compress_ms of
the BGZF one, plain and BGZF bytes, the stored-block count, and -- after the timed part -- the size zlib
level 1 gives for the same 65 280-byte cuts of a 64 MB sample of the text, next to the device encoder's
size for that sample.  The floor beside it: reading the text and writing the blocks at the streaming rate.

  python tools/bgzf_cost.py [--genome hg19|hg19r|<Mbp>] [--reads N] [--steps K]
"""
import argparse
import os
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "genome-weaver-align_amd")]

STREAM_B_PER_S = 6.0e12  # a streaming kernel's bytes
SLICE = 65280


def say(*a):
    print("[bgzf_cost]", *a, flush=True)


def stat(v):
    v = sorted(v)
    return "%.3f (%.3f-%.3f)" % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="hg19")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--sample-mb", type=int, default=64)
    args = ap.parse_args()
    import numpy as np
    import gwa
    import synth
    m, n = 100, args.reads
    t0 = time.time()
    if args.genome in ("hg19", "hg19r"):
        gen = synth.genome_repeats if args.genome == "hg19r" else synth.genome_ngaps
        codes, names, lengths = gen(synth.HG19_CONTIGS, config_id=1)
    else:
        codes, names, lengths = synth.genome([("chr1", int(float(args.genome) * 1e6))], 1)
    seqs = synth.reads_codes(codes, lengths, n, m, 2, config_id=2)
    seq_blob = synth.SYM[seqs].tobytes()
    del seqs
    off = np.arange(0, m * (n + 1), m, dtype=np.uint64)
    nb, no = synth.name_blob(n)
    blobs = (nb, no, seq_blob, off, b"I" * (m * n), off)
    say("genome + %d reads in %.0fs" % (n, time.time() - t0))
    t0 = time.time()
    gi = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths)
    del codes
    b = gwa.Batch(gi, gwa.AlignmentConfig(k=2.0), blobs=blobs)
    b.run()
    say("index + batch aligned in %.0fs" % (time.time() - t0))
    plain_ms, bgzf_fmt_ms, comp_ms = [], [], []
    for rep in range(args.steps + 1):
        plain = b.format_device()
        st = b.stats()
        if rep:
            plain_ms.append(st.format_ms)
        z = b.format_bgzf()
        st = b.stats()
        if rep:
            bgzf_fmt_ms.append(st.format_ms)
            comp_ms.append(st.compress_ms)
    say("gwa_batch_format:      format_ms %s, %d bytes" % (stat(plain_ms), plain))
    say("gwa_batch_format_bgzf: format_ms %s + compress_ms %s, %d bytes in %d blocks (%d stored), %.4f of the plain bytes"
        % (stat(bgzf_fmt_ms), stat(comp_ms), z, st.bgzf_blocks, st.bgzf_stored, z / max(1, plain)))
    floor = (plain + 2 * (plain + 31 * st.bgzf_blocks) + 2 * z) / STREAM_B_PER_S
    say("floor of compress_ms at %.1f TB/s: the text read, the slots zeroed and written, the blocks read and written: %.3f ms"
        % (STREAM_B_PER_S / 1e12, floor * 1e3))
    med = sorted(comp_ms)[len(comp_ms) // 2]
    say("%.2f GB/s of text, %.1f us per block per CU at 256 CUs" % (plain / med / 1e6, med * 1e3 * 256 / max(1, st.bgzf_blocks)))
    # after the timed part: zlib level 1 on a sample of the same text, cut the same way
    k = min(n, args.sample_mb * (1 << 20) * n // max(1, plain))
    text = b.results(0, k)[0].encode()
    t0 = time.time()
    zl = 0
    for at in range(0, len(text), SLICE):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        zl += len(c.compress(text[at:at + SLICE]) + c.flush()) + 26
    tz = time.time() - t0
    dev = len(gwa.bgzf_compress(text, device=gi.device))
    say("sample of %d reads, %d bytes: device encoder %d (%.4f), zlib level 1 %d (%.4f; %.1fs on one core = %.0f MB/s); "
        "device / zlib = %.3f" % (k, len(text), dev, dev / len(text), zl, zl / len(text), tz, len(text) / tz / 1e6, dev / zl))
    b.close()
    gi.close()


if __name__ == "__main__":
    main()
