"""What duplicate marking costs (needs a GPU, writes under $TMPDIR).  Three parts, each `--rounds`
times, the median (min-max) printed:

  kernel   gwa_bam_markdup_timed over N synthetic 100-bp pair records resident in HBM (199 bytes each, every tenth
           pair a copy of an earlier one) against the memory floor: the record bytes read once and 24 bytes
           written per record, at 8 TB/s.
  resolve  the sorter's resolve_s (and keys_s, order_s) for T single-record templates of 20 bases through
           gwa_bam_sorter_add_records in runs of 2^20 records; run under a kernel trace, the radix sorts' share
           is read from the trace.
  e2e      `gwa_cli.py align --timing --bam --sort --index` with and without --markdup over P pairs in two FASTQ
           files (mates of 100 bases from fragments of 300, every tenth pair a copy), a synthetic genome from a
           saved index; with --parent-lib NAME also the same call without --markdup through that library
           (GWA_LIB).

  python tools/markdup_cost.py [--part kernel,resolve,e2e] [--records N] [--templates T] [--pairs P] [--genome Mbp]
                               [--rounds K] [--parent-lib libgwa_parent.so]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "genome-weaver-align_amd"), os.path.join(REPO, "tools")]


def say(*a):
    print("[markdup_cost]", *a, flush=True)


def med(v):
    v = sorted(v)
    return "%.4g (%.4g-%.4g)" % (v[len(v) // 2], v[0], v[-1])


def records(n, lseq, paired, rng, span=50_000_000):
    """n records of 36 + 9 + 4 + (lseq + 1) / 2 + lseq bytes as one uint8 array: names r%07d (a pair shares one),
    CIGAR <lseq>M, random qualities 2..41, positions random on 4 contigs, every tenth template a copy of an
    earlier one's coordinates"""
    size = 36 + 9 + 4 + (lseq + 1) // 2 + lseq
    t = n // 2 if paired else n
    pos = rng.integers(0, span, t).astype(np.int32)
    ref = rng.integers(0, 4, t).astype(np.int32)
    src = np.arange(t)
    copies = np.arange(10, t, 10)
    src[copies] = rng.integers(0, copies, len(copies))
    pos, ref = pos[src], ref[src]
    rec = np.zeros((n, size), dtype=np.uint8)

    def put32(col, v):
        rec[:, col:col + 4] = v.astype("<u4").view(np.uint8).reshape(-1, 4)

    tid = np.repeat(np.arange(t), 2)[:n] if paired else np.arange(n)
    second = (np.arange(n) % 2 == 1) if paired else np.zeros(n, dtype=bool)
    put32(0, np.full(n, size - 4))
    put32(4, ref[tid])
    put32(8, np.where(second, pos[tid] + 200, pos[tid]))
    rec[:, 12] = 9
    rec[:, 16] = 1  # n_cigar_op
    flag = np.where(second, 0x93, 0x63) if paired else np.zeros(n, dtype=np.int64)
    rec[:, 18] = flag & 255
    rec[:, 19] = flag >> 8
    put32(20, np.full(n, lseq))
    put32(24, np.full(n, -1))
    put32(28, np.full(n, -1))
    rec[:, 36] = ord("r")
    for k in range(7):  # seven decimal digits, then the NUL
        rec[:, 37 + k] = ord("0") + (tid // 10 ** (6 - k)) % 10
    put32(45, np.full(n, lseq << 4))
    q0 = 49 + (lseq + 1) // 2
    rec[:, q0:q0 + lseq] = rng.integers(2, 42, (n, lseq), dtype=np.uint8)
    return rec.reshape(-1)


def part_kernel(a, gwa):
    rng = np.random.default_rng(1)
    data = records(a.records, 100, True, rng).tobytes()
    ms = []
    for _ in range(a.rounds):
        n, t = gwa.bam_markdup_timed(data, device=0, repeat=3)
        ms.append(t)
    floor = (len(data) + 24 * n) / 8e12 * 1e3
    say("kernel: %d records, %d bytes: %s ms; memory floor %.4f ms (x%.1f)" % (n, len(data), med(ms), floor, sorted(ms)[len(ms) // 2] / floor))


def part_resolve(a, gwa):
    import synth
    codes, names, lengths = synth.genome([("chr%d" % (i + 1), 20000) for i in range(4)], 1)
    fm = gwa.FMIndexOnGenome.buildFromCodes(codes, names, lengths, device=0)
    rng = np.random.default_rng(2)
    data = records(a.templates, 20, False, rng)
    size = len(data) // a.templates
    res, keys, order = [], [], []
    try:
        for _ in range(a.rounds):
            s = gwa.BamSorter(fm, markdup=True, mem=64 << 30)
            try:
                for k, at in enumerate(range(0, a.templates, 1 << 20)):
                    s.add_records(k, data[at * size:(at + (1 << 20)) * size].tobytes())
                with open(os.devnull, "wb") as f:
                    st = s.finish(f.fileno())
                ms = s.markdup_stats()
                res.append(ms.resolve_s)
                keys.append(ms.keys_s)
                order.append(st.order_s)
                last = ms
            finally:
                s.close()
    finally:
        fm.close()
    say("resolve: %d templates (%d duplicate fragment templates): resolve_s %s, keys_s %s, order_s %s"
        % (last.templates, last.dup_frag_templates, med(res), med(keys), med(order)))


def part_e2e(a):
    import synth
    contigs = [("chr%d" % (i + 1), int(float(a.genome) * 1e6 / 4)) for i in range(4)]
    codes, names, lengths = synth.genome(contigs, config_id=1)
    d = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    fa = os.path.join(d, "ref.fa")
    with open(fa, "wb") as f:
        off = 0
        for nm, L in zip(names, lengths):
            f.write(b">%s\n" % nm.encode() + synth.SYM[codes[off:off + L]].tobytes() + b"\n")
            off += L
    rng = np.random.default_rng(3)
    P, m, frag = a.pairs, 100, 300
    offs = np.concatenate([[0], np.cumsum(lengths)])
    ci = rng.integers(0, 4, P)
    start = offs[ci] + rng.integers(0, np.array(lengths)[ci] - frag - 1)
    copies = np.arange(10, P, 10)
    start[copies] = start[rng.integers(0, copies, len(copies))]
    idx = start[:, None] + np.arange(m)[None, :]
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    m1 = synth.SYM[codes[idx]]
    m2 = synth.SYM[comp[codes[idx + (frag - m)]][:, ::-1]]
    fqs = [os.path.join(d, "m_1.fq"), os.path.join(d, "m_2.fq")]
    for path, mates in zip(fqs, (m1, m2)):
        q = (rng.integers(2, 42, (P, m), dtype=np.uint8) + 33)
        with open(path, "wb") as f:
            for c0 in range(0, P, 1 << 17):
                f.write(b"".join(b"@p%08d\n%s\n+\n%s\n" % (i, mates[i].tobytes(), q[i].tobytes()) for i in range(c0, min(P, c0 + (1 << 17)))))
    del m1, m2, idx, codes
    cli = [sys.executable, os.path.join(REPO, "genome-weaver-align_amd", "gwa_cli.py")]
    subprocess.run(cli + ["bwt", fa], check=True, stderr=subprocess.DEVNULL)
    kinds = [("--sort --index", [], None), ("--sort --index --markdup", ["--markdup"], None)]
    if a.parent_lib:
        kinds.append(("--sort --index, parent library", [], a.parent_lib))
    wall = {k[0]: [] for k in kinds}
    for rnd in range(a.rounds + 1):
        for kind, flags, lib in kinds:
            env = dict(os.environ)
            if lib:
                env["GWA_LIB"] = lib
            out = os.path.join(d, "out.bam")
            t0 = time.time()
            p = subprocess.run(cli + ["align", "-r", fa, "-k", "2", "--timing", "--bam", "--sort", "--index", "-o", out] + flags + fqs,
                               stderr=subprocess.PIPE, env=env)
            if p.returncode != 0:
                print(p.stderr.decode())
                sys.exit(p.returncode)
            err = p.stderr.decode()
            secs = float(re.search(r"align \(read file -> SAM, index load excluded\) (\d+\.\d+)s", err).group(1))
            lines = [l[len("[gwa] "):] for l in err.splitlines() if l.startswith("[gwa] sort:") or l.startswith("[gwa] markdup:")]
            if rnd:
                wall[kind].append(secs)
            say("round %d%s %-32s align %.2fs (process %.1fs), %d bytes; %s"
                % (rnd, "" if rnd else " (untimed)", kind, secs, time.time() - t0, os.path.getsize(out), "; ".join(lines)))
    for kind, _, _ in kinds:
        say("e2e %-32s align seconds %s" % (kind, med(wall[kind])))
    for p in fqs + [fa, fa + ".gwa.idx", os.path.join(d, "out.bam"), os.path.join(d, "out.bam.bai")]:
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,resolve,e2e")
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--genome", default="50")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    parts = a.part.split(",")
    if "kernel" in parts or "resolve" in parts:
        import gwa
        if "kernel" in parts:
            part_kernel(a, gwa)
        if "resolve" in parts:
            part_resolve(a, gwa)
    if "e2e" in parts:
        part_e2e(a)


if __name__ == "__main__":
    main()
