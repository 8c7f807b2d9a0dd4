"""BGZF read file -> SAM through the CLI, this build against the zlib path (BGZF input; GPU box;
writes under $TMPDIR): a synthetic genome saved as an index by `bwt`, N 100 bp reads with skewed qualities
written once from a seed as plain FASTQ and as BGZF (gwa.bgzf_compress on the device, plus the EOF marker).
`align --timing --warm-passes 2` (the timed pass only) runs `--rounds` times each, alternating, on

  base   --parent-cli PATH: the gwa_cli.py of another build (the parent commit's, built in its own tree);
         without it this build with GWA_BGZF_INPUT=0 (the same zlib reader)
  bgzf   this build, the file inflated on the device

then once on the plain file (the ceiling).  Prints each run's reads/s and stage lines, the verdict (bgzf beats
base by more than the larger of the two spreads), whether the SAM files are equal byte for byte, and the
kernel alone: HIP events around inflate_block_kernel over the first --kernel-mb MB of the compressed file
resident in HBM, against the memory floor (compressed bytes read + text written, at the measured HBM rate).

  python tools/bgzf_input_e2e.py [--genome <Mbp>] [--reads N] [--rounds K] [--parent-cli PATH]
"""
import argparse
import filecmp
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tools"), os.path.join(REPO, "genome-weaver-align_amd")]
HBM_MEASURED = 6.29e12  # bytes/s, float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="50")
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-mb", type=int, default=64)
    ap.add_argument("--parent-cli", default=None)
    a = ap.parse_args()
    import numpy as np
    import gwa
    import synth
    contigs = [("chr%d" % (i + 1), int(float(a.genome) * 1e6 / 4)) for i in range(4)]
    codes, names, lengths = synth.genome(contigs, config_id=1)
    d = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    fa, fq, fz = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "reads.fq.gz")
    t0 = time.time()
    with open(fa, "wb") as f:
        off = 0
        for nm, L in zip(names, lengths):
            f.write(b">%s\n" % nm.encode())
            rows = (L + 59) // 60  # 60 bases a line
            flat = np.full(rows * 60, ord("A"), dtype=np.uint8)
            flat[:L] = synth.SYM[codes[off:off + L]]
            blk = np.full((rows, 61), ord("\n"), dtype=np.uint8)
            blk[:, :60] = flat.reshape(rows, 60)
            data = blk.tobytes()
            tail = rows * 60 - L  # drop the padding of the last line, keep its newline
            f.write(data[:len(data) - 1 - tail] + b"\n" if tail else data)
            off += L
    m = 100
    sb = synth.SYM[synth.reads_codes(codes, lengths, a.reads, m, 2, config_id=2)]
    rng = np.random.default_rng(7)
    w = np.array([2.0 ** (12 - k) for k in range(13)])
    qa = np.frombuffer(b"IHGFEDCBA@?>=", dtype=np.uint8)
    with open(fq, "wb") as f, open(fz, "wb") as z:
        for c0 in range(0, a.reads, 1 << 18):
            c1 = min(a.reads, c0 + (1 << 18))
            q = qa[rng.choice(13, size=(c1 - c0, m), p=w / w.sum())]
            text = b"".join(b"@r%09d\n%s\n+\n%s\n" % (i, sb[i].tobytes(), q[i - c0].tobytes()) for i in range(c0, c1))
            f.write(text)
            z.write(gwa.bgzf_compress(text, device=0))  # (each piece its own run of blocks)
        z.write(gwa.BGZF_EOF)
    del sb, codes
    print("[bgzf_in] inputs written in %.1fs: %.3f GB of FASTQ, %.3f GB as BGZF" % (time.time() - t0, os.path.getsize(fq) / 1e9,
                                                                                 os.path.getsize(fz) / 1e9), flush=True)
    cli = [sys.executable, os.path.join(REPO, "genome-weaver-align_amd", "gwa_cli.py")]
    subprocess.run(cli + ["bwt", fa], check=True, stderr=subprocess.DEVNULL)
    base_cli = [sys.executable, a.parent_cli] if a.parent_cli else cli
    base_env = dict(os.environ) if a.parent_cli else dict(os.environ, GWA_BGZF_INPUT="0")
    runs = {"base": (base_cli, base_env, fz), "bgzf": (cli, dict(os.environ), fz)}
    outs = {k: os.path.join(d, "out_%s.sam" % k) for k in ("base", "bgzf", "plain")}
    rates = {k: [] for k in runs}

    def one(kind, c, env, path):
        r = subprocess.run(c + ["align", "-r", fa, "-k", "2", "--timing", "--warm-passes", "2", "-o", outs[kind], path],
                           stderr=subprocess.PIPE, text=True, env=env)
        if r.returncode != 0:
            print(r.stderr)
            sys.exit(r.returncode)
        rate = int(re.search(r"after it (\d+) reads/s", r.stderr).group(1))
        pl = [l for l in r.stderr.splitlines() if l.startswith("[gwa] pipeline") or l.startswith("[gwa] BGZF")]
        rd = re.search(r"read ([0-9.]+)s", pl[0]) if pl else None
        inf = re.search(r"inflate ([0-9.]+)s", pl[-1]) if len(pl) > 1 else None
        print("[bgzf_in] %-5s %6.2f M reads/s, read_s %s, inflate_s %s" % (kind, rate / 1e6, rd.group(1) if rd else "?",
                                                                          inf.group(1) if inf else "-"), flush=True)
        return rate

    for rnd in range(a.rounds):
        for kind, (c, env, path) in runs.items():
            rates[kind].append(one(kind, c, env, path))
    one("plain", cli, dict(os.environ), fq)
    spread = {k: max(v) - min(v) for k, v in rates.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    for k in runs:
        print("[bgzf_in] %-5s median %.2f M reads/s, spread (max - min) %.2f M" % (k, med[k] / 1e6, spread[k] / 1e6))
    gain = min(rates["bgzf"]) - max(rates["base"])
    print("[bgzf_in] slowest bgzf run - fastest base run = %.2f M reads/s; medians differ by %.2f M, larger spread %.2f M: %s"
          % (gain / 1e6, (med["bgzf"] - med["base"]) / 1e6, max(spread.values()) / 1e6,
             "bgzf wins" if med["bgzf"] - med["base"] > max(spread.values()) else "no win"))
    print("[bgzf_in] SAM base == bgzf: %s; bgzf == plain: %s" % (filecmp.cmp(outs["base"], outs["bgzf"], shallow=False),
                                                                 filecmp.cmp(outs["bgzf"], outs["plain"], shallow=False)))
    # the kernel alone
    data = open(fz, "rb").read(a.kernel_mb << 20)
    at = 0
    while at + 18 <= len(data):
        size = int.from_bytes(data[at + 16:at + 18], "little") + 1
        if at + size > len(data):
            break
        at += size
    data = data[:at]
    for rep in range(3):
        n, ms = gwa.bgzf_decompress_timed(data, device=0, repeat=3)
        floor = (len(data) + n) / HBM_MEASURED * 1e3
        print("[bgzf_in] kernel: %d compressed bytes -> %d text bytes in %.3f ms = %.1f GB/s of text; memory floor %.4f ms "
              "(%.0fx)" % (len(data), n, ms, n / ms / 1e6, floor, ms / floor), flush=True)
    for p in list(outs.values()) + [fa, fq, fz, fa + ".gwa.idx"]:
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(d)


if __name__ == "__main__":
    main()
