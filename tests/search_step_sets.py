"""The read sets of tests/test_hostcore_search_steps.py (CPU) and tests/test_gpu_search_steps.py (GPU)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import synth  # noqa: E402

SETS = {
    # C2: 100 bp, 0-2 substitutions, -k 2 (1.5 verifications per read)
    "c2": dict(n=2000, m=100, k=2.0, kw=dict(config_id=2)),
    # C4: 150 bp, up to 5 edits with indels, -k 5 (10 verifications per read, split chains)
    "c4": dict(n=400, m=150, k=5.0, kw=dict(config_id=4, indels=True, max_edits=5)),
}


def genome():
    return synth.genome([("c%d" % (i + 1), 2000000) for i in range(4)], 1)


def reads_of(codes, lengths, name):
    s = SETS[name]
    seqs, rn = synth.reads(codes, lengths, s["n"], s["m"], 2, **s["kw"])
    strs = synth.to_strings(seqs)
    return [(rn[i], strs[i], "I" * s["m"]) for i in range(len(strs))], s["k"]
