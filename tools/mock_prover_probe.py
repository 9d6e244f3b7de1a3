"""Wall time of one zk_mock_prover_verify (plonk.dev.NativeMockProver) on the sgx-shaped circuit, split into its passes by the library's HIP-event timers
(zk_timing_enable): copies (gather-compare + compaction), gates (detection over 2^k rows + compaction), gate_rows (attribution on the failing rows), lookups
(compression, table sorts, searches, compaction).  A satisfied witness, then one with a gate, a lookup and a copy cell corrupted.

    python tools/mock_prover_probe.py [--k 19] [--full-chain]      (--full-chain: the full_chain_x4 census at k = 21 as well)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import zk_dcap_verifier_amd as z  # noqa: E402
from zk_dcap_verifier_amd.fields import R_MOD, fr_mont  # noqa: E402
from zk_dcap_verifier_amd.plonk.dev import NativeMockProver  # noqa: E402
import sgx_shaped_circuit as sgx  # noqa: E402

PASSES = ("mock_copies", "mock_gates", "mock_gate_rows", "mock_lookups")


def probe(be, k, census, reps=3):
    t0 = time.time()
    cs, fixed, asm, advice = sgx.build(z, be, k, census=census)
    print(f"[{census} k={k}] circuit built in {time.time() - t0:.1f} s: {len(cs.gates)} gate polynomials, {len(cs.lookups)} lookups, "
          f"{len(cs.permutation_columns)} permutation columns", flush=True)
    dfix = [be.to_device(np.ascontiguousarray(c)) for c in fixed]
    for label, adv in (("satisfied", advice), ("3 corrupted cells", None)):
        if adv is None:
            adv = [np.ascontiguousarray(c).copy() for c in advice]
            adv[3][4 * 20 + 3] = fr_mont(R_MOD - 1)
            sel = sgx.N_TABLE_COLS + 2 % (len(fixed) - sgx.N_TABLE_COLS)                       # lookup 2's selector: on at the first row of every other block
            row = next(4 * b for b in range(100, 2000) if fixed[sel][4 * b].any())
            adv[len(advice) - len(cs.lookups) + 2][row] = fr_mont(1 << 16)
            adv[6][4 * 25 + 1] = fr_mont(12345)
        dadv = [be.to_device(np.ascontiguousarray(c)) for c in adv]
        for rep in range(reps):
            nm = NativeMockProver.run(k, cs, dfix, dadv, [], asm, backend=be)
            be.timing(True)
            t = time.time()
            counts = nm.counts
            wall = (time.time() - t) * 1e3
            split = {p: be.timing_get(p)[0] for p in PASSES}
            be.timing(False)
            print(f"  {label:18s} rep {rep}: {wall:8.1f} ms wall (device-resident columns), counts {counts}; passes: " +
                  ", ".join(f"{p[5:]} {v:.2f} ms" for p, v in split.items() if v is not None), flush=True)
        for d in dadv:
            d.free()
    for d in dfix:
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=19)
    ap.add_argument("--full-chain", action="store_true")
    a = ap.parse_args()
    be = z.Backend(0)
    print(be.version(), flush=True)
    probe(be, a.k, "chip_estimate")
    if a.full_chain:
        probe(be, 21, "full_chain_x4", reps=2)
    be.close()


if __name__ == "__main__":
    main()
