"""Wall time of one zk_mock_prover_verify (plonk.dev.NativeMockProver) on the sgx-shaped circuit, split into its passes by the library's HIP-event timers
(zk_timing_enable): copies (gather-compare + compaction), gates (detection over 2^k rows + compaction), gate_rows (attribution on the failing rows), lookups
(compression, table sorts, searches, compaction).  A satisfied witness, then one with a gate, a lookup and a copy cell corrupted.

    python tools/mock_prover_probe.py [--k 19] [--full-chain]      (--full-chain: the full_chain_x4 census at k = 21 as well)
    python tools/mock_prover_probe.py --session 20 [--k 19] [--full-chain]
--session N: the same columns through a session (plonk.dev.NativeMockSession: zk_mock_prover_open once, N x zk_mock_prover_check) beside the one-shot call, in the
same process: wall time of open, per-check wall time and pass timers, and the copy edges the handle keeps against the cells of the mapping.
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
from zk_dcap_verifier_amd.plonk.dev import NativeMockProver, NativeMockSession  # noqa: E402
import sgx_shaped_circuit as sgx  # noqa: E402

PASSES = ("mock_copies", "mock_gates", "mock_gate_rows", "mock_lookups")
SESSION_PASSES = ("mock_copy_edges", "mock_gates", "mock_gate_rows", "mock_lookups")


def probe(be, k, census, reps=3, session=0):
    t0 = time.time()
    cs, fixed, asm, advice = sgx.build(z, be, k, census=census)
    print(f"[{census} k={k}] circuit built in {time.time() - t0:.1f} s: {len(cs.gates)} gate polynomials, {len(cs.lookups)} lookups, "
          f"{len(cs.permutation_columns)} permutation columns", flush=True)
    dfix = [be.to_device(np.ascontiguousarray(c)) for c in fixed]
    ses = None
    if session:
        be.timing(True)
        t = time.time()
        ses = NativeMockSession(k, cs, dfix, asm, backend=be)
        wall = (time.time() - t) * 1e3
        info = ses.info
        print(f"  session open: {wall:8.1f} ms wall (blobs compiled in Python included), mock_open {be.timing_get('mock_open')[0]:.2f} ms; {info['n_edges']} copy edges of "
              f"{info['n_cells']} cells ({100.0 * info['n_edges'] / max(1, info['n_cells']):.1f} %), {info['n_resident_tables']} of {info['n_tables']} tables resident, "
              f"{info['n_programs']} programs, {info['device_bytes'] / 2**20:.1f} MiB held", flush=True)
        be.timing(False)
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
        if ses is not None:
            walls, sums = [], []
            for rep in range(session):
                be.timing(True)
                t = time.time()
                ses.check(dadv, [], cap=0)
                walls.append((time.time() - t) * 1e3)
                split = {p: be.timing_get(p)[0] or 0.0 for p in SESSION_PASSES}
                be.timing(False)
                sums.append(sum(split.values()))
            print(f"  {label:18s} session, {session} checks: wall min {min(walls):.2f} / median {sorted(walls)[len(walls) // 2]:.2f} / first {walls[0]:.2f} ms, counts {ses.counts}; "
                  f"kernel sum median {sorted(sums)[len(sums) // 2]:.2f} ms; last check: " + ", ".join(f"{p[5:]} {v:.2f} ms" for p, v in split.items()), flush=True)
        for d in dadv:
            d.free()
    if ses is not None:
        ses.close()
    for d in dfix:
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=19)
    ap.add_argument("--full-chain", action="store_true")
    ap.add_argument("--session", type=int, default=0, metavar="N", help="also open a session and run N checks per witness")
    a = ap.parse_args()
    be = z.Backend(0)
    print(be.version(), flush=True)
    probe(be, a.k, "chip_estimate", session=a.session)
    if a.full_chain:
        probe(be, 21, "full_chain_x4", reps=2, session=a.session)
    be.close()


if __name__ == "__main__":
    main()
