#!/usr/bin/env python3
"""GPU-box probe: one proof over m circuits (NativeProver.create_proof_multi, zk_plonk_create_proof_multi) against single-circuit proofs, on the sgx-shaped synthetic
circuit (tools/sgx_shaped_circuit.py) at k = 19 by default.  Prints one JSON line:
  multi[m]        m-circuit proofs one after another on one context: seconds per proof, circuit instances per hour (proofs/hour x m), proof bytes
  single_x4       single-circuit proofs, four in flight (one context + host thread each, one shared key): circuit instances per hour
Usage: multi_circuit_probe.py [k] [reps] [m ...]   (defaults 19 2 1 2 4).  Timing only: the m-circuit proofs are VERIFIED by tests/test_multi_circuit.py."""
import json, os, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
import sgx_shaped_circuit as sc

TAU = 0x1C59A59B6CFF4308740943526ADE1D8C09F71B337A67269CC89586BCDD6DFCBA


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 19
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    ms = [int(v) for v in sys.argv[3:]] or [1, 2, 4]
    be = z.Backend(0)
    cs, fixed, asm, advice = sc.build(z, be, k)
    params = z.kzg.ParamsKZG.setup(k, TAU, backend=be)
    pk = plonk.keygen(params, cs, fixed, asm)
    native = plonk.NativeProver(params, pk)
    out = {"k": k, "reps": reps, "multi": {}}
    native.create_proof([a.copy() for a in advice], [], np.random.default_rng(1))          # warm-up: workspaces, pools
    for m in ms:
        advices = [[a.copy() for a in advice] for _ in range(m)]
        proof = native.create_proof_multi(advices, [[] for _ in range(m)], np.random.default_rng(2))    # (warm-up of this m's buffer sizes)
        t = time.time()
        for r in range(reps):
            native.create_proof_multi([[a.copy() for a in adv] for adv in advices], [[] for _ in range(m)], np.random.default_rng(3 + r))
        dt = (time.time() - t) / reps
        out["multi"][m] = {"s_per_proof": round(dt, 3), "proofs_per_hour": round(3600 / dt, 1), "instances_per_hour": round(3600 * m / dt, 1), "proof_bytes": len(proof),
                           "phase_ms": native.phase_ms}
        print(json.dumps({"m": m, **out["multi"][m]}), file=sys.stderr, flush=True)
    # four single-circuit proofs in flight: one context and host thread each, the key shared (the bench's throughput mode)
    n_fl = 4
    bes = [be] + [z.Backend(0) for _ in range(n_fl - 1)]
    prs = [native]
    for b in bes[1:]:
        p_ = z.kzg.ParamsKZG.shared_with(params, b)
        prs.append(plonk.NativeProver(p_, plonk.ProvingKey.shared_with(pk, b)))
    for pr in prs[1:]:
        pr.create_proof([a.copy() for a in advice], [], np.random.default_rng(1))
    per = max(reps, 2)
    errs = []

    def work(pr, i):
        try:
            for r in range(per):
                pr.create_proof([a.copy() for a in advice], [], np.random.default_rng(100 * i + r))
        except BaseException as e:
            errs.append(e)
    ts = [threading.Thread(target=work, args=(pr, i)) for i, pr in enumerate(prs)]
    t = time.time()
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    dt = time.time() - t
    if errs:
        raise errs[0]
    out["single_x4"] = {"proofs": n_fl * per, "seconds": round(dt, 3), "instances_per_hour": round(3600 * n_fl * per / dt, 1)}
    print(json.dumps(out))
    os._exit(0)                                         # (the shared keys and contexts go with the process)


if __name__ == "__main__":
    main()
