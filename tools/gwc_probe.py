#!/usr/bin/env python3
"""GPU-box probe of the GWC multi-open (zk_plonk_multiopen_set, csrc/prover.hip gwc_create_proof) on the sgx-shaped synthetic circuit, k = 19 by default.  Two
measurements, each as alternating pairs on one box, wall clock around calls that end in a device synchronise; prints one JSON line (and writes it to the file given):

  proofs      one native proof alone, GWC then SHPLONK, `pairs` times after a warm-up of both: ms per proof, ms of the multi-open phase (zk_plonk_last_phase_ms[8]),
              the number of opening points P and the proof bytes.  A report, no threshold: GWC commits P - 2 more columns of 2^k coefficients by construction.
  multiopen   the GWC phase on the proof's own query shape (group sizes from the constraint system, uniform polynomials of 2^k coefficients): the batched path — one
              zk_fr_lincomb_batch_dev, one zk_kate_division_batch_dev — against the same phase composed from the single calls, P x zk_fr_lincomb_dev and
              P x zk_kate_division_dev, as plonk/gwc.py composes it; both end in the same MSM batch of the P witness columns, timed apart.  Outputs are compared first.
Usage: gwc_probe.py [k] [pairs] [reps] [out.json]   (defaults 19 3 5).  Timing only: the proofs are VERIFIED by tests/test_gwc.py."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, fr_mont_array, rand_fr_array
import sgx_shaped_circuit as sc

TAU = 0x1C59A59B6CFF4308740943526ADE1D8C09F71B337A67269CC89586BCDD6DFCBA


def group_sizes(cs):
    """queries per opening point, groups in order of first appearance: the multi-open order of one circuit with the points named by their rotation"""
    bf = cs.blinding_factors()
    chunk = cs.permutation_chunk_len()
    n_sets = -(-len(cs.permutation_columns) // chunk) if cs.permutation_columns else 0
    rots = [r for _, r in cs.advice_queries()]
    rots += [0, 1] * n_sets + [-(bf + 1)] * max(n_sets - 1, 0)
    rots += [0, 0, 0, -1, 1] * len(cs.lookups)
    rots += [r for _, r in cs.fixed_queries()] + [0] * len(cs.permutation_columns) + [0, 0]
    order = list(dict.fromkeys(rots))
    return [rots.count(r) for r in order]


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 19
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    n = 1 << k
    be = z.Backend(0)
    cs, fixed, asm, advice = sc.build(z, be, k)
    params = z.kzg.ParamsKZG.setup(k, TAU, backend=be)
    pk = plonk.keygen(params, cs, fixed, asm)
    provers = {s: plonk.NativeProver(params, pk, multiopen=s) for s in ("gwc", "shplonk")}
    out = {"k": k, "pairs": pairs, "reps": reps, "version": be.version(), "group_sizes": group_sizes(cs), "proofs": {"gwc": [], "shplonk": []}}
    proofs = {}
    for s, pr in provers.items():                                      # warm-up: workspaces, pools, code objects of both paths
        proofs[s] = pr.create_proof([a.copy() for a in advice], [], np.random.default_rng(1))
    unit = 32
    out["P"] = (len(proofs["gwc"]) - len(proofs["shplonk"])) // unit + 2
    assert out["P"] == len(out["group_sizes"]), (out["P"], out["group_sizes"])
    out["proof_bytes"] = {s: len(b) for s, b in proofs.items()}
    for i in range(pairs):
        for s in ("gwc", "shplonk"):
            cols = [a.copy() for a in advice]
            t = time.perf_counter()
            provers[s].create_proof(cols, [], np.random.default_rng(2 + i))
            ms = (time.perf_counter() - t) * 1e3
            out["proofs"][s].append({"ms": round(ms, 2), "multiopen_ms": provers[s].phase_ms["9_shplonk"]})
    pk.release()

    # ---- the phase alone: batched against composed from single calls -------------------------------------------------------------------------------------------
    sizes = out["group_sizes"]
    P = len(sizes)
    rng = np.random.default_rng(9)
    pool = [be.to_device(rand_fr_array(rng, n)) for _ in range(max(sizes))]            # the lists share polynomials, as a proof's do
    lists = [pool[:s] for s in sizes]
    v = rand_fr_array(rng, 1)
    vi = fr_int_array(v)[0]
    scal = [fr_mont_array([pow(vi, j, R_MOD) for j in range(s)]) for s in sizes]
    pts = rand_fr_array(rng, P)
    B = [be.alloc(n * 32) for _ in range(P)]
    W = {"batched": [be.alloc(n * 32) for _ in range(P)], "composed": [be.alloc(n * 32) for _ in range(P)]}

    def batched():
        be.fr_lincomb_batch_dev(lists, scal, n, B)
        be.kate_division_batch_dev(B, n, pts, W["batched"])
        for w in W["batched"]:
            w.zero((n - 1) * 32, 32)

    def composed():
        for i in range(P):
            be.fr_lincomb_dev(lists[i], scal[i], n, B[0])
            be.kate_division_dev(B[0], n, pts[i], W["composed"][i])
            W["composed"][i].zero((n - 1) * 32, 32)
    run = {"batched": batched, "composed": composed}
    for f in run.values():
        f()
    for a, b in zip(W["batched"], W["composed"]):
        assert (a.download((n, 4)) == b.download((n, 4))).all(), "the two compositions disagree"
    out["multiopen"] = {"batched": [], "composed": [], "commit_ms": []}
    for i in range(pairs):
        for name in ("batched", "composed"):
            be.sync()
            t = time.perf_counter()
            for _ in range(reps):
                run[name]()
            be.sync()
            out["multiopen"][name].append(round((time.perf_counter() - t) * 1e3 / reps, 3))
        t = time.perf_counter()
        params.commit_columns("g", W["batched"])
        out["multiopen"]["commit_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(line + "\n")
    os._exit(0)                                         # (the key and the context go with the process)


if __name__ == "__main__":
    main()
