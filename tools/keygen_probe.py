"""Wall time of keygen on the sgx-shaped circuit at a chosen k, the two routes alternating on the same box:

  keygen()            plonk/keygen.py: identity columns transformed on the device, DOWNLOADED, sigma gathered on the host, UPLOADED, committed; then the key's forms
  native              plonk.keygen_vk_native (zk_plonk_keygen_vk: mapping check + sigma from the copy mapping on the device, one commitment batch) +
                      plonk.NativeKey.from_keygen (zk_plonk_keygen_pk on the resident columns)

and the time of the two new kernels by the library's HIP-event timers ("keygen_mapping_check", "keygen_sigma").  One-time work per circuit: the figure of interest
is the removed host round trip, not a rate.  Both routes end with the same verifying key (asserted).

    python tools/keygen_probe.py [--k 19] [--reps 3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import zk_dcap_verifier_amd as z  # noqa: E402
from zk_dcap_verifier_amd import plonk  # noqa: E402
import sgx_shaped_circuit as sgx  # noqa: E402

TAU = 0x1C59A59B6CFF4308740943526ADE1D8C09F71B337A67269CC89586BCDD6DFCBA % z.fields.R_MOD
KERNELS = ("keygen_mapping_check", "keygen_sigma")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=19)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    be = z.Backend(0)
    k = args.k
    t0 = time.time()
    cs, fixed, asm, _advice = sgx.build(z, be, k, census="chip_estimate")
    params = z.kzg.ParamsKZG.setup(k, TAU, backend=be)
    print(f"[k={k}] circuit and SRS in {time.time() - t0:.1f} s: {cs.num_fixed_columns} fixed, {len(cs.permutation_columns)} permutation columns", flush=True)
    rows = []
    for rep in range(args.reps):
        t = time.time()
        pk = plonk.keygen(params, cs, fixed, asm)
        be.sync()
        old_ms = (time.time() - t) * 1e3
        want = (pk.vk.fixed_commitments, pk.vk.permutation_commitments, pk.vk.transcript_repr)
        pk.release()
        be.timing(True)
        t = time.time()
        vk, kg = plonk.keygen_vk_native(params, cs, fixed, asm)
        be.sync()
        vk_ms = (time.time() - t) * 1e3
        t = time.time()
        key = plonk.NativeKey.from_keygen(params, kg, vk)
        be.sync()
        pk_ms = (time.time() - t) * 1e3
        kernels = {name: be.timing_get(name)[0] for name in KERNELS}
        be.timing(False)
        assert (vk.fixed_commitments, vk.permutation_commitments, vk.transcript_repr) == want, "the two routes disagree on the verifying key"
        kg.release()
        key.release()
        row = {"k": k, "rep": rep, "keygen_ms": round(old_ms, 1), "native_vk_ms": round(vk_ms, 1), "native_pk_ms": round(pk_ms, 1),
               "native_ms": round(vk_ms + pk_ms, 1), **{name + "_ms": None if v is None else round(v, 3) for name, v in kernels.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"version": be.version(), "rows": rows}, f, indent=1)
    params.release()
    be.close()


if __name__ == "__main__":
    main()
