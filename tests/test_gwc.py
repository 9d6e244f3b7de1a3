"""Proofs that end with halo2's GWC multi-open (ProverGWC) instead of SHPLONK: zk_plonk_multiopen_set, csrc/prover.hip gwc_create_proof, plonk/gwc.py.

For every case of tests/gwc_cases.py (k = 6 .. 9: the toy and the sgx-shaped circuit, m = 2 and 3 circuits in one proof, a phased circuit, one opening point, eight
opening points, points whose first-appearance order is not the ascending one) and each of the three transcripts (Blake2b, Poseidon, EVM / Keccak):
  (a) every byte before the multi-open equals the SHPLONK proof of the same inputs and draws without its last two commitments — where the case has a committed golden
      (the independent CPU prover's SHPLONK proof, Blake2b), that SHPLONK proof is the golden;
  (b) the length is that prefix + P points, P the number of distinct opening points;
  (c) tests/gwc_verifier.py accepts: every W_i satisfies its own opening equation under the test's trapdoor, which determines W_i uniquely;
  (d) the Python twin (plonk.create_proof(.., multiopen="gwc"): P single combinations and P single divisions) emits the native prover's bytes (one batched combination,
      one batched division).  The twin proves one circuit: the m = 2 and m = 3 cases have no twin to compare, as for SHPLONK.
Then the verifier's own sanity (five tampered proofs, every one rejected), a context that alternates between the two arguments, every entry point, and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.plonk.keygen import NativeKey
from zk_dcap_verifier_amd.plonk.native import RNG_FN
from zk_dcap_verifier_amd.transcript import Blake2bWrite, EvmWrite, PoseidonWrite, point_to_bytes

import gwc_cases as gc
import proof_cases as pc
import test_create_proof as tcp

TRANSCRIPTS = ("blake2b", "poseidon", "evm")
WRITERS = {"blake2b": Blake2bWrite, "poseidon": PoseidonWrite, "evm": EvmWrite}
POINT_BYTES = {"blake2b": 32, "poseidon": 32, "evm": 64}
ZK_ERR_ARG, ZK_ERR_LIMIT = -1, -5


def _reader(transcript):
    import evm_ref
    import poseidon_ref
    return {"blake2b": None, "poseidon": poseidon_ref.Reader, "evm": evm_ref.Reader}[transcript]


def _setup(be, case):
    params = z.kzg.ParamsKZG.setup(case.k, gc.TAU, backend=be)
    return params, plonk.keygen(params, case.cs, case.fixed, case.asm)


def _native(be, case, params, pk, transcript, multiopen):
    """the native proof through the entry point the case calls for: zk_plonk_prove_phased on a key handle (phased), zk_plonk_create_proof_multi (m > 1), zk_plonk_create_proof"""
    if case.phased is not None:
        key = NativeKey(params, pk, transcript=TRANSCRIPTS.index(transcript))
        try:
            return plonk.PhasedProver(params, pk, key=key, multiopen=multiopen).create_proof(case.host_advices(), case.instances_list, case.rng(), case.phased.next_phase())
        finally:
            key.release()
    prover = plonk.NativeProver(params, pk, transcript=transcript, multiopen=multiopen)
    if case.m > 1:
        return prover.create_proof_multi(case.host_advices(), case.instances_list, case.rng())
    return prover.create_proof(case.host_advices()[0], case.instances_list[0], case.rng())


def _twin(case, params, pk, transcript):
    tr = WRITERS[transcript]()
    info = plonk.create_proof(params, pk, case.host_advices()[0], case.instances_list[0], case.rng(), tr,
                              next_phase=case.phased.next_phase() if case.phased is not None else None, multiopen="gwc")
    return tr.finalize(), info


def _check_case(be, name):
    import gwc_verifier as gv
    case = gc.CASES[name](be)
    params, pk = _setup(be, case)
    try:
        for transcript in TRANSCRIPTS:
            pt = POINT_BYTES[transcript]
            shplonk = _native(be, case, params, pk, transcript, "shplonk")
            if case.golden and transcript == "blake2b":
                assert shplonk == tcp._golden(case.golden), (name, "the SHPLONK proof of these draws is no longer the committed golden")
            gwc = _native(be, case, params, pk, transcript, "gwc")
            info = {}
            assert gv.verify_proof_gwc(pk.vk, gc.TAU, case.instances_list, gwc, reader=_reader(transcript), info=info) is True, (name, transcript)      # (c)
            P = len(info["points"])
            assert case.points is None or P == case.points, (name, transcript, P)
            assert case.min_points is None or P >= case.min_points, (name, transcript, P)
            prefix = len(shplonk) - 2 * pt
            assert info["witness_at"] == prefix and gwc[:prefix] == shplonk[:prefix], (name, transcript, pc.first_difference(gwc[:prefix], shplonk[:prefix]))   # (a)
            assert len(gwc) == prefix + P * pt, (name, transcript, len(gwc), prefix, P)                                               # (b)
            if name == "unsorted":
                assert info["points"] != sorted(info["points"]) and len(set(info["points"])) == P, "this x leaves the points in ascending order: the case separates nothing"
                assert info["sizes"][0] == 1, "the first group is the one query at omega^2 x"
            if case.m == 1:
                twin, twin_info = _twin(case, params, pk, transcript)
                assert twin == gwc, (name, transcript, "twin vs native", pc.first_difference(twin, gwc))                               # (d)
                assert twin_info["commitments"] * pt + twin_info["evals"] * 32 == len(gwc)
        assert be.multiopen_get() == "shplonk", "a prover with multiopen= must leave the context as it found it"
    finally:
        pk.release()
        params.release()


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_gwc_proofs_emulated(emu, orc, name):
    _check_case(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_gwc_proofs_gpu(gpu, orc, name):
    _check_case(gpu, name)


# ---- the verifier itself: what it must reject ---------------------------------------------------------------------------------------------------------------------------
def test_gwc_verifier_rejects_every_tampered_proof(emu, orc, pyref):
    import gwc_verifier as gv
    case = gc.toy()
    params, pk = _setup(emu, case)
    try:
        proof = _native(emu, case, params, pk, "blake2b", "gwc")
    finally:
        pk.release()
        params.release()
    info = {}
    assert gv.verify_proof_gwc(pk.vk, gc.TAU, case.instances_list, proof, info=info) is True
    at, P = info["witness_at"], len(info["points"])
    assert P >= 2 and len(proof) == at + 32 * P
    W = [proof[at + 32 * i: at + 32 * i + 32] for i in range(P)]
    assert len(set(W)) == P

    def rejected(bad):
        try:
            return gv.verify_proof_gwc(pk.vk, gc.TAU, case.instances_list, bytes(bad)) is False
        except ValueError:
            return True
    tampered = {}
    bad = bytearray(proof)
    bad[info["first_eval_at"]] ^= 1
    tampered["one evaluation changed"] = bad
    tampered["two W_i swapped"] = proof[:at] + W[1] + W[0] + b"".join(W[2:])
    generator = point_to_bytes(pyref.G1_GEN)
    assert generator not in W
    tampered["one W_i replaced by the generator"] = proof[:at] + b"".join(W[:-1]) + generator
    tampered["a trailing byte added"] = proof + b"\x00"
    tampered["the last point dropped"] = proof[:-32]
    assert len(tampered) == 5
    for what, bad in tampered.items():
        assert rejected(bad), what
    wrong = [[list(col) for col in inst] for inst in case.instances_list]
    wrong[0][0][1] = (wrong[0][0][1] + 1) % pyref.R
    assert gv.verify_proof_gwc(pk.vk, gc.TAU, wrong, proof) is False


# ---- the setting belongs to the context -----------------------------------------------------------------------------------------------------------------------------------
def _check_context_history(be):
    """GWC, SHPLONK, GWC, SHPLONK on one context, through provers that leave the setting alone: both SHPLONK proofs are the golden, both GWC proofs are equal"""
    import gwc_verifier as gv
    case = gc.toy()
    params, pk = _setup(be, case)
    prover = plonk.NativeProver(params, pk)
    assert be.multiopen_get() == "shplonk"                            # the default
    proofs, squeezed = [], []
    try:
        for scheme in ("gwc", "shplonk", "gwc", "shplonk"):
            be.multiopen_set(scheme)
            assert be.multiopen_get() == scheme
            proofs.append(prover.create_proof(case.host_advices()[0], case.instances_list[0], case.rng()))
            squeezed.append(plonk.last_challenges(be))
    finally:
        be.multiopen_set("shplonk")
        pk.release()
        params.release()
    assert proofs[1] == proofs[3] == tcp._golden(case.golden)
    assert proofs[0] == proofs[2] and proofs[0] != proofs[1]
    info = {}
    assert gv.verify_proof_gwc(pk.vk, gc.TAU, case.instances_list, proofs[0], info=info) is True
    # zk_plonk_last_challenges: theta, beta, gamma, y, x and then SHPLONK's y, v, u or GWC's v alone
    assert [len(s) for s in squeezed] == [6, 8, 6, 8] and squeezed[0][:5] == squeezed[1][:5] and squeezed[0][5] == info["v"]


def test_context_history_emulated(emu, orc):
    _check_context_history(emu)


@pytest.mark.gpu
def test_context_history_gpu(gpu, orc):
    _check_context_history(gpu)


def _by_key_handle(be, key, fn, case, cap):
    """zk_plonk_prove (fn = "zk_plonk_prove") or zk_plonk_prove_multi on a key handle, host columns"""
    from zk_dcap_verifier_amd.fields import rand_fr_array
    rng = case.rng()

    def draw(_user, count, out):
        a = rand_fr_array(rng, int(count))
        C.memmove(out, a.ctypes.data, a.nbytes)
    cb = RNG_FN(draw)
    keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in case.host_advices()[0]]
    adv = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    inst = [np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in col) or bytes(32), dtype=np.uint8).copy() for col in case.instances_list[0]]
    inst_ptrs = (C.c_void_p * max(1, len(inst)))(*[a.ctypes.data for a in inst])
    lens = (C.c_uint32 * max(1, len(inst)))(*[len(col) for col in case.instances_list[0]])
    out = np.empty(cap, dtype=np.uint8)
    ln = C.c_size_t()
    head = (be.ctx, C.c_uint64(key.handle)) + ((C.c_uint32(1),) if fn == "zk_plonk_prove_multi" else ())
    be._ck(getattr(be.lib, fn)(*head, adv, C.c_int(0), inst_ptrs, lens, cb, None, out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(ln)))
    return out[: ln.value].tobytes()


def _check_every_entry_point(be):
    """one setting, six entry points: zk_plonk_create_proof, _create_proof_multi (descriptors), zk_plonk_prove, _prove_multi, _prove_phased (key handles) emit the same GWC
    proof of the toy circuit (the sixth, a phased key through zk_plonk_prove_phased, is the phased_A case above)"""
    case = gc.toy()
    params, pk = _setup(be, case)
    key = NativeKey(params, pk)
    try:
        prover = plonk.NativeProver(params, pk, multiopen="gwc")
        want = prover.create_proof(case.host_advices()[0], case.instances_list[0], case.rng())
        assert prover.create_proof_multi(case.host_advices(), case.instances_list, case.rng()) == want
        assert plonk.PhasedProver(params, pk, key=key, multiopen="gwc").create_proof(case.host_advices(), case.instances_list, case.rng()) == want
        be.multiopen_set("gwc")
        try:
            for fn in ("zk_plonk_prove", "zk_plonk_prove_multi"):
                assert _by_key_handle(be, key, fn, case, prover.proof_cap) == want, fn
        finally:
            be.multiopen_set("shplonk")
    finally:
        key.release()
        pk.release()
        params.release()


def test_every_entry_point_emulated(emu, orc):
    _check_every_entry_point(emu)


@pytest.mark.gpu
def test_every_entry_point_gpu(gpu, orc):
    _check_every_entry_point(gpu)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_refusals(be):
    case = gc.toy()
    params, pk = _setup(be, case)
    native = plonk.NativeProver(params, pk)
    try:
        # any scheme but the two: ZK_ERR_ARG, the setting unchanged
        for before in ("shplonk", "gwc"):
            be.multiopen_set(before)
            for scheme in (2, 0xFFFFFFFF):
                with pytest.raises(z.ZkError) as e:
                    be.multiopen_set(scheme)
                assert e.value.code == ZK_ERR_ARG
                assert be.multiopen_get() == before
        assert be.lib.zk_plonk_multiopen_get(be.ctx, None) == ZK_ERR_ARG
        # proof_cap one byte short: ZK_ERR_LIMIT, the length reported, nothing written
        be.multiopen_set("gwc")
        whole = pc.RawCall(be, native, case.host_advices()[0], case.instances_list[0], case.rng())
        need = len(whole.proof)
        short = pc.RawCall(be, native, case.host_advices()[0], case.instances_list[0], case.rng(), cap=need - 1)
        assert short.rc == ZK_ERR_LIMIT and short.len == need and bool((short.out == pc.SENTINEL).all())
        exact = pc.RawCall(be, native, case.host_advices()[0], case.instances_list[0], case.rng(), cap=need)
        assert exact.proof == whole.proof
        # a sharded descriptor with GWC set: ZK_ERR_ARG that names the reason, before a draw is asked for or a byte written
        native.desc.shard_world, native.desc.shard_rank = 2, 0
        sharded = pc.RawCall(be, native, case.host_advices()[0], case.instances_list[0], case.rng())
        assert sharded.rc == ZK_ERR_ARG and "GWC" in sharded.error and "shard_world 2" in sharded.error, sharded.error
        assert sharded.untouched() and sharded.draw_calls == 0
        native.desc.shard_world = 0
        be.multiopen_set("shplonk")
        assert pc.RawCall(be, native, case.host_advices()[0], case.instances_list[0], case.rng()).proof == tcp._golden(case.golden)      # the context is as usable as before
    finally:
        native.desc.shard_world = 0
        be.multiopen_set("shplonk")
        pk.release()
        params.release()


def test_refusals_emulated(emu, orc):
    _check_refusals(emu)


@pytest.mark.gpu
def test_refusals_gpu(gpu, orc):
    _check_refusals(gpu)
