"""One halo2 proof over several circuit instances (zk_plonk_create_proof_multi / zk_plonk_prove_multi, NativeProver.create_proof_multi): halo2's
create_proof(params, pk, &[c0, c1, ..], &[inst0, inst1, ..], ..).  The proofs are checked by the test-side m-circuit verifier (multi_circuit_verifier.py), which
rejects them when any circuit's instance changes, when the circuits are swapped or when one circuit's witness violates a gate; m = 1 gives the single-circuit
goldens.  The accumulate mode of the quotient (zk_quotient_run_acc_dev: out <- out * y^E + numerator, halo2's fold across circuits) is pinned on its own."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, fr_mont, fr_mont_array, rand_fr_array

import multi_circuit_verifier as mv
import test_create_proof as tcp

ZK_ERR_ARG, ZK_ERR_LIMIT = -1, -5


# ---- circuits: one key, several witnesses ---------------------------------------------------------------------------------------------------------
def toy_witness(k, s=0, t=0, tamper=None):
    """a witness of tcp.toy_circuit(k) with its values shifted (a by s <= 7, b by t): the fixed columns and the copies stay those of the key"""
    n = 1 << k
    cs, _, _, _, _ = tcp.toy_circuit(k)
    u = cs.usable_rows(k)
    A = [(i % 8) + 1 + s for i in range(n)]                          # period 8 (a[0] == a[8], a[i + 1] = a[i] + 1 inside a block), inside the table 0 .. 15
    B = [((i // 2) % 5) + 2 + t for i in range(n)]
    Cc = [x * y % R_MOD for x, y in zip(A, B)]
    if tamper == "gate":
        Cc[5] = (Cc[5] + 1) % R_MOD
    if tamper == "lookup":                                           # as tcp.toy_circuit(tamper="lookup") but on this key's fixed columns: a value outside the table on a row the
        A[9], A[10] = 200, 201                                       # lookup reads (the rotation gate fails there too; the lookup is refused first)
        Cc[9], Cc[10] = A[9] * B[9] % R_MOD, A[10] * B[10] % R_MOD
    assert u > 8
    return [fr_mont_array(A), fr_mont_array(B), fr_mont_array(Cc)], [[Cc[0], Cc[3]]]


def graded_witness(k, s=0, t=0):
    """a witness of test_piece_cosets.graded_circuit(k, 1) (degree 4: the key keeps cosets 0 .. 2, the quotient runs by cosets with the degree split)"""
    n = 1 << k
    A = [(i % 8) + 1 + s for i in range(n)]
    B = [((i // 2) % 5) + 2 + t for i in range(n)]
    Cc = [x * y % R_MOD for x, y in zip(A, B)]
    return [fr_mont_array(A), fr_mont_array(B), fr_mont_array(Cc)], [[Cc[0]]]


def _sgx_module():
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    return sc


def sgx_circuits(be, k, m):
    """the sgx-shaped circuit with m witnesses on ONE key: the builder's seed draws the witness; when it also moved the fixed columns or the copies the circuits
    would not share a key, and then only the first witness is used (every circuit proves the same statement)"""
    sc = _sgx_module()
    cs, fixed, asm, advice = sc.build(z, be, k)
    advices = [advice]
    for i in range(1, m):
        cs_i, fixed_i, asm_i, advice_i = sc.build(z, be, k, seed=20241008 + 17 * i)
        same_key = len(fixed_i) == len(fixed) and all((a == b).all() for a, b in zip(fixed, fixed_i)) and getattr(asm_i, "copies", None) == getattr(asm, "copies", None)
        advices.append(advice_i if same_key else [a.copy() for a in advice])
    return cs, fixed, asm, advices


def _setup(be, k, cs, fixed, asm, **kw):
    params = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=be)
    pk = plonk.keygen(params, cs, fixed, asm, **kw)
    return params, pk, plonk.NativeProver(params, pk)


def _release(params, pk):
    pk.release()
    params.release()


# ---- proofs verify, and are one proof over all circuits ----------------------------------------------------------------------------------------------
def _toy_multi(be, k, m, seed=5):
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    params, pk, native = _setup(be, k, cs, fixed, asm)
    wit = [toy_witness(k, s=c, t=2 * c) for c in range(m)]
    advices, insts = [w[0] for w in wit], [w[1] for w in wit]
    proof = native.create_proof_multi([[a.copy() for a in adv] for adv in advices], insts, np.random.default_rng(seed))
    assert len(proof) == mv.proof_length(cs, m)
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, insts, proof) is True
    # the verifier holds the proof to every circuit's statement, in order
    bad_inst = [list(map(list, i)) for i in insts]
    bad_inst[m - 1][0][1] = (bad_inst[m - 1][0][1] + 1) % R_MOD
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, bad_inst, proof) is False
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [insts[1], insts[0]] + insts[2:], proof) is False
    # device-resident witnesses: the same bytes
    dev = [[be.to_device(a) for a in adv] for adv in advices]
    assert native.create_proof_multi(dev, insts, np.random.default_rng(seed)) == proof
    for adv in dev:
        for d in adv:
            d.free()
    _release(params, pk)
    return proof


@pytest.mark.parametrize("m", [2, 3])
def test_toy_circuits_in_one_proof_verify_emulated(emu, orc, m):
    _toy_multi(emu, 6, m)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 1])
def test_toy_circuits_in_one_proof_verify_gpu(gpu, orc, jit):
    gpu.tune(quot_jit=jit)
    try:
        _toy_multi(gpu, 8, 2)
        _toy_multi(gpu, 7, 3)
    finally:
        gpu.tune(quot_jit=0)


def _graded_multi(be, k, m, seed=9):
    """cs_degree 4: the key holds cosets 0 .. 2 and the quotient runs coset by coset (zk_coeff_to_coset_batch_dev + the degree split's parts on coset layout)"""
    import test_piece_cosets as tpc
    cs, fixed, asm, _, _ = tpc.graded_circuit(k, 1)
    params, pk, native = _setup(be, k, cs, fixed, asm)
    assert pk.pieces_from_cosets
    wit = [graded_witness(k, s=c, t=c + 1) for c in range(m)]
    proof = native.create_proof_multi([w[0] for w in wit], [w[1] for w in wit], np.random.default_rng(seed))
    assert len(proof) == mv.proof_length(cs, m)
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [w[1] for w in wit], proof) is True
    _release(params, pk)


def test_cosets_route_circuits_in_one_proof_verify_emulated(emu, orc):
    _graded_multi(emu, 5, 2)
    _graded_multi(emu, 5, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 1])
def test_cosets_route_circuits_in_one_proof_verify_gpu(gpu, orc, jit):
    gpu.tune(quot_jit=jit)
    try:
        _graded_multi(gpu, 10, 2)
    finally:
        gpu.tune(quot_jit=0)


def _sgx_multi(be, k, m, seed=3):
    cs, fixed, asm, advices = sgx_circuits(be, k, m)
    params, pk, native = _setup(be, k, cs, fixed, asm)
    assert not pk.pieces_from_cosets                                 # cs_degree 5: the extended route
    proof = native.create_proof_multi(advices, [[] for _ in range(m)], np.random.default_rng(seed))
    assert len(proof) == mv.proof_length(cs, m)
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [[] for _ in range(m)], proof) is True
    _release(params, pk)
    return proof


def test_sgx_shaped_circuits_in_one_proof_verify_emulated(emu, orc):
    _sgx_multi(emu, 8, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 1])
def test_sgx_shaped_circuits_in_one_proof_verify_gpu(gpu, orc, jit):
    gpu.tune(quot_jit=jit)
    try:
        _sgx_multi(gpu, 9, 2)
    finally:
        gpu.tune(quot_jit=0)


@pytest.mark.gpu
def test_sgx_shaped_circuits_in_one_proof_verify_k19_gpu(gpu, orc):
    _sgx_multi(gpu, 19, 2)


def test_one_circuit_is_the_golden_emulated(emu, orc):
    """zk_plonk_create_proof_multi over ONE circuit emits the independent CPU prover's bytes (tests/golden), as zk_plonk_create_proof does"""
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    params, pk, native = _setup(emu, 6, cs, fixed, asm)
    proof = native.create_proof_multi([[a.copy() for a in advice]], [instances], np.random.default_rng(7))
    assert proof == tcp._golden(tcp.GOLDEN_PROOF) and len(proof) == mv.proof_length(cs, 1)
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [instances], proof) is True
    _release(params, pk)
    sc = _sgx_module()
    cs, fixed, asm, advice = sc.build(z, emu, 8)
    params, pk, native = _setup(emu, 8, cs, fixed, asm)
    assert native.create_proof_multi([advice], [[]], np.random.default_rng(3)) == tcp._golden(tcp.GOLDEN_SGX)
    _release(params, pk)


@pytest.mark.gpu
def test_one_circuit_is_the_golden_gpu(gpu, orc):
    sc = _sgx_module()
    cs, fixed, asm, advice = sc.build(z, gpu, 8)
    params, pk, native = _setup(gpu, 8, cs, fixed, asm)
    assert native.create_proof_multi([advice], [[]], np.random.default_rng(3)) == tcp._golden(tcp.GOLDEN_SGX)
    _release(params, pk)


def test_a_circuit_that_violates_a_gate_is_rejected_emulated(emu, orc):
    """circuit 1 of 2 breaks a gate: the (halo2-byte) proof does not verify.  The key is built without the degree split, so the quotient is halo2's own evaluation"""
    emu.tune(quot_degree_split=0)
    try:
        k = 6
        cs, fixed, asm, _, _ = tcp.toy_circuit(k)
        params, pk, native = _setup(emu, k, cs, fixed, asm)
        assert emu.quotient_program_split(pk.evaluator.handle)["low_cosets"] == 0
        good, bad = toy_witness(k, s=1), toy_witness(k, s=2, tamper="gate")
        proof = native.create_proof_multi([good[0], bad[0]], [good[1], bad[1]], np.random.default_rng(4))
        assert mv.verify_proof_multi(pk.vk, tcp.TAU, [good[1], bad[1]], proof) is False
        _release(params, pk)
    finally:
        emu.tune(quot_degree_split=1)


# ---- draws -------------------------------------------------------------------------------------------------------------------------------------------
def test_draws_leave_the_callers_rng_where_halo2_would(emu, orc):
    """an m-circuit proof consumes halo2's m-circuit schedule block by block — per circuit its advice blinding rows and Blinds, then per circuit and lookup the permuted
    rows and Blinds, per circuit the permutation sets, per circuit the lookup products, the vanishing argument once — and nothing more"""
    k, m = 6, 3
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    params, pk, native = _setup(emu, k, cs, fixed, asm)
    wit = [toy_witness(k, s=c) for c in range(m)]
    rng = np.random.default_rng(21)
    native.create_proof_multi([w[0] for w in wit], [w[1] for w in wit], rng)
    n, bf, A, L = 1 << k, cs.blinding_factors(), cs.num_advice_columns, len(cs.lookups)
    chunk = cs.permutation_chunk_len()
    n_sets = -(-len(cs.permutation_columns) // chunk)
    blocks = []
    for _ in range(m):
        blocks += [bf + 1] * A + [1] * A
    blocks += [bf + 1, bf + 1, 1, 1] * (m * L)
    blocks += [bf, 1] * (m * n_sets)
    blocks += [bf, 1] * (m * L)
    blocks += [n] + [1] * cs.degree()                                # the random polynomial + its Blind, one Blind per h piece
    ref = np.random.default_rng(21)
    for b in blocks:
        rand_fr_array(ref, b)
    assert rng.integers(0, 1 << 62) == ref.integers(0, 1 << 62)
    _release(params, pk)


# ---- the side lane -----------------------------------------------------------------------------------------------------------------------------------
def _side_lane_multi(be, k):
    cs, fixed, asm, advices = sgx_circuits(be, k, 2)
    params, pk, native = _setup(be, k, cs, fixed, asm)
    proofs = []
    try:
        for mode in (2, 0):
            be.tune(prover_side_lane=mode)
            proofs.append(native.create_proof_multi(advices, [[], []], np.random.default_rng(3)))
    finally:
        be.tune(prover_side_lane=1)
    assert proofs[0] == proofs[1]
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [[], []], proofs[0]) is True
    _release(params, pk)


def test_side_lane_changes_no_byte_of_a_two_circuit_proof_emulated(emu, orc):
    _side_lane_multi(emu, 7)


@pytest.mark.gpu
def test_side_lane_changes_no_byte_of_a_two_circuit_proof_gpu(gpu, orc):
    _side_lane_multi(gpu, 12)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------
def _raw(be, native, m, advice_ptrs, inst_ptrs, lens, cap):
    cb = plonk.native.RNG_FN(lambda _u, count, out: C.memmove(out, rand_fr_array(np.random.default_rng(1), int(count)).ctypes.data, 32 * int(count)))
    out = np.zeros(max(cap, 1), np.uint8)
    ln = C.c_size_t()
    rc = be.lib.zk_plonk_create_proof_multi(be.ctx, C.byref(native.desc), C.c_uint32(m), advice_ptrs, C.c_int(0), inst_ptrs, lens, cb, None,
                                            out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(ln))
    return rc, ln.value


def test_errors_emulated(emu, orc):
    k = 5
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    params, pk, native = _setup(emu, k, cs, fixed, asm)
    w0, w1 = toy_witness(k), toy_witness(k, s=1)
    # m = 0
    adv = (C.c_void_p * 6)(*[a.ctypes.data for a in w0[0] + w1[0]])
    inst = [np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in col), np.uint8).copy() for col in (w0[1][0], w1[1][0])]
    inst_ptrs = (C.c_void_p * 2)(*[a.ctypes.data for a in inst])
    lens = (C.c_uint32 * 2)(2, 2)
    assert _raw(emu, native, 0, adv, inst_ptrs, lens, 1 << 16)[0] == ZK_ERR_ARG
    # a short output buffer: ZK_ERR_LIMIT, the needed length reported
    rc, need = _raw(emu, native, 2, adv, inst_ptrs, lens, 64)
    assert rc == ZK_ERR_LIMIT and need == mv.proof_length(cs, 2)
    assert _raw(emu, native, 2, adv, inst_ptrs, lens, need)[0] == 0
    # m > 1 on a sharded descriptor
    native.desc.shard_world, native.desc.shard_rank = 2, 0
    assert _raw(emu, native, 2, adv, inst_ptrs, lens, 1 << 16)[0] == ZK_ERR_ARG
    assert b"sharded" in emu.lib.zk_last_error(emu.ctx)
    native.desc.shard_world = 0
    # an unknown key handle
    ln = C.c_size_t()
    assert emu.lib.zk_plonk_prove_multi(emu.ctx, C.c_uint64(1 << 40), C.c_uint32(2), adv, C.c_int(0), inst_ptrs, lens, None, None, None, C.c_size_t(0), C.byref(ln)) == ZK_ERR_ARG
    # a lookup input outside its table in circuit 1 only: ZK_ERR_ARG as for one circuit (halo2's ConstraintSystemFailure)
    bad = toy_witness(k, s=1, tamper="lookup")
    with pytest.raises(z.ZkError) as e:
        native.create_proof_multi([w0[0], bad[0]], [w0[1], bad[1]], np.random.default_rng(1))
    assert e.value.code == ZK_ERR_ARG
    # and the context is fine afterwards
    proof = native.create_proof_multi([w0[0], w1[0]], [w0[1], w1[1]], np.random.default_rng(1))
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [w0[1], w1[1]], proof) is True
    _release(params, pk)


# ---- the accumulate mode of the quotient on its own ------------------------------------------------------------------------------------------------------
def _acc_kernel(be, k, circuit, seed, cancel=False, kind="uniform", orc=None):
    """for random columns, every route and part: zk_quotient_run_acc_dev gives prev * y^E + N, N from the non-accumulating entry point, prev random, E counted from
    the constraint system; checked with host big-int arithmetic.  cancel: one more accumulating run per route with prev = -N * y^(-E), which must leave exactly 0 (all limbs) on
    every row; kind: the columns are structured ones (parity_cases.structured_fr) instead of uniform"""
    cs, fixed, asm = circuit
    params, pk, _ = _setup(be, k, cs, fixed, asm, piece_cosets=False)
    prog = pk.evaluator.handle
    ek = pk.domain.extended_k
    size, n = 1 << ek, 1 << k
    E = mv.identities_per_circuit(cs)
    chunk = cs.permutation_chunk_len()
    n_sets = -(-len(cs.permutation_columns) // chunk)
    L = len(cs.lookups)
    rng = np.random.default_rng(seed)
    counts = dict(fixed=cs.num_fixed_columns, advice=cs.num_advice_columns, instance=cs.num_instance_columns, perm_cosets=len(cs.permutation_columns),
                  perm_products=n_sets, lookup_product=L, lookup_input=L, lookup_table=L)
    host = {key: [rand_fr_array(rng, size) for _ in range(c)] for key, c in counts.items()}
    host_l = [rand_fr_array(rng, size) for _ in range(3)]
    beta, gamma, theta, y = (fr_mont(int(v)) for v in rng.integers(1, 1 << 62, size=4))
    yE = pow(fr_int_array(y.reshape(1, 4))[0], E, R_MOD)
    if kind != "uniform":
        import parity_cases as pc
        import pyref
        host = {key: [pc.structured_fr(orc, pyref, size, kind, seed + 10 * i + j) for j in range(c)] for i, (key, c) in enumerate(counts.items())}
        host_l = [pc.structured_fr(orc, pyref, size, kind, seed + 100 + j) for j in range(3)]
    split = be.quotient_program_split(prog)["low_cosets"]
    assert split == 2                                                # (the programs here all have a degree split: every part is covered)

    def run(cols, ls, rows, out_rows, **kw):
        dev = {key: [be.to_device(np.ascontiguousarray(c[rows])) for c in v] for key, v in cols.items()}
        dl = [be.to_device(np.ascontiguousarray(c[rows])) for c in ls]
        prev = rand_fr_array(rng, out_rows)
        outs = []
        for acc in (False, True):
            o = be.to_device(prev.copy())
            be.quotient_run_dev(prog, **{key: dev[key] for key in dev}, l0=dl[0], l_last=dl[1], l_active_row=dl[2], challenges=[], beta=beta, gamma=gamma,
                                theta=theta, y=y, out=o, accumulate=acc, **kw)
            outs.append(o.download((out_rows, 4)))
            o.free()
        if cancel:
            yEi = pow(yE, -1, R_MOD)
            o = be.to_device(fr_mont_array([(-n_ * yEi) % R_MOD for n_ in fr_int_array(outs[0])]))
            be.quotient_run_dev(prog, **{key: dev[key] for key in dev}, l0=dl[0], l_last=dl[1], l_active_row=dl[2], challenges=[], beta=beta, gamma=gamma,
                                theta=theta, y=y, out=o, accumulate=True, **kw)
            assert not o.download((out_rows, 4)).any(), ("prev * y^E + N must be the canonical zero on every row", kw)
            o.free()
        for v in dev.values():
            for d in v:
                d.free()
        for d in dl:
            d.free()
        N, got, P = fr_int_array(outs[0]), fr_int_array(outs[1]), fr_int_array(prev)
        assert got == [(p_ * yE + n_) % R_MOD for p_, n_ in zip(P, N)], kw
        return outs

    whole = slice(None)
    run(host, host_l, whole, size)                                   # the whole extended domain
    run(host, host_l, whole, size, part=1)                           # its high part
    run(host, host_l, whole, split * n, part=2, low_cosets=split)    # its low part on cosets 0 .. split-1 (accumulate: the program's own low cosets)
    nc = size // n
    for j in (0, nc - 1):                                            # one coset (coset layout): whole program, high part, low part
        rows = slice(j, None, nc)
        run(host, host_l, rows, n, coset=j)
        run(host, host_l, rows, n, coset=j, part=1)
        run(host, host_l, rows, n, coset=j, part=2)
    _release(params, pk)


def test_accumulate_mode_of_the_quotient_emulated(emu, orc):
    cs, fixed, asm, _, _ = tcp.toy_circuit(5)
    _acc_kernel(emu, 5, (cs, fixed, asm), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
def test_accumulate_mode_of_the_quotient_gpu(gpu, orc, jit):
    gpu.tune(quot_jit=jit, quot_jit_group=64)
    try:
        cs, fixed, asm, _, _ = tcp.toy_circuit(9)
        _acc_kernel(gpu, 9, (cs, fixed, asm), 2)
        sc = _sgx_module()
        cs, fixed, asm, _ = sc.build(z, gpu, 8)
        _acc_kernel(gpu, 8, (cs, fixed, asm), 3)
    finally:
        gpu.tune(quot_jit=0)
