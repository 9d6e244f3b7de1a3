"""Multi-phase advice and halo2's Challenge API through the native prover: zk_plonk_pk_build_phased / zk_plonk_prove_phased / zk_plonk_last_challenges /
zk_mock_prover_verify_phased (include/zkmi355.h), their Python bindings (plonk.NativeKey, plonk.PhasedProver, plonk.last_challenges, NativeMockProver) and
the Python twin plonk.create_proof(.., next_phase=..).  The circuits are tests/phased_cases.py (A two-phase RLC, B three phases, C index order != commitment
order, D two circuits), the acceptance check is tests/phased_verifier.py — an independent restatement of halo2's verifier on oracle/pyref.py.
Every check runs on the kernel emulator and, marked gpu, on the device."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd._lib import PHASE_FN, PlonkPhases
from zk_dcap_verifier_amd.transcript import Blake2bWrite

import phased_cases as pc
import phased_verifier as pv
import test_create_proof as tcp

ZK_ERR_ARG, ZK_ERR_LIMIT, ZK_ERR_PROGRAM = -1, -5, -4


class World:
    """per backend: SRS, keys and provers of the cases, built once and shared by the tests of this module"""

    def __init__(self):
        self.made = {}

    def get(self, be, name, k=6):
        key = (id(be), name, k)
        if key not in self.made:
            case = pc.CASES[name](k)
            params = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=be)
            pk = plonk.keygen(params, case.cs, case.fixed, case.asm)
            self.made[key] = (case, params, pk, plonk.PhasedProver(params, pk))
        return self.made[key]

    def close(self):
        for case, params, pk, prover in self.made.values():
            prover.release()
            pk.release()
            params.release()
        self.made.clear()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def _prove(world, be, name, seed=5, tamper=None, shift=0, k=6):
    case, params, pk, prover = world.get(be, name, k)
    proof = prover.create_proof(case.phase0(tamper), case.instances, np.random.default_rng(seed), case.next_phase(tamper, shift))
    return case, pk, prover, proof


def _verify(pk, case, proof, out=None):
    try:
        return pv.verify_proof_phased(pk.vk, tcp.TAU, case.instances, proof, out)
    except ValueError:
        return False


# ---- accepted proofs, the Python twin, the challenges --------------------------------------------------------------------------------------------------
def _accepted_and_twin(world, be, name):
    case, pk, prover, proof = _prove(world, be, name)
    assert len(proof) == pv.proof_length(case.cs, case.m)
    squeezed = []
    assert _verify(pk, case, proof, squeezed) is True
    assert plonk.last_challenges(be) == squeezed and len(squeezed) == case.cs.num_challenges + 8      # what a fresh transcript squeezes when fed the proof bytes
    if case.m == 1:
        _, params, _, _ = world.get(be, name)
        tr = Blake2bWrite()
        plonk.create_proof(params, pk, case.phase0()[0], [], np.random.default_rng(5), tr, next_phase=case.next_phase())
        assert tr.finalize() == proof, "the Python twin emits other bytes"
    other = prover.create_proof(case.phase0(), case.instances, np.random.default_rng(6), case.next_phase())
    assert other != proof and _verify(pk, case, other) is True


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_phased_proofs_are_accepted_and_equal_the_twin_emulated(emu, orc, world, name):
    _accepted_and_twin(world, emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_phased_proofs_are_accepted_and_equal_the_twin_gpu(gpu, orc, world, name):
    _accepted_and_twin(world, gpu, name)


def _negative_controls(world, be):
    case, pk, _, good = _prove(world, be, "A")
    assert _verify(pk, case, good) is True
    _, _, _, bad = _prove(world, be, "A", tamper="acc")                # one wrong acc row
    assert _verify(pk, case, bad) is False
    _, _, _, bad = _prove(world, be, "A", shift=1)                     # phase 1 built from c0 + 1
    assert _verify(pk, case, bad) is False
    swapped = good[32:64] + good[:32] + good[64:]                      # the first two advice commitments swapped
    assert swapped != good and _verify(pk, case, swapped) is False


def test_negative_controls_are_rejected_emulated(emu, orc, world):
    _negative_controls(world, emu)


@pytest.mark.gpu
def test_negative_controls_are_rejected_gpu(gpu, orc, world):
    _negative_controls(world, gpu)


# ---- the caller's rng: phase-major blocks -------------------------------------------------------------------------------------------------------------------
def _expected_blocks(cs, m, n):
    """the Fr::random blocks in halo2's order ([3P-MEM] plonk/prover.rs): per phase, per circuit, the blinding rows of the phase's columns and then one Blind each; then
    as for single-phase circuits"""
    bf = cs.blinding_factors()
    phase_of = cs._advice_phases()
    L = len(cs.lookups)
    chunk = cs.permutation_chunk_len()
    n_sets = -(-len(cs.permutation_columns) // chunk) if cs.permutation_columns else 0
    blocks = []
    for p in cs.phases():
        cols = sum(1 for q in phase_of if q == p)
        for _ in range(m):
            blocks += [bf + 1] * cols + [1] * cols
    blocks += [bf + 1, bf + 1, 1, 1] * (m * L) + [bf, 1] * (m * n_sets) + [bf, 1] * (m * L) + [n, 1] + [1] * (cs.degree() - 1)
    A = cs.num_advice_columns
    single_phase_total = m * (A * (bf + 1) + A + L * (2 * (bf + 1) + 2) + n_sets * (bf + 1) + L * (bf + 1)) + n + 1 + (cs.degree() - 1)
    return blocks, single_phase_total


def _draw_blocks(world, be, name):
    case, _, prover, _ = _prove(world, be, name)
    blocks, total = _expected_blocks(case.cs, case.m, 1 << case.k)
    assert prover.draw_counts == blocks
    assert sum(prover.draw_counts) == total


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_rng_sees_the_phase_major_block_sequence_emulated(emu, orc, world, name):
    _draw_blocks(world, emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_rng_sees_the_phase_major_block_sequence_gpu(gpu, orc, world, name):
    _draw_blocks(world, gpu, name)


# ---- single-phase circuits keep their bytes ---------------------------------------------------------------------------------------------------------------------
def _toy_golden(be):
    cs, fixed, asm, advice, instances = tcp.toy_circuit(6)
    assert not cs.is_phased()
    params = z.kzg.ParamsKZG.setup(6, tcp.TAU, backend=be)
    pk = plonk.keygen(params, cs, fixed, asm)
    prover = plonk.PhasedProver(params, pk)                           # all-zero phase lists, no challenges
    proof = prover.create_proof([[a.copy() for a in advice]], [instances], np.random.default_rng(7), next_phase=None)      # a NULL callback
    assert proof == tcp._golden(tcp.GOLDEN_PROOF)
    squeezed = []
    assert pv.verify_proof_phased(pk.vk, tcp.TAU, [instances], proof, squeezed) is True
    assert plonk.last_challenges(be) == squeezed and len(squeezed) == 8
    # the descriptor-level entry records its challenges too
    assert plonk.NativeProver(params, pk).create_proof([a.copy() for a in advice], instances, np.random.default_rng(7)) == proof
    assert plonk.last_challenges(be) == squeezed
    small = np.zeros(32, dtype=np.uint8)
    n = C.c_size_t()
    assert be.lib.zk_plonk_last_challenges(small.ctypes.data_as(C.c_void_p), C.c_size_t(32), C.byref(n)) == ZK_ERR_LIMIT and n.value == 8
    prover.release()
    pk.release()
    params.release()


def test_all_zero_phases_reproduce_the_toy_golden_emulated(emu, orc):
    _toy_golden(emu)


@pytest.mark.gpu
def test_all_zero_phases_reproduce_the_toy_golden_gpu(gpu, orc):
    _toy_golden(gpu)


def test_phased_verifier_returns_what_the_oracle_verifier_returns_on_the_goldens(emu, orc):
    """the three committed single-phase goldens tie tests/phased_verifier.py to what is already pinned"""
    import verifier
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    cases = []
    cs, fixed, asm, _, instances = tcp.toy_circuit(6)
    cases.append((6, cs, fixed, asm, instances, tcp.GOLDEN_PROOF))
    for k, census, golden in ((8, "chip_estimate", tcp.GOLDEN_SGX), (9, "reference_exact", tcp.GOLDEN_REF_EXACT)):
        cs, fixed, asm, _ = sc.build(z, emu, k, census=census)
        cases.append((k, cs, fixed, asm, [], golden))
    for k, cs, fixed, asm, instances, golden in cases:
        params = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=emu)
        pk = plonk.keygen(params, cs, fixed, asm)
        proof = tcp._golden(golden)
        assert pv.verify_proof_phased(pk.vk, tcp.TAU, [instances], proof) is verifier.verify_proof(pk.vk, tcp.TAU, instances, proof) is True
        bad = bytearray(proof)
        bad[40] ^= 1
        results = []
        for fn in (lambda b: pv.verify_proof_phased(pk.vk, tcp.TAU, [instances], b), lambda b: verifier.verify_proof(pk.vk, tcp.TAU, instances, b)):
            try:
                results.append(fn(bytes(bad)))
            except ValueError:
                results.append("malformed")
        assert results[0] == results[1] and results[0] is not True
        pk.release()
        params.release()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def _build(be, key, params, advice_phase=None, challenge_phase=None, n_advice=None, n_challenges=None, shard_world=0):
    """zk_plonk_pk_build_phased on a copy of the key's host description with other phase lists; returns (rc, handle)"""
    ap = np.asarray(key.pk.vk.cs._advice_phases() if advice_phase is None else advice_phase, dtype=np.uint8)
    cp = np.asarray(key.pk.vk.cs.challenge_phase if challenge_phase is None else challenge_phase, dtype=np.uint8)
    ph = PlonkPhases()
    ph.struct_size = C.sizeof(PlonkPhases)
    ph.n_advice, ph.advice_phase = len(ap) if n_advice is None else n_advice, ap.ctypes.data if ap.size else None
    ph.n_challenges, ph.challenge_phase = len(cp) if n_challenges is None else n_challenges, cp.ctypes.data if cp.size else None
    host = type(key.host)()
    C.memmove(C.byref(host), C.byref(key.host), C.sizeof(host))
    host.shard_world = shard_world
    out = C.c_uint64()
    rc = be.lib.zk_plonk_pk_build_phased(be.ctx, C.byref(host), C.byref(ph), C.c_uint64(params.g.handle), C.c_uint64(params.g_lagrange.handle), C.byref(out))
    return rc, out.value


def _refusals(world, be):
    case, params, pk, prover = world.get(be, "A")
    key = prover.key
    err = lambda: (be.lib.zk_last_error(be.ctx) or b"").decode()
    rc, handle = _build(be, key, params)
    assert rc == 0
    assert be.lib.zk_plonk_pk_release(be.ctx, C.c_uint64(handle)) == 0
    assert _build(be, key, params, advice_phase=[0, 0, 2, 2])[0] == ZK_ERR_ARG and "phase 2" in err()          # a gap
    assert _build(be, key, params, advice_phase=[0, 0, 1, 3])[0] == ZK_ERR_ARG                               # a phase above 2
    assert _build(be, key, params, advice_phase=[0, 0, 0, 0], challenge_phase=[1])[0] == ZK_ERR_ARG          # a challenge after a phase not in use
    assert _build(be, key, params, advice_phase=[0, 0, 1])[0] == ZK_ERR_ARG                                  # the phase list and the key disagree on n_advice
    assert _build(be, key, params, challenge_phase=[0, 0])[0] == ZK_ERR_ARG and "challenges" in err()        # the blobs declare one challenge, the list two
    assert _build(be, key, params, challenge_phase=[])[0] == ZK_ERR_ARG
    assert _build(be, key, params, shard_world=2)[0] == ZK_ERR_ARG and "single-phase" in err()                # one proof over several GPUs stays single-phase
    assert _build(be, key, params, challenge_phase=[0] * 300)[0] == ZK_ERR_LIMIT and "constant bank" in err()
    # a NULL callback on a key with later phases
    with pytest.raises(z.ZkError) as e:
        prover.create_proof(case.phase0(), case.instances, np.random.default_rng(1), next_phase=None)
    assert e.value.code == ZK_ERR_ARG and "next_phase is NULL" in str(e.value)
    # a callback that returns 1: ZK_ERR_ARG naming the phase; the next proof on the same context succeeds
    seen = []

    def refuse(_user, phase, _chal, n_chal, _advice):
        seen.append((phase, n_chal))
        return 1
    with pytest.raises(z.ZkError) as e:
        prover.create_proof(case.phase0(), case.instances, np.random.default_rng(1), raw_callback=PHASE_FN(refuse))
    assert e.value.code == ZK_ERR_ARG and "phase 1" in str(e.value) and seen == [(1, 1)]
    # ... and one that returns 0 but leaves the pointers NULL
    with pytest.raises(z.ZkError) as e:
        prover.create_proof(case.phase0(), case.instances, np.random.default_rng(1), raw_callback=PHASE_FN(lambda *a: 0))
    assert e.value.code == ZK_ERR_ARG and "NULL in phase 1" in str(e.value)
    proof = prover.create_proof(case.phase0(), case.instances, np.random.default_rng(5), case.next_phase())
    assert _verify(pk, case, proof) is True
    # an exception in the caller's synthesis ends the proof and comes out as itself
    def broken(phase, challenges, circuit=0):
        raise KeyError("synthesis failed")
    with pytest.raises(KeyError):
        prover.create_proof(case.phase0(), case.instances, np.random.default_rng(1), broken)
    assert prover.create_proof(case.phase0(), case.instances, np.random.default_rng(5), case.next_phase()) == proof


def test_refusals_emulated(emu, orc, world):
    _refusals(world, emu)


@pytest.mark.gpu
def test_refusals_gpu(gpu, orc, world):
    _refusals(world, gpu)


# ---- the mock prover with challenge values -------------------------------------------------------------------------------------------------------------------
def _mock(be):
    case = pc.case_a()
    u = case.cs.usable_rows(case.k)
    ch = [0x1234567 * 0x89ABCDEF % plonk.circuit.R_MOD]
    for tamper, want in ((None, []), ("acc", [plonk.dev.MockFailure("gate", 1, u - 2, 0, 0)]), ("lookup", [plonk.dev.MockFailure("lookup", 0, 4, 0, 0)])):
        w = case.witness(ch, 0, tamper)
        native = plonk.NativeMockProver.run(case.k, case.cs, case.fixed, w, [], case.asm, backend=be, challenges=ch)
        host = plonk.MockProver.run(case.k, case.cs, case.fixed, w, [], case.asm, challenges=ch)
        assert native.failures() == want
        assert native.verify() == host.verify()
        assert tuple(native.counts) == (sum(1 for f in want if f.kind == "gate"), sum(1 for f in want if f.kind == "lookup"), 0)
    # three phases, four challenges, one of them in a gate only
    case = pc.case_b()
    ch = [3, 5, 7, 11]
    w = case.witness(ch, 0)
    assert plonk.NativeMockProver.run(case.k, case.cs, case.fixed, w, [], case.asm, backend=be, challenges=ch).verify() == []
    w[2][6] = (w[2][6] + 1) % plonk.circuit.R_MOD
    native = plonk.NativeMockProver.run(case.k, case.cs, case.fixed, w, [], case.asm, backend=be, challenges=ch)
    assert native.verify() == plonk.MockProver.run(case.k, case.cs, case.fixed, w, [], case.asm, challenges=ch).verify() != []
    # the values are the caller's: other challenges, other verdict; a wrong count is an argument error; the unphased entry keeps refusing such blobs
    assert plonk.NativeMockProver.run(case.k, case.cs, case.fixed, case.witness(ch, 0), [], case.asm, backend=be, challenges=[3, 5, 8, 11]).verify() != []
    with pytest.raises(z.ZkError) as e:
        plonk.NativeMockProver.run(case.k, case.cs, case.fixed, case.witness(ch, 0), [], case.asm, backend=be, challenges=[3, 5, 7]).verify()
    assert e.value.code == ZK_ERR_ARG
    with pytest.raises(z.ZkError) as e:
        plonk.NativeMockProver.run(case.k, case.cs, case.fixed, case.witness(ch, 0), [], case.asm, backend=be).verify()
    assert e.value.code == ZK_ERR_PROGRAM


def test_mock_prover_takes_challenge_values_emulated(emu, orc):
    _mock(emu)


@pytest.mark.gpu
def test_mock_prover_takes_challenge_values_gpu(gpu, orc):
    _mock(gpu)


# ---- the Python mirror ---------------------------------------------------------------------------------------------------------------------------------------------
def test_constraint_system_phases_and_challenges():
    from zk_dcap_verifier_amd.plonk import expression as ex
    cs = plonk.ConstraintSystem(num_advice_columns=2)
    assert cs.phases() == [0] and cs.num_challenges == 0 and not cs.is_phased()
    with pytest.raises(ValueError):
        cs.advice_column_in(2)                                         # no column in phase 1
    with pytest.raises(ValueError):
        cs.challenge_usable_after(1)
    c0 = cs.challenge_usable_after(0)
    assert cs.advice_column_in(1) == 2 and cs.advice_column_in(2) == 3 and cs.phases() == [0, 1, 2] and cs.advice_column_phase == [0, 0, 1, 2]
    c1 = cs.challenge_usable_after(2)
    assert (c0, c1) == (ex.Challenge(0), ex.Challenge(1)) and cs.challenge_phase == [0, 2] and cs.is_phased()
    e = plonk.Fixed(0) * plonk.Advice(2) * c0 + c1
    assert ex.degree(c0) == 0 and ex.degree(e) == 2
    log = {}
    ex.queries(e, log)
    assert list(log) == [("fixed", 0, 0), ("advice", 2, 0)]            # a challenge creates no query
    assert ex.evaluate(e, lambda c, r: 2, lambda c, r: 3, None, lambda i: [5, 7][i]) == 2 * 3 * 5 + 7
    with pytest.raises(ValueError):
        ex.evaluate(e, lambda c, r: 2, lambda c, r: 3, None)
    # value source 5 in the ZKQ1 blob, and the blob's challenge count
    cs.create_gate(e)
    prog = plonk.compile_program(cs, 4, 6)
    assert prog.n_challenges == 2 and np.frombuffer(prog.to_blob(), dtype=np.uint32)[6] == 2
    assert any(op[0] == z.evaluation.CHALLENGE for calc in prog.custom_gates.calculations for op in calc[2] if isinstance(op, tuple) and len(op) == 3 and isinstance(op[0], int))


def test_rust_and_ctypes_declarations_match_the_header():
    """pk_desc.rs declares zk_plonk_phases, mi355x.rs zk_phase_fn and the new entry points as include/zkmi355.h does; so do the ctypes mirrors.  (The header declares
    the struct apart from its typedef and the callback as a function type plus a pointer to it; both are rewritten here into the form the shared parser reads.)"""
    import re
    import test_shim_abi as sa
    from conftest import ROOT
    from zk_dcap_verifier_amd.plonk.native import PkHost
    hdr = open(sa.HEADER).read()
    hdr = hdr.replace("typedef struct zk_plonk_phases zk_plonk_phases;", "")
    hdr = re.sub(r"\bstruct zk_plonk_phases \{(.*?)\};", lambda m: "typedef struct zk_plonk_phases {%s} zk_plonk_phases;" % m.group(1), hdr, flags=re.S)
    hdr, n = re.subn(r"typedef int ZK_PHASE_CALLBACK\((.*?)\);\s*typedef ZK_PHASE_CALLBACK\* zk_phase_fn;", lambda m: "typedef int (*zk_phase_fn)(%s);" % m.group(1), hdr, flags=re.S)
    assert n == 1
    hs, fnptrs, protos = sa.parse_header(hdr)
    assert "zk_phase_fn" in fnptrs and {"zk_plonk_pk_build_phased", "zk_plonk_prove_phased", "zk_plonk_last_challenges", "zk_mock_prover_verify_phased"} <= set(protos)
    seen = set()
    for f in ("pk_desc.rs", "mi355x.rs", "mock_native.rs", "create_proof_native.rs"):
        rs = open(os.path.join(ROOT, "shim", "halo2_proofs_mi355x", "src", f)).read()
        rs = rs.replace("#[repr(C)]\n#[derive(Debug)]\npub struct ZkPlonkPhases", "#[repr(C)]\npub struct ZkPlonkPhases").replace('unsafe extern "C" fn(', 'extern "C" fn(')
        structs, externs, fntypes, _ = sa.parse_rust(rs)
        seen |= set(structs) | set(externs) | set(fntypes)
        bad = sa.diff_against_header(rs, f, header_text=hdr + "\n" + open(sa.RCCL_HEADER).read())
        assert not bad, "\n".join(bad)
    assert {"ZkPlonkPhases", "ZkPhaseFn", "zk_plonk_pk_build_phased", "zk_plonk_prove_phased", "zk_plonk_last_challenges", "zk_mock_prover_verify_phased"} <= seen
    assert [n_ for n_, _ in hs["zk_plonk_phases"]] == [n_ for n_, _ in PlonkPhases._fields_]
    assert [n_ for n_, _ in hs["zk_plonk_pk_host"]] == [n_ for n_, _ in PkHost._fields_]
    lib = C.CDLL(z.LIB_PATH)
    lib.zk_abi_struct_size.restype = C.c_uint32
    assert lib.zk_abi_struct_size(b"zk_plonk_phases") == C.sizeof(PlonkPhases) == 32 and lib.zk_abi_struct_size(b"zk_plonk_pk_host") == C.sizeof(PkHost)


# ---- GPU only --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_case_a_at_the_shims_min_len_gpu(gpu, orc, world):
    case, pk, _, proof = _prove(world, gpu, "A", k=12)
    assert _verify(pk, case, proof) is True


@pytest.mark.gpu
def test_case_a_with_device_resident_advice_gpu(gpu, orc, world):
    case, params, pk, prover = world.get(gpu, "A")
    _, _, _, want = _prove(world, gpu, "A")
    first = [[None if a is None else gpu.to_device(a) for a in case.phase0()[0]]]
    host_fn = case.next_phase()
    later = []

    def on_device(phase, challenges, circuit=0):
        cols = {i: gpu.to_device(a) for i, a in host_fn(phase, challenges, circuit).items()}
        later.extend(cols.values())
        return cols
    assert prover.create_proof(first, case.instances, np.random.default_rng(5), on_device) == want
    for d in [a for a in first[0] if a is not None] + later:
        d.free()


@pytest.mark.gpu
def test_case_a_generated_quotient_kernels_emit_the_interpreters_bytes_gpu(gpu, orc, world):
    _, _, _, want = _prove(world, gpu, "A")
    case = pc.case_a()
    gpu.tune(quot_jit=1)
    try:
        params = z.kzg.ParamsKZG.setup(case.k, tcp.TAU, backend=gpu)
        pk = plonk.keygen(params, case.cs, case.fixed, case.asm)
        prover = plonk.PhasedProver(params, pk)
        got = prover.create_proof(case.phase0(), case.instances, np.random.default_rng(5), case.next_phase())
    finally:
        gpu.tune(quot_jit=0)
    assert got == want
    prover.release()
    pk.release()
    params.release()


@pytest.mark.gpu
def test_case_a_side_lane_on_and_off_gpu(gpu, orc, world):
    """the helper context transforms phase 0's columns while the callback synthesises phase 1: no byte depends on it.  (A's key keeps three cosets by default and such a
    proof has no side lane: the key here is built with its extended forms.)"""
    _, _, _, want = _prove(world, gpu, "A")
    case = pc.case_a()
    gpu.tune(quot_piece_cosets=0)
    try:
        params = z.kzg.ParamsKZG.setup(case.k, tcp.TAU, backend=gpu)
        pk = plonk.keygen(params, case.cs, case.fixed, case.asm, piece_cosets=False)
        prover = plonk.PhasedProver(params, pk)
    finally:
        gpu.tune(quot_piece_cosets=1)
    try:
        for lane in (2, 0):
            gpu.tune(prover_side_lane=lane)
            assert prover.create_proof(case.phase0(), case.instances, np.random.default_rng(5), case.next_phase()) == want
    finally:
        gpu.tune(prover_side_lane=1)
    prover.release()
    pk.release()
    params.release()


@pytest.mark.gpu
def test_two_contexts_prove_case_a_from_one_shared_key_gpu(gpu, orc, world):
    case, params, pk, prover = world.get(gpu, "A")
    _, _, _, want = _prove(world, gpu, "A")
    other = z.Backend(0)
    params_b = z.kzg.ParamsKZG.shared_with(params, other)
    key_b = prover.key.shared_with(other, params_b)
    prover_b = plonk.PhasedProver(params_b, pk, key=key_b)
    out = {}

    def run(name, p):
        out[name] = [p.create_proof(case.phase0(), case.instances, np.random.default_rng(5), case.next_phase()) for _ in range(2)]
    ts = [threading.Thread(target=run, args=(n, p)) for n, p in (("a", prover), ("b", prover_b))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out["a"] == out["b"] == [want, want]
    key_b.release()
    params_b.release()
    other.close()
