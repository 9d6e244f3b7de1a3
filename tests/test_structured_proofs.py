"""Whole proofs on structured witnesses and planted random draws (tests/proof_cases.py): the native prover (zk_plonk_create_proof, _multi) and its Python twin
(plonk/prover.py + shplonk.py) must emit, byte for byte, what the independent CPU prover (oracle/prover.py) emits for the same circuit, witness and rng stream —
where the committed columns are zero, constant or r - 1 on every row, where lookup inputs are one table row, where blinding rows are 0 or r - 1, where the
rejection sampler meets draws that share r's top limbs, and where a commitment is the identity and the proof must be refused, explained and harmless.

The circuits and what each was chosen for:
  random_circuits.random_circuit(k, seed), witnesses that do NOT satisfy the gates (halo2's own route only: quot_degree_split = 0, piece_cosets = False) — SEEDS below
  the same circuits with their gates switched off (proof_cases.gates_off): satisfied, the lookup and permutation arguments still run; seed 3 has degree 4, so the key can
      keep three cosets (h(X) from cosets) or the extended domain, with and without the degree split
  tcp.toy_circuit (degree 5: the extended route, degree split on / off; lookup with a product input; instance query), tpc.graded_circuit(k, 1) (degree 4: both routes),
  tools/sgx_shaped_circuit.build (the bench's census: 25 advice columns, 11 lookups of 4-5 expressions, 6 permutation sets) with witnesses at the edge of what their gates allow
"""
import numpy as np
import pytest

import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, rand_fr_array
from zk_dcap_verifier_amd.transcript import Blake2bWrite

import multi_circuit_verifier as mv
import proof_cases as pc
import random_circuits as rc
import test_create_proof as tcp
import test_piece_cosets as tpc

ZK_ERR_ARG = -1

# seed -> the features it was picked for (test_the_seeds_cover_what_they_claim holds the generator to them)
SEEDS = {2: dict(lookups=0, sets=2, e=1),                             # no lookup; degree 3, one permutation column per set
         3: dict(lookups=1, sets=2, e=2, instance=1),                 # degree 4; one lookup; an instance column
         7: dict(lookups=2, shared_table=True, sets=2, e=2, instance=1),   # two lookups into one table (the table column is compressed and sorted once)
         33: dict(lookups=1, sets=1, e=3, instance=1)}                # degree 6: extended_k - k = 3
EMU_K = {seed: 5 + seed % 2 for seed in SEEDS}                        # as tests/test_random_circuits.py
GPU_K = {2: 8, 3: 6, 7: 7, 33: 6}

_REF = {}                                                             # (circuit, witness, draws) -> the oracle's bytes, or the exception it raised
_CIRCUITS = {}


def test_the_seeds_cover_what_they_claim():
    for seed, want in SEEDS.items():
        cs, _, _, _, instances = rc.random_circuit(EMU_K[seed], seed)
        e = 0
        while (1 << e) < cs.degree() - 1:
            e += 1
        tabs = [tuple(lk.table_expressions) for lk in cs.lookups]
        got = dict(lookups=len(cs.lookups), sets=pc.n_sets(cs), e=e)
        if len(set(tabs)) < len(tabs):
            got["shared_table"] = True
        if cs.num_instance_columns:
            got["instance"] = cs.num_instance_columns
        assert got == want, (seed, got)
        assert pc.free_advice(cs), seed                               # every circuit has advice columns that feed no lookup
    assert any(f["lookups"] == 0 for f in SEEDS.values()) and any(f.get("shared_table") for f in SEEDS.values())
    assert any(f["sets"] >= 2 for f in SEEDS.values()) and any(f["e"] == 3 for f in SEEDS.values())


# ---- PlantedRng itself, and the two samplers on it --------------------------------------------------------------------------------------------------------------
def test_boundary_pattern_holds_every_edge_of_the_rejection_rule():
    R, top, m64 = R_MOD, R_MOD >> 192, (1 << 64) - 1
    vals = [v for v in pc.BOUNDARY if v is not None]
    assert {R - 1, R, R + 1, 0, 1, (1 << 254) - 1} <= set(vals) and max(vals) < 1 << 254
    tie = [v for v in vals if v >> 192 == top]                        # decided by the lower limbs
    assert any(v < R and (v >> 128) != (R >> 128) for v in tie) and any(v >= R and (v >> 128) != (R >> 128) for v in tie)         # differ from r in limb 2
    assert any(v < R and (v >> 128) == (R >> 128) and (v >> 64) != (R >> 64) for v in tie) and any(v >= R and (v >> 128) == (R >> 128) and (v >> 64) != (R >> 64) for v in tie)   # ... in limb 1
    top3 = [v for v in vals if v >> 64 == R >> 64]                    # r's top three limbs
    assert {v & m64 for v in top3} >= {0, (R & m64) - 1, R & m64, (R & m64) + 1, m64}
    run = best = 0
    for v in pc.BOUNDARY * 2:
        run = run + 1 if v is not None and v >= R else 0
        best = max(best, run)
    assert best >= 8                                                  # longer than a batch of blinding rows


@pytest.mark.parametrize("count", [1, 6, 7, 32, 64, 169])
def test_both_samplers_agree_on_the_boundary_stream(orc, count):
    """fields.rand_fr_array (the provers') and oracle/prover.py:rand_fr (Python integers) on equal planted streams, at every offset into the pattern: the same elements, all
    below r, the same rows consumed; from 6 rows on some batch is redrawn more than once, on a shrinking set"""
    import prover as op
    rounds = 0
    for offset in range(len(pc.BOUNDARY)):
        a, b = pc.PlantedRng(count, pattern=pc.BOUNDARY), pc.PlantedRng(count, pattern=pc.BOUNDARY)
        if offset:
            a.integers(0, 1 << 64, size=(offset, 4), dtype=np.uint64), b.integers(0, 1 << 64, size=(offset, 4), dtype=np.uint64)
        got = rand_fr_array(a, count)
        assert fr_int_array(got) == op.rand_fr(b, count), (count, offset)
        assert all(sum(int(row[j]) << (64 * j) for j in range(4)) < R_MOD for row in got)
        assert a.served == b.served and a.calls == b.calls and a.planted_rejected == b.planted_rejected
        redraws = a.calls[2 if offset else 1:]
        assert redraws == sorted(redraws, reverse=True) and all(r <= count for r in redraws)
        rounds = max(rounds, len(redraws))
    assert rounds >= (2 if count >= 6 else 0), rounds


def test_item_addressed_streams_are_never_rejected(orc):
    cs, *_ = rc.random_circuit(5, 3)
    items = pc.draw_items(cs, 5)
    fills = {("bi", 0): "zeros", ("bt", 0): "minus_one", ("perm_blind", 1): ("const", 5), ("random_poly", 0): ("delta_last", 9), ("blind", 2): "minus_one", ("advice", 4): ("delta_first", 3)}
    rng = pc.PlantedRng.for_items(1, items, fills)
    for purpose, index, count in items:
        got = rand_fr_array(rng, count)
        raw = [sum(int(row[j]) << (64 * j) for j in range(4)) for row in got]
        if (purpose, index) in fills:
            assert raw == pc.fill_values(fills[purpose, index], count)
        assert all(v < R_MOD for v in raw)
    assert rng.calls == [c for _, _, c in items]                      # one batch per item: nothing was redrawn
    rng.assert_exhausted()
    with pytest.raises(AssertionError):
        pc.PlantedRng.for_items(1, items, {("bi", 1): "zeros"})        # (no such item in this circuit)


# ---- keys kept for the module: one keygen per (circuit, route) ---------------------------------------------------------------------------------------------------
class Keyring:
    def __init__(self, be):
        self.be, self.params, self.keys = be, {}, {}

    def key(self, circ, piece_cosets=False, split=0):
        """(params, pk, NativeProver) of a circuit on one route: h(X) from cosets or from the extended domain, the quotient program compiled with or without its degree split"""
        k = circ["k"]
        if k not in self.params:
            self.params[k] = z.kzg.ParamsKZG.setup(k, tcp.TAU, backend=self.be)
        name = (circ["key"], piece_cosets, split)
        if name not in self.keys:
            self.be.tune(quot_degree_split=split)
            try:
                pk = plonk.keygen(self.params[k], circ["cs"], circ["fixed"], circ["asm"], piece_cosets=piece_cosets)
            finally:
                self.be.tune(quot_degree_split=1)
            assert pk.pieces_from_cosets == piece_cosets
            assert split or self.be.quotient_program_split(pk.evaluator.handle)["low_cosets"] == 0
            self.keys[name] = (pk, plonk.NativeProver(self.params[k], pk))
        return (self.params[k],) + self.keys[name]

    def native(self, circ, advice, instances, rng, piece_cosets=False, split=0, device=False):
        _, _, prover = self.key(circ, piece_cosets, split)
        self.be.tune(quot_degree_split=split)
        try:
            cols = [self.be.to_device(a) for a in advice] if device else [a.copy() for a in advice]
            try:
                return prover.create_proof(cols, instances, rng)
            finally:
                if device:
                    for c in cols:
                        c.free()
        finally:
            self.be.tune(quot_degree_split=1)

    def twin(self, circ, advice, instances, rng, piece_cosets=False, split=0):
        params, pk, _ = self.key(circ, piece_cosets, split)
        self.be.tune(quot_degree_split=split)
        try:
            tr = Blake2bWrite()
            plonk.create_proof(params, pk, [a.copy() for a in advice], instances, rng, tr)
            return tr.finalize()
        finally:
            self.be.tune(quot_degree_split=1)

    def close(self):
        for pk, _ in self.keys.values():
            pk.release()
        for p in self.params.values():
            p.release()


@pytest.fixture(scope="module")
def emu_ring(emu):
    ring = Keyring(emu)
    yield ring
    ring.close()


@pytest.fixture(scope="module")
def gpu_ring(gpu):
    ring = Keyring(gpu)
    yield ring
    ring.close()


def _circuit(key, k, build):
    if key not in _CIRCUITS:
        cs, fixed, asm, advice, instances = build()
        _CIRCUITS[key] = dict(key=key, k=k, cs=cs, fixed=fixed, asm=asm, advice=advice, instances=instances)
    return _CIRCUITS[key]


def random_case(k, seed):
    return _circuit(("random", k, seed), k, lambda: rc.random_circuit(k, seed))


def _reference(circ, wkey, advice, instances, dkey, draws, satisfied=False):
    """the oracle's bytes for (circuit, witness `wkey`, draws `dkey`), computed once; `draws()` makes a fresh generator"""
    name = (circ["key"], wkey, dkey, satisfied)
    if name not in _REF:
        rng = draws()
        try:
            _REF[name] = pc.oracle_proof(circ["k"], tcp.TAU, circ["cs"], circ["fixed"], circ["asm"], advice, instances, rng, circ["key"], require_satisfied=satisfied)
        except ValueError as e:
            _REF[name] = e
        if isinstance(rng, pc.PlantedRng) and rng.pattern is None and not isinstance(_REF[name], Exception):
            rng.assert_exhausted()
    return _REF[name]


def _same(got, want, who, circ, dkey):
    assert got == want, (who, circ["key"], dkey, "first differing 32-byte word", pc.first_difference(got, want))


def _check(ring, circ, wkey, advice, instances, dkey, draws, routes=((False, 0),), satisfied=False, device=False, twin=True):
    """native prover (every route) and Python twin (the first route) against the oracle: byte for byte"""
    want = _reference(circ, wkey, advice, instances, dkey, draws, satisfied)
    assert isinstance(want, bytes), want
    for i, (piece_cosets, split) in enumerate(routes):
        rng = draws()
        _same(ring.native(circ, advice, instances, rng, piece_cosets, split, device), want, ("native", "cosets" if piece_cosets else "extended", "split %d" % split), circ, dkey)
        if isinstance(rng, pc.PlantedRng) and rng.pattern is None:
            rng.assert_exhausted()                                    # item-addressed: the proof drew exactly its plan
        if isinstance(rng, pc.PlantedRng) and rng.pattern is not None:
            assert rng.planted_rejected > 0
        if twin and i == 0:
            rng = draws()
            _same(ring.twin(circ, advice, instances, rng, piece_cosets, split), want, "python twin", circ, dkey)
            if isinstance(rng, pc.PlantedRng) and rng.pattern is None:
                rng.assert_exhausted()
    return want


# ---- 2. planted draws on unsatisfied random circuits -----------------------------------------------------------------------------------------------------------------
DELTA = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R_MOD     # the one non-zero coefficient of a planted random polynomial


def planted(circ, plan, seed, m=1):
    """() -> a fresh PlantedRng for one of the draw plans of section 2"""
    cs, k = circ["cs"], circ["k"]
    if plan == "boundary":
        return lambda: pc.PlantedRng(seed, pattern=pc.BOUNDARY)
    ev = lambda purpose, fill: pc.every(cs, k, purpose, fill, m)
    fills = {"lookup_rows_zero": {**ev("bi", "zeros"), **ev("bt", "zeros")},                        # the extension rows of every permuted input and table are 0
             "product_rows_zero": {**ev("perm_blind", "zeros"), **ev("lookup_blind", "zeros")},     # the tails of every z are 0 (and the next set's last_z handoff follows)
             "product_rows_minus_one": {**ev("perm_blind", "minus_one"), **ev("lookup_blind", "minus_one")},
             "advice_rows_minus_one": ev("advice", "minus_one"),
             "random_poly_delta_first": {("random_poly", 0): ("delta_first", DELTA)},               # its commitment is [c] G
             "random_poly_delta_last": {("random_poly", 0): ("delta_last", DELTA)},
             "blinds_minus_one": ev("blind", "minus_one")}[plan]                                     # the discarded Blinds: r - 1 must change nothing but the stream's position
    assert fills, (plan, "plants nothing in", circ["key"])
    items = pc.draw_items(cs, k, m)
    return lambda: pc.PlantedRng.for_items(seed, items, fills)


PLANS = ("boundary", "lookup_rows_zero", "product_rows_zero", "product_rows_minus_one", "advice_rows_minus_one", "random_poly_delta_first", "random_poly_delta_last", "blinds_minus_one")
PLANTED_CASES = [(seed, plan) for seed in SEEDS for plan in PLANS if not (plan == "lookup_rows_zero" and not SEEDS[seed]["lookups"])]


def _planted(ring, k, seed, plan, twin=True):
    circ = random_case(k, seed)
    _check(ring, circ, "uniform", circ["advice"], circ["instances"], plan, planted(circ, plan, seed), twin=twin)


@pytest.mark.parametrize("seed,plan", PLANTED_CASES)
def test_planted_draws_emulated(emu_ring, orc, seed, plan):
    _planted(emu_ring, EMU_K[seed], seed, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,plan", PLANTED_CASES)
def test_planted_draws_gpu(gpu_ring, orc, seed, plan):
    _planted(gpu_ring, GPU_K[seed], seed, plan)


# ---- 3. structured witnesses on the same circuits, seeded draws ----------------------------------------------------------------------------------------------------------
def _seeded(seed):
    return lambda: np.random.default_rng(seed)


def _structured_advice(ring, orc, k, seed, kind, **kw):
    import pyref
    circ = random_case(k, seed)
    advice = pc.structured_advice(orc, pyref, circ["cs"], k, circ["advice"], kind, seed)
    return _check(ring, circ, ("advice", kind), advice, circ["instances"], "seeded", _seeded(seed), **kw)


@pytest.mark.parametrize("kind", pc.ADVICE_KINDS)
@pytest.mark.parametrize("seed", list(SEEDS))
def test_structured_advice_emulated(emu_ring, orc, seed, kind):
    _structured_advice(emu_ring, orc, EMU_K[seed], seed, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pc.ADVICE_KINDS)
@pytest.mark.parametrize("seed", list(SEEDS))
def test_structured_advice_gpu(gpu_ring, orc, seed, kind):
    _structured_advice(gpu_ring, orc, GPU_K[seed], seed, kind)


def _structured_lookups(ring, k, seed, kind):
    circ = random_case(k, seed)
    advice = pc.structured_lookup_inputs(circ["cs"], k, circ["fixed"], circ["advice"], kind)
    _check(ring, circ, ("lookup", kind), advice, circ["instances"], "seeded", _seeded(seed))


LOOKUP_CASES = [(seed, kind) for seed in SEEDS if SEEDS[seed]["lookups"] for kind in pc.LOOKUP_KINDS]


@pytest.mark.parametrize("seed,kind", LOOKUP_CASES)
def test_structured_lookup_inputs_emulated(emu_ring, orc, seed, kind):
    _structured_lookups(emu_ring, EMU_K[seed], seed, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kind", LOOKUP_CASES)
def test_structured_lookup_inputs_gpu(gpu_ring, orc, seed, kind):
    _structured_lookups(gpu_ring, GPU_K[seed], seed, kind)


def _structured_instances(ring, k, seed):
    """instance columns empty (all-zero columns through every transform), as long as the usable rows, and holding 0 and r - 1; one value too many is refused"""
    circ = random_case(k, seed)
    cs = circ["cs"]
    u, I = cs.usable_rows(k), cs.num_instance_columns
    rnd = np.random.default_rng(seed)
    full = [[int(v) for v in fr_int_array(rand_fr_array(rnd, u))] for _ in range(I)]
    for name, inst in (("empty", [[] for _ in range(I)]), ("usable", full), ("edges", [[0, R_MOD - 1, 0, R_MOD - 1][: 2 + c] for c in range(I)])):
        _check(ring, circ, "uniform", circ["advice"], inst, ("instances", name), _seeded(seed))
    long = [full[0] + [1]] + full[1:]
    raw = pc.RawCall(ring.be, ring.key(circ)[2], circ["advice"], long, np.random.default_rng(seed))
    assert raw.rc == ZK_ERR_ARG and raw.untouched()
    with pytest.raises(AssertionError):
        ring.twin(circ, circ["advice"], long, np.random.default_rng(seed))
    _check(ring, circ, "uniform", circ["advice"], full, ("instances", "usable"), _seeded(seed), twin=False)       # ... and the context is fine afterwards
    assert raw.draw_calls == raw.draw_calls_at_return


@pytest.mark.parametrize("seed", [3, 33])
def test_structured_instances_emulated(emu_ring, orc, seed):
    _structured_instances(emu_ring, EMU_K[seed], seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 7])
def test_structured_instances_gpu(gpu_ring, orc, seed):
    _structured_instances(gpu_ring, GPU_K[seed], seed)


def _device_and_side_lane(ring, orc, k, seed):
    """the advice device-resident; then the side lane (coefficient and extended forms on the helper context) forced on and off: all-zero instance columns, zero / constant /
    r - 1 advice columns go through both lanes; every proof the oracle's"""
    import pyref
    circ = random_case(k, seed)
    cs = circ["cs"]
    want = _structured_advice(ring, orc, k, seed, "mixed", device=True, twin=False)
    advice = pc.structured_advice(orc, pyref, cs, k, circ["advice"], "mixed", seed)
    empty = [[] for _ in range(cs.num_instance_columns)]
    proofs = []
    try:
        for mode in (2, 0):
            ring.be.tune(prover_side_lane=mode)
            assert ring.native(circ, advice, circ["instances"], np.random.default_rng(seed)) == want
            proofs.append(_check(ring, circ, ("advice", "zeros+empty"), pc.structured_advice(orc, pyref, cs, k, circ["advice"], "zeros", seed), empty, "seeded", _seeded(seed), twin=False))
    finally:
        ring.be.tune(prover_side_lane=1)
    assert proofs[0] == proofs[1]


def test_device_resident_advice_and_the_side_lane_emulated(emu_ring, orc):
    _device_and_side_lane(emu_ring, orc, EMU_K[7], 7)


@pytest.mark.gpu
def test_device_resident_advice_and_the_side_lane_gpu(gpu_ring, orc):
    _device_and_side_lane(gpu_ring, orc, GPU_K[7], 7)


def toy_case(k, extreme=None):
    return _circuit(("toy", k), k, lambda: tcp.toy_circuit(k)), tcp.toy_circuit(k, extreme=extreme)[3:]


def _two_circuits(ring, k):
    """one proof over two circuits of the toy key: circuit 0 structured (b = c = 0 on every row, both instances 0), circuit 1 the usual witness.  The twin is single-circuit
    (the whole two-circuit proof against the oracle's create_proof_multi: tests/test_oracle_multi_phased.py): twin and oracle pin the one-circuit form of the same entry point, and circuit 0's advice commitments, which open the two-circuit proof (its draws come first);
    the m-circuit verifier accepts the whole and holds it to both statements"""
    circ, (adv0, inst0) = toy_case(k, "zero_b")
    adv1, inst1 = circ["advice"], circ["instances"]
    _, pk, native = ring.key(circ, split=1)
    want0 = _check(ring, circ, "zero_b", adv0, inst0, "seeded", _seeded(k), routes=((False, 1),), satisfied=True)
    assert native.create_proof_multi([[a.copy() for a in adv0]], [inst0], np.random.default_rng(k)) == want0
    proof = native.create_proof_multi([[a.copy() for a in adv0], [a.copy() for a in adv1]], [inst0, inst1], np.random.default_rng(k))
    A = circ["cs"].num_advice_columns
    assert proof[: 32 * A] == want0[: 32 * A] and len(proof) == mv.proof_length(circ["cs"], 2)
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [inst0, inst1], proof) is True
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [inst1, inst0], proof) is False
    assert mv.verify_proof_multi(pk.vk, tcp.TAU, [inst0, [[inst1[0][0], (inst1[0][1] + 1) % R_MOD]]], proof) is False


def test_two_circuits_one_structured_emulated(emu_ring, orc):
    _two_circuits(emu_ring, 6)


@pytest.mark.gpu
def test_two_circuits_one_structured_gpu(gpu_ring, orc):
    _two_circuits(gpu_ring, 7)


# ---- 4. structured witnesses that satisfy their circuit, on the production routes ------------------------------------------------------------------------------------------
EXTENDED = ((False, 0), (False, 1))                                   # piece_cosets, quot_degree_split
BOTH = ((False, 0), (False, 1), (True, 0), (True, 1))


def _sgx_case(be, k, extreme):
    import os, sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    circ = _circuit(("sgx", k), k, lambda: sc.build(z, be, k) + ([],))
    return circ, (sc.build(z, be, k, extreme=extreme)[3], [])


def _satisfied_case(be, name, k, extreme):
    """-> (circuit, (advice, instances), routes)"""
    if name == "toy":                                                 # degree 5: four pieces on four cosets, the extended domain
        return toy_case(k, extreme) + (EXTENDED,)
    if name == "graded":                                              # degree 4: three pieces — the key keeps three cosets, or the extended domain
        circ = _circuit(("graded", k), k, lambda: tpc.graded_circuit(k, 1))
        return circ, tpc.graded_circuit(k, 1, extreme=extreme)[3:], BOTH
    if name == "sgx":
        return _sgx_case(be, k, extreme) + (EXTENDED,)
    seed = int(name[len("gates_off_"):])
    circ = _circuit(("gates_off", k, seed), k, lambda: pc.gates_off(k, seed))
    return circ, (circ["advice"], circ["instances"]), (BOTH if circ["cs"].degree() == 4 else EXTENDED)


def _satisfied(ring, name, k, extreme, plan):
    import verifier
    circ, (advice, instances), routes = _satisfied_case(ring.be, name, k, extreme)
    cs = circ["cs"]
    assert plonk.NativeMockProver.run(k, cs, circ["fixed"], advice, instances, circ["asm"], backend=ring.be).verify() == []
    draws = _seeded(k) if plan == "seeded" else planted(circ, plan, k)
    proof = _check(ring, circ, extreme, advice, instances, plan, draws, routes=routes, satisfied=True)
    _, keys = pc.oracle_keys(k, tcp.TAU, cs, circ["fixed"], circ["asm"], circ["key"])
    assert verifier.verify_proof(keys, tcp.TAU, instances, proof) is True
    if instances and instances[0]:
        wrong = [[(instances[0][0] + 1) % R_MOD] + list(instances[0][1:])] + [list(c) for c in instances[1:]]
        assert verifier.verify_proof(keys, tcp.TAU, wrong, proof) is False


# every route sees a boundary stream and an item-addressed one: extended (toy, sgx, gates_off_7) and by cosets (graded, gates_off_3), each with and without the degree split
SATISFIED_EMU = [("toy", 5, "zero_b", "boundary"), ("toy", 5, "max", "product_rows_zero"),
                 ("graded", 5, "zero_b", "advice_rows_minus_one"), ("graded", 5, "max", "boundary"),
                 ("sgx", 6, "zeros", "boundary"), ("sgx", 6, "max", "lookup_rows_zero"),
                 ("gates_off_3", 5, None, "boundary"), ("gates_off_3", 5, None, "product_rows_minus_one"), ("gates_off_7", 6, None, "lookup_rows_zero"), ("gates_off_2", 6, None, "boundary")]
SATISFIED_GPU = [(name, {5: 7, 6: 8}[k] if name != "sgx" else 6, extreme, plan) for name, k, extreme, plan in SATISFIED_EMU]


@pytest.mark.parametrize("name,k,extreme,plan", SATISFIED_EMU)
def test_satisfied_structured_witnesses_on_every_route_emulated(emu_ring, orc, name, k, extreme, plan):
    _satisfied(emu_ring, name, k, extreme, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,extreme,plan", SATISFIED_GPU)
def test_satisfied_structured_witnesses_on_every_route_gpu(gpu_ring, orc, name, k, extreme, plan):
    _satisfied(gpu_ring, name, k, extreme, plan)


def test_gates_off_circuits_keep_their_arguments():
    """switching the gates off leaves the lookups, the permutation columns and the copies of the random circuit in place (the arguments still run), on a witness MockProver accepts"""
    for k, seed in ((5, 3), (6, 7), (6, 2)):
        cs, fixed, asm, advice, instances = pc.gates_off(k, seed)
        cs0, _, asm0, _, _ = rc.random_circuit(k, seed)
        assert (len(cs.lookups), cs.permutation_columns, cs.degree(), asm.copies) == (len(cs0.lookups), cs0.permutation_columns, cs0.degree(), asm0.copies) and asm.copies
        plonk.MockProver.run(k, cs, fixed, advice, instances, asm).assert_satisfied()


# ---- 5. identity commitments: refused, explained, harmless --------------------------------------------------------------------------------------------------------------------
def _identity_case(circ, site, m=1):
    """-> (advice, fills, phase named in the refusal): exactly one commitment of the proof is the identity.  m = 2: the witness is circuit 1's, circuit 0 keeps the usual one"""
    cs, k = circ["cs"], circ["k"]
    A, L = cs.num_advice_columns, len(cs.lookups)
    advice = [a.copy() for a in circ["advice"]]
    if site == "random_poly":
        return advice, {("random_poly", 0): "zeros"}, "random polynomial"
    if site == "advice":                                              # a column that is zero on the usable rows, its blinding rows zero too
        col = pc.free_advice(cs)[-1]
        advice[col] = np.zeros_like(advice[col])
        return advice, {("advice", (m - 1) * A + col): "zeros"}, "advice"
    assert site == "permuted_input"                                   # the lookups' input is the table's zero row everywhere and its extension rows are zero
    advice = pc.structured_lookup_inputs(cs, k, circ["fixed"], advice, "zero_row")
    return advice, {("bi", (m - 1) * L): "zeros"}, "lookup permutation"                  # (of the first lookup: a second one keeps its seeded extension rows)


def _identity(ring, k, seed, site):
    circ = random_case(k, seed)
    cs = circ["cs"]
    advice, fills, phase = _identity_case(circ, site)
    items = pc.draw_items(cs, k)
    draws = lambda: pc.PlantedRng.for_items(seed, items, fills)
    ref = _reference(circ, ("identity", site), advice, circ["instances"], ("identity", site), draws)
    assert isinstance(ref, ValueError) and "infinity" in str(ref), ref
    with pytest.raises(ValueError, match="cannot write points at infinity"):
        ring.twin(circ, advice, circ["instances"], draws())
    _, _, native = ring.key(circ)
    ring.be.tune(quot_degree_split=0)
    try:
        raw = pc.RawCall(ring.be, native, advice, circ["instances"], draws())
    finally:
        ring.be.tune(quot_degree_split=1)
    assert raw.rc == ZK_ERR_ARG
    assert raw.untouched()                                            # no byte of the output buffer, and *proof_len as it was
    assert raw.error and "point at infinity" in raw.error and ("the %s phase" % phase) in raw.error, raw.error
    with pytest.raises(z.ZkError, match="point at infinity") as e:    # ... and what the binding raises says so
        ring.native(circ, advice, circ["instances"], draws())
    assert e.value.code == ZK_ERR_ARG
    # the next proof on the same context and key is the oracle's, before and after the context gave its per-proof buffers back
    _check(ring, circ, "uniform", circ["advice"], circ["instances"], "boundary", planted(circ, "boundary", seed), twin=False)
    ring.be.trim_pool()
    _check(ring, circ, "uniform", circ["advice"], circ["instances"], "boundary", planted(circ, "boundary", seed), twin=False)
    assert raw.draw_calls == raw.draw_calls_at_return                 # the refused proof's rng callback was not called again after its entry point returned


IDENTITY_CASES = [(3, "random_poly"), (3, "advice"), (3, "permuted_input"), (2, "random_poly"), (7, "permuted_input"), (33, "advice")]


@pytest.mark.parametrize("seed,site", IDENTITY_CASES)
def test_identity_commitment_is_refused_explained_and_harmless_emulated(emu_ring, orc, seed, site):
    _identity(emu_ring, EMU_K[seed], seed, site)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,site", IDENTITY_CASES)
def test_identity_commitment_is_refused_explained_and_harmless_gpu(gpu_ring, orc, seed, site):
    _identity(gpu_ring, GPU_K[seed], seed, site)


def _identity_in_circuit_one(ring, k, seed, site):
    """two circuits in one proof, the identity among circuit 1's commitments only"""
    circ = random_case(k, seed)
    cs = circ["cs"]
    advice1, fills, phase = _identity_case(circ, site, m=2)
    items = pc.draw_items(cs, k, m=2)
    _, _, native = ring.key(circ)
    flat_inst = list(circ["instances"]) + list(circ["instances"])
    ring.be.tune(quot_degree_split=0)
    try:
        raw = pc.RawCall(ring.be, native, list(circ["advice"]) + advice1, flat_inst, pc.PlantedRng.for_items(seed, items, fills), m=2)
        assert raw.rc == ZK_ERR_ARG and raw.untouched()
        assert "point at infinity" in raw.error and ("the %s phase" % phase) in raw.error, raw.error
        if site == "advice":                                          # the same zero blinding rows under circuit 1's usual, non-zero column: a proof, and it draws exactly its plan
            rng = pc.PlantedRng.for_items(seed, items, fills)
            ok = pc.RawCall(ring.be, native, list(circ["advice"]) * 2, flat_inst, rng, m=2)
            assert ok.rc == 0 and ok.len == mv.proof_length(cs, 2), (ok.rc, ok.error)
            rng.assert_exhausted()
    finally:
        ring.be.tune(quot_degree_split=1)
    _check(ring, circ, "uniform", circ["advice"], circ["instances"], "boundary", planted(circ, "boundary", seed), twin=False)
    assert raw.draw_calls == raw.draw_calls_at_return


@pytest.mark.parametrize("seed,site", [(3, "advice"), (3, "permuted_input"), (7, "random_poly")])
def test_identity_in_the_second_of_two_circuits_emulated(emu_ring, orc, seed, site):
    _identity_in_circuit_one(emu_ring, EMU_K[seed], seed, site)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,site", [(3, "advice"), (7, "permuted_input")])
def test_identity_in_the_second_of_two_circuits_gpu(gpu_ring, orc, seed, site):
    _identity_in_circuit_one(gpu_ring, GPU_K[seed], seed, site)
