"""TEST INFRASTRUCTURE ONLY — what tests/test_oracle_multi_phased.py shares: the reference of proofs over several circuits and of phased proofs (oracle/prover.py
create_proof_multi, computed once per case in the process), the order of a proof's random draws and of its transcript items written out from INTEGRATION.md §2c / §2e
(a third statement beside the native prover's plan and the oracle's in-place draws: it only ADDRESSES planted values and NAMES differing words), the planted constants,
and the builders of the four committed goldens (tools/gen_golden_proof.py writes them, the test regenerates them).
"""
import numpy as np

from zk_dcap_verifier_amd.fields import R_MOD, fr_int_array, fr_mont_array, rand_fr_array

import phased_cases as phc
import proof_cases as pc
import test_create_proof as tcp

R = R_MOD
TAU = tcp.TAU


def phase_lists(cs):
    ap = list(getattr(cs, "advice_column_phase", None) or [])
    ap += [0] * (cs.num_advice_columns - len(ap))
    return ap, list(getattr(cs, "challenge_phase", None) or [])


# ---- the draws of one proof, in stream order (§2c, §2e) ---------------------------------------------------------------------------------------------------------
PURPOSES = ("advice", "bi", "bt", "perm_blind", "lookup_blind")


def draw_items(cs, k, m=1):
    """[(purpose, index, count)]: per phase in use, per circuit, the blinding rows of the phase's columns in ascending index and then one Blind per column; per circuit and
    lookup the permuted input rows, the permuted table rows, two Blinds; per circuit its permutation sets (rows, Blind); per circuit its lookup products (rows, Blind);
    the random polynomial, its Blind and one Blind per piece of h(X).  Circuit c's item i of a purpose has index c * (items per circuit) + i, the Blinds are numbered in
    their order of appearance (proof_cases.draw_items' convention; for one single-phase circuit the two lists are equal)."""
    n, bf, A, L, S = 1 << k, cs.blinding_factors(), cs.num_advice_columns, len(cs.lookups), pc.n_sets(cs)
    phase_of, _ = phase_lists(cs)
    raw = []
    for phase in range(max(phase_of, default=0) + 1):
        cols = [i for i in range(A) if phase_of[i] == phase]
        for c in range(m):
            raw += [("advice", c * A + i, bf + 1) for i in cols] + [("blind", None, 1)] * len(cols)
    for c in range(m):
        for j in range(L):
            raw += [("bi", c * L + j, bf + 1), ("bt", c * L + j, bf + 1), ("blind", None, 1), ("blind", None, 1)]
    for c in range(m):
        for s in range(S):
            raw += [("perm_blind", c * S + s, bf), ("blind", None, 1)]
    for c in range(m):
        for j in range(L):
            raw += [("lookup_blind", c * L + j, bf), ("blind", None, 1)]
    raw += [("random_poly", 0, n), ("blind", None, 1)] + [("blind", None, 1)] * (cs.degree() - 1)
    out, b = [], 0
    for p, i, c in raw:
        if p == "blind":
            i, b = b, b + 1
        out.append((p, i, c))
    return out


def planted_constants(cs, k, m):
    """{(purpose, index): ("const", v)} — every item of every per-circuit purpose gets a constant of its own: circuit c's item j of purpose number q (PURPOSES) holds
    1000 c + 100 q + j + 1 on all its rows (q = 0, the advice blinding rows: 1000 c + j + 1), so that two blocks of equal size that changed places change the proof"""
    per = {"advice": cs.num_advice_columns, "bi": len(cs.lookups), "bt": len(cs.lookups), "perm_blind": pc.n_sets(cs), "lookup_blind": len(cs.lookups)}
    fills = {}
    for q, purpose in enumerate(PURPOSES):
        assert per[purpose] < 100
        for c in range(m):
            for j in range(per[purpose]):
                fills[purpose, c * per[purpose] + j] = ("const", 1000 * c + 100 * q + j + 1)
    assert len({v for _, v in fills.values()}) == len(fills) and all(0 < v < R for _, v in fills.values())
    return fills


def planted(cs, k, m, seed):
    """() -> a fresh item-addressed PlantedRng with planted_constants"""
    items, fills = draw_items(cs, k, m), planted_constants(cs, k, m)
    return lambda: pc.PlantedRng.for_items(seed, items, fills)


def boundary(seed):
    return lambda: pc.PlantedRng(seed, pattern=pc.BOUNDARY)


def seeded(seed):
    return lambda: np.random.default_rng(seed)


# ---- the 32-byte words of one proof, by name (§2c transcript order; §2e for the advice commitments) -------------------------------------------------------------------
def transcript_items(cs, m, multiopen="shplonk"):
    """multiopen = "gwc": the items up to the last evaluation; the words after them are the W_i, one per opening point (same_proof names them by their number)"""
    A, L, S = cs.num_advice_columns, len(cs.lookups), pc.n_sets(cs)
    phase_of, _ = phase_lists(cs)
    out = []
    for phase in range(max(phase_of, default=0) + 1):
        for c in range(m):
            out += ["advice commitment: phase %d, circuit %d, column %d" % (phase, c, i) for i in range(A) if phase_of[i] == phase]
    for c in range(m):
        for j in range(L):
            out += ["permuted input commitment: circuit %d, lookup %d" % (c, j), "permuted table commitment: circuit %d, lookup %d" % (c, j)]
    out += ["permutation product commitment: circuit %d, set %d" % (c, s) for c in range(m) for s in range(S)]
    out += ["lookup product commitment: circuit %d, lookup %d" % (c, j) for c in range(m) for j in range(L)]
    out += ["random polynomial commitment"] + ["h piece %d commitment" % i for i in range(cs.degree() - 1)]
    out += ["advice evaluation: circuit %d, query %r" % (c, q) for c in range(m) for q in cs.advice_queries()]
    out += ["fixed evaluation: query %r" % (q,) for q in cs.fixed_queries()] + ["random polynomial evaluation"]
    out += ["sigma evaluation %d" % j for j in range(len(cs.permutation_columns))]
    for c in range(m):
        for s in range(S):
            out += ["permutation evaluation: circuit %d, set %d, %s" % (c, s, what) for what in (("z", "z_next", "z_last") if s + 1 < S else ("z", "z_next"))]
    for c in range(m):
        for j in range(L):
            out += ["lookup evaluation: circuit %d, lookup %d, %s" % (c, j, what) for what in ("z", "z_next", "a", "a_inv", "s")]
    return out + (["SHPLONK h1", "SHPLONK h2"] if multiopen == "shplonk" else [])


def same_proof(got, want, cs, m, who, multiopen="shplonk"):
    """byte equality; on a mismatch the first differing 32-byte word and the transcript item it is"""
    if got != want:
        word = pc.first_difference(got, want)
        items = transcript_items(cs, m, multiopen)
        name = items[word] if isinstance(word, int) and word < len(items) else None
        if multiopen == "gwc" and isinstance(word, int) and word >= len(items):
            name = "GWC witness W_%d (group %d in order of first appearance)" % (word - len(items), word - len(items))
        raise AssertionError((who, "first differing 32-byte word", word, name))


# ---- the reference: once per (circuit, witness, draws) in the process, shared by both backends --------------------------------------------------------------------------
_REF, _OPENING = {}, {}


def ints(col):
    import oracle as orc
    return None if col is None else (orc.fr_to_ints(col) if isinstance(col, np.ndarray) else [int(v) for v in col])


def oracle_callback(case):
    """phased_cases' later-phase synthesis as the oracle takes it: canonical ints"""
    def fn(phase, challenges, circuit):
        w = case.witness(challenges, circuit)
        return {i: w[i] for i in range(len(w)) if case.phase_of[i] == phase}
    return fn


def reference(name, k, cs, fixed, asm, key, advices, instances_list, draws, next_phase=None, satisfied=True, multiopen="shplonk", opening=None):
    """-> (proof bytes, squeezed challenges, the oracle's Keys) of the independent CPU prover; an item-addressed stream must end where the oracle's own order ends.
    multiopen = "gwc": the proof that ends with ProverGWC (cached under its own name); opening, a dict, receives what the oracle's argument made of the queries."""
    import prover as op
    if multiopen != "shplonk":
        name = (name, multiopen)
    if name not in _REF:
        params, keys = pc.oracle_keys(k, TAU, cs, fixed, asm, key)
        rng, squeezed, made = draws(), [], {}
        proof = op.create_proof_multi(params, keys, [[ints(a) for a in adv] for adv in advices], instances_list, rng, next_phase=next_phase,
                                      require_satisfied=satisfied, challenges_out=squeezed, multiopen=multiopen, opening_out=made)
        if isinstance(rng, pc.PlantedRng) and rng.pattern is None:
            rng.assert_exhausted()
        _REF[name] = (proof, squeezed, keys)
        _OPENING[name] = made
    if opening is not None:
        opening.update(_OPENING[name])
    return _REF[name]


def assert_no_identity(cs, k, advices, fills=None):
    """from the inputs: no advice column is committed as the identity — it holds a non-zero usable row, or its blinding rows are not planted with zeros (seeded rows
    and the constants of planted_constants are non-zero); the native prover refuses the identity by design, elsewhere"""
    u, A = cs.usable_rows(k), cs.num_advice_columns
    for c, adv in enumerate(advices):
        for i, col in enumerate(adv):
            if col is None:
                continue
            rows = np.asarray(col)[:u]
            assert rows.any() or (fills or {}).get(("advice", c * A + i)) not in ("zeros", ("const", 0)), ("circuit", c, "column", i, "would be committed as the identity")


# ---- witnesses ----------------------------------------------------------------------------------------------------------------------------------------------------------
def toy_pair(k, kinds, instances="usual"):
    """m witnesses of tcp.toy_circuit(k)'s key: kind c is ("shift", c) -> test_multi_circuit.toy_witness(k, s=c, t=2c), or one of toy_circuit's extremes (None: the usual
    witness).  instances = "empty_full": circuit 0 (which must be zero_b: its copied cells are 0) gets an empty instance column, the last circuit one as long as the
    usable rows (its first two values are the copied ones, the rest seeded: no gate reads them)."""
    import test_multi_circuit as tmc
    advices, insts = [], []
    for kind in kinds:
        if isinstance(kind, tuple):
            adv, inst = tmc.toy_witness(k, s=kind[1], t=2 * kind[1])
        else:
            adv, inst = tcp.toy_circuit(k, extreme=kind)[3:]
        advices.append(adv)
        insts.append([list(col) for col in inst])
    if instances == "empty_full":
        cs = tcp.toy_circuit(k)[0]
        assert kinds[0] == "zero_b" and insts[0] == [[0, 0]]
        insts[0] = [[]]
        extra = fr_int_array(rand_fr_array(np.random.default_rng(k), cs.usable_rows(k) - 2))
        insts[-1] = [insts[-1][0] + [int(v) for v in extra]]
    return advices, insts


def shifted_copy(cs, advice, constant=12345):
    """circuit 0's witness with the first advice column that feeds no lookup shifted by a constant (the lookups' inputs stay in their tables)"""
    col = pc.free_advice(cs)[0]
    out = [a.copy() for a in advice]
    out[col] = fr_mont_array([(v + constant) % R for v in fr_int_array(advice[col])])
    return out


# ---- the committed goldens: (file, builder); builder() -> (reference(..) result, cs, instances_list, phased) ----------------------------------------------------------------
def golden_toy_m2():
    k = 6
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    advices, insts = toy_pair(k, [("shift", 0), ("shift", 1)])
    return reference(("toy", k, "shift2", "seeded5"), k, cs, fixed, asm, ("toy", k), advices, insts, seeded(5)), cs, insts, False


def golden_phased(name):
    def build():
        case = phc.CASES[name](6)
        ref = reference(("phased", name, 6, "seeded5"), 6, case.cs, case.fixed, case.asm, ("phased", name, 6), case.phase0(), case.instances, seeded(5),
                        next_phase=oracle_callback(case))
        return ref, case.cs, case.instances, True
    return build


GOLDENS = [("toy_m2_k6_seed5.bin", golden_toy_m2), ("phased_A_k6_seed5.bin", golden_phased("A")), ("phased_B_k6_seed5.bin", golden_phased("B")),
           ("phased_D_k6_seed5.bin", golden_phased("D"))]
