"""TEST INFRASTRUCTURE ONLY — the circuits, witnesses and draws of tests/test_gwc.py and tests/test_oracle_gwc.py: proofs that end with halo2's GWC multi-open instead
of SHPLONK.

Reused as they are: tcp.toy_circuit and the sgx-shaped circuit (tools/sgx_shaped_circuit.py) with the seeds of their committed goldens, multi_phase_cases' toy pairs
(m = 2 with its golden, m = 3) and phased_cases' circuit A (golden).  Three circuits of this file give the grouping by point something to get wrong:

  rot0      one gate, every query at rotation 0, no permutation, no lookup: every query opens at x, so P = 1 and the one combination has every polynomial of the proof
  rot8      one advice column read at rotations -3, -2, 0, 2, 3, 5 and a permutation over two sets (x_next, x_last): eight distinct opening points
  unsorted  the FIRST advice query has rotation 2 and the second rotation -1: the first-appearance order of the points starts omega^2 x, omega^-1 x, x, omega x.  SHPLONK
            sorts its point sets by canonical value, GWC must not; the test asserts that the order this proof's x gives is not the ascending one.
  alias     (test_oracle_gwc.py only) rotations 1 and 1 - n of one column: one cell, one point, two queries — see alias() below; the bare circuit is refused by every
            prover (a zero piece of h(X)), alias_eq — one more equality-enabled column — proves.

Every case is (cs, fixed, asm, advices, instances_list, seed): advices[c] circuit c's columns as (n, 4) Montgomery arrays (None for later-phase columns), the rng of every
proof np.random.default_rng(seed) — a fresh one per proof, so the SHPLONK and the GWC proof of a case are made from the same draws.
"""
import os
import sys

import numpy as np

from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.fields import R_MOD, fr_mont_array
from zk_dcap_verifier_amd.plonk import ADVICE, Advice, Fixed

import multi_phase_cases as mpc
import phased_cases as phc
import test_create_proof as tcp

TAU = tcp.TAU


class GwcCase:
    def __init__(self, name, k, cs, fixed, asm, advices, instances_list, seed, golden=None, phased=None, min_points=None, points=None):
        """golden: the committed SHPLONK proof (Blake2b) of the same inputs and draws; phased: the phased_cases.Case whose later phases the prover asks for;
        points / min_points: the number of distinct opening points the circuit must give"""
        self.name, self.k, self.cs, self.fixed, self.asm, self.advices, self.instances_list, self.seed = name, k, cs, fixed, asm, advices, instances_list, seed
        self.golden, self.phased, self.min_points, self.points = golden, phased, min_points, points
        self.m = len(advices)

    def rng(self):
        return np.random.default_rng(self.seed)

    def host_advices(self):
        return [[None if a is None else a.copy() for a in adv] for adv in self.advices]


def _no_copies(cs, k):
    asm = plonk.Assembly(cs, k)
    asm.copies = []
    return asm


def rot0(k=7):
    n = 1 << k
    cs = plonk.ConstraintSystem(num_fixed_columns=1, num_advice_columns=3, num_instance_columns=0)
    cs.create_gate(Fixed(0) * (Advice(0) * Advice(1) - Advice(2)))
    u = cs.usable_rows(k)
    rnd = np.random.default_rng(70)
    A = [int(v) for v in rnd.integers(1, 1 << 60, n)]
    B = [int(v) for v in rnd.integers(1, 1 << 60, n)]
    C = [a * b % R_MOD for a, b in zip(A, B)]
    assert not cs.permutation_columns and not cs.lookups and {r for _, r in cs.advice_queries() + cs.fixed_queries()} == {0}
    return GwcCase("rot0", k, cs, [[1 if i < u else 0 for i in range(n)]], _no_copies(cs, k), [[fr_mont_array(c) for c in (A, B, C)]], [[]], seed=11, points=1)


ROTATIONS = (-3, -2, 0, 2, 3, 5)


def rot8(k=7):
    n = 1 << k
    cs = plonk.ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0)
    total = Advice(0, ROTATIONS[0])
    for r in ROTATIONS[1:]:
        total = total + Advice(0, r)
    cs.create_gate(Fixed(0) * (total - Advice(1)))
    cs.enable_equality(ADVICE, 0)
    cs.enable_equality(ADVICE, 1)
    u = cs.usable_rows(k)
    A = [int(v) for v in np.random.default_rng(71).integers(1, 1 << 60, n)]
    A[20] = A[4]
    Q = [1 if 3 <= i < u - 5 else 0 for i in range(n)]               # no rotation of an active row leaves the usable rows
    B = [sum(A[i + r] for r in ROTATIONS) % R_MOD if Q[i] else 9 for i in range(n)]
    asm = _no_copies(cs, k)
    asm.copy((ADVICE, 0, 4), (ADVICE, 0, 20))
    asm.copy((ADVICE, 1, 1), (ADVICE, 1, 2))                          # both 9: rows the gate does not read
    assert {r for _, r in cs.advice_queries()} == set(ROTATIONS)
    assert cs.permutation_chunk_len() == 1                            # degree 3: one column per permutation set, so the first set is also opened at x_last
    return GwcCase("rot8", k, cs, [Q], asm, [[fr_mont_array(A), fr_mont_array(B)]], [[]], seed=12, points=len(ROTATIONS) + 2)


def unsorted(k=9):
    n = 1 << k
    cs = plonk.ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0)
    cs.create_gate(Fixed(0) * (Advice(0, 2) - Advice(1, -1) - Advice(0) - 1))
    cs.enable_equality(ADVICE, 1)
    u = cs.usable_rows(k)
    assert cs.advice_queries()[:3] == [(0, 2), (1, -1), (0, 0)]
    Q = [1 if 1 <= i < u - 2 else 0 for i in range(n)]
    B = [int(v) for v in np.random.default_rng(72).integers(1, 1 << 60, n)]
    B[8] = B[3]
    A = [0] * n
    A[0], A[1], A[2] = 5, 6, 7
    for i in range(1, u - 2):                                          # a[i + 2] = a[i] + b[i - 1] + 1
        A[i + 2] = (A[i] + B[i - 1] + 1) % R_MOD
    asm = _no_copies(cs, k)
    asm.copy((ADVICE, 1, 3), (ADVICE, 1, 8))
    return GwcCase("unsorted", k, cs, [Q], asm, [[fr_mont_array(A), fr_mont_array(B)]], [[]], seed=13, points=4)      # omega^2 x, omega^-1 x, x, omega x


def alias(k=5, eq=False):
    """rotations 1 and 1 - n of advice column 0 name the same cell and the same point omega x, and stay two queries with two (equal) evaluations: GWC's group at
    omega x, the first one, holds that column's polynomial twice, with v^0 and v^1 — a prover that merges equal (polynomial, point) queries writes another W_0; SHPLONK
    holds the polynomial once, in the set {omega x}.
    eq = False: the bare circuit — one gate of degree 2, no permutation, no lookup.  Its numerator has degree < 2n, so the second of the cs.degree() - 1 = 2 pieces of
    h(X) is the zero polynomial and its commitment the identity, which no transcript absorbs: every prover REFUSES this circuit, as halo2 does (the test asserts the
    message, layer by layer).  The opening points would be omega x and x.
    eq = True ("alias_eq": what separates it from alias is one equality-enabled column): advice column 1 is equality-enabled as well, with one copy.  The advice queries
    are the same three — (1, 0) is the query the gate made already — the permutation argument's degree-3 identity fills the second piece of h(X), and the product
    polynomial is opened at x and omega x, the two points there were: P = 2, the group at omega x is still the first."""
    n = 1 << k
    cs = plonk.ConstraintSystem(num_fixed_columns=1, num_advice_columns=2, num_instance_columns=0)
    cs.create_gate(Fixed(0) * (Advice(0, 1) + Advice(0, 1 - n) - Advice(1)))
    if eq:
        cs.enable_equality(ADVICE, 1)
    u = cs.usable_rows(k)
    assert cs.advice_queries() == [(0, 1), (0, 1 - n), (1, 0)]
    assert cs.permutation_columns == ([(ADVICE, 1)] if eq else []) and not cs.lookups and cs.degree() == 3
    Q = [1 if i + 1 < u else 0 for i in range(n)]                     # the row after an active row is a usable one
    A = [int(v) for v in np.random.default_rng(73).integers(1, 1 << 60, n)]
    A[9] = A[4]
    B = [2 * A[i + 1] % R_MOD if Q[i] else 9 for i in range(n)]       # b[i] = a[i + 1] + a[i + 1 - n]: one cell read twice
    asm = _no_copies(cs, k)
    if eq:
        asm.copy((ADVICE, 1, 3), (ADVICE, 1, 8))                      # b[3] = 2 a[4] = 2 a[9] = b[8]
    return GwcCase("alias_eq" if eq else "alias", k, cs, [Q], asm, [[fr_mont_array(A), fr_mont_array(B)]], [[]], seed=14, points=2)      # omega x, x


def toy(k=6):
    cs, fixed, asm, advice, instances = tcp.toy_circuit(k)
    return GwcCase("toy", k, cs, fixed, asm, [advice], [instances], seed=7, golden=tcp.GOLDEN_PROOF if k == 6 else None, min_points=4)


def toy_m(m, k=6):
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    advices, insts = mpc.toy_pair(k, [("shift", c) for c in range(m)])
    return GwcCase("toy_m%d" % m, k, cs, fixed, asm, advices, insts, seed=5, golden="toy_m2_k6_seed5.bin" if (m, k) == (2, 6) else None, min_points=4)


def phased_a(k=6):
    case = phc.CASES["A"](k)
    return GwcCase("phased_A", k, case.cs, case.fixed, case.asm, case.phase0(), case.instances, seed=5, golden="phased_A_k6_seed5.bin" if k == 6 else None, phased=case, min_points=3)


def sgx_shaped(be, k=8):
    """needs a backend: tools/sgx_shaped_circuit.py builds its witness through the library"""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    import zk_dcap_verifier_amd as z
    cs, fixed, asm, advice = sc.build(z, be, k)
    return GwcCase("sgx_shaped", k, cs, fixed, asm, [advice], [[]], seed=3, golden=tcp.GOLDEN_SGX if k == 8 else None, min_points=4)


CASES = {"toy": lambda be: toy(), "sgx_shaped": sgx_shaped, "toy_m2": lambda be: toy_m(2), "toy_m3": lambda be: toy_m(3), "phased_A": lambda be: phased_a(),
         "rot0": lambda be: rot0(), "rot8": lambda be: rot8(), "unsorted": lambda be: unsorted()}


# ---- the same cases at a size of the caller's choice, and their reference (tests/test_oracle_gwc.py) ----------------------------------------------------------------------------
BUILDERS = {"toy": lambda be, k: toy(k), "sgx_shaped": sgx_shaped, "toy_m2": lambda be, k: toy_m(2, k), "toy_m3": lambda be, k: toy_m(3, k),
            "phased_A": lambda be, k: phased_a(k), "rot0": lambda be, k: rot0(k), "rot8": lambda be, k: rot8(k), "unsorted": lambda be, k: unsorted(k)}
assert set(BUILDERS) == set(CASES)


def oracle_key(case):
    """the name under which proof_cases.oracle_keys keeps this circuit's keys: the toy and the phased circuits share theirs with tests/test_oracle_multi_phased.py"""
    if case.name in ("toy", "toy_m2", "toy_m3"):
        return ("toy", case.k)
    if case.phased is not None:
        return ("phased", case.phased.name, case.k)
    return ("gwc", case.name, case.k)


def reference(case, multiopen="gwc", opening=None):
    """-> (proof bytes, squeezed challenges, the oracle's Keys): oracle/prover.py on the case's inputs and draws, ending with `multiopen`; once per process"""
    return mpc.reference(("gwc_cases", case.name, case.k, case.seed), case.k, case.cs, case.fixed, case.asm, oracle_key(case), case.advices, case.instances_list,
                         mpc.seeded(case.seed), next_phase=mpc.oracle_callback(case.phased) if case.phased is not None else None, multiopen=multiopen, opening=opening)


# the committed GWC goldens (tools/gen_golden_proof.py writes them from the oracle, Blake2b): (file, the case's builder)
GOLDENS = [("toy_gwc_k6_seed7.bin", toy), ("toy_m2_gwc_k6_seed5.bin", lambda: toy_m(2)), ("phased_A_gwc_k6_seed5.bin", phased_a), ("alias_eq_gwc_k5.bin", lambda: alias(5, eq=True))]
