"""TEST INFRASTRUCTURE ONLY — the circuits, witnesses and draws of tests/test_gwc.py: proofs that end with halo2's GWC multi-open instead of SHPLONK.

Reused as they are: tcp.toy_circuit and the sgx-shaped circuit (tools/sgx_shaped_circuit.py) with the seeds of their committed goldens, multi_phase_cases' toy pairs
(m = 2 with its golden, m = 3) and phased_cases' circuit A (golden).  Three circuits of this file give the grouping by point something to get wrong:

  rot0      one gate, every query at rotation 0, no permutation, no lookup: every query opens at x, so P = 1 and the one combination has every polynomial of the proof
  rot8      one advice column read at rotations -3, -2, 0, 2, 3, 5 and a permutation over two sets (x_next, x_last): eight distinct opening points
  unsorted  the FIRST advice query has rotation 2 and the second rotation -1: the first-appearance order of the points starts omega^2 x, omega^-1 x, x, omega x.  SHPLONK
            sorts its point sets by canonical value, GWC must not; the test asserts that the order this proof's x gives is not the ascending one.

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


def toy(k=6):
    cs, fixed, asm, advice, instances = tcp.toy_circuit(k)
    return GwcCase("toy", k, cs, fixed, asm, [advice], [instances], seed=7, golden=tcp.GOLDEN_PROOF, min_points=4)


def toy_m(m, k=6):
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    advices, insts = mpc.toy_pair(k, [("shift", c) for c in range(m)])
    return GwcCase("toy_m%d" % m, k, cs, fixed, asm, advices, insts, seed=5, golden="toy_m2_k6_seed5.bin" if m == 2 else None, min_points=4)


def phased_a(k=6):
    case = phc.CASES["A"](k)
    return GwcCase("phased_A", k, case.cs, case.fixed, case.asm, case.phase0(), case.instances, seed=5, golden="phased_A_k6_seed5.bin", phased=case, min_points=3)


def sgx_shaped(be, k=8):
    """needs a backend: tools/sgx_shaped_circuit.py builds its witness through the library"""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sgx_shaped_circuit as sc
    import zk_dcap_verifier_amd as z
    cs, fixed, asm, advice = sc.build(z, be, k)
    return GwcCase("sgx_shaped", k, cs, fixed, asm, [advice], [[]], seed=3, golden=tcp.GOLDEN_SGX, min_points=4)


CASES = {"toy": lambda be: toy(), "sgx_shaped": sgx_shaped, "toy_m2": lambda be: toy_m(2), "toy_m3": lambda be: toy_m(3), "phased_A": lambda be: phased_a(),
         "rot0": lambda be: rot0(), "rot8": lambda be: rot8(), "unsorted": lambda be: unsorted()}
