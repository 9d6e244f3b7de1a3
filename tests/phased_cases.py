"""TEST INFRASTRUCTURE ONLY — satisfiable circuits with advice in several phases whose later-phase witness is a function of the challenges (tests/test_phased.py).

A  two phases: phase-0 advice a, b; challenge c0 after phase 0; phase-1 advice acc (the running random linear combination of a: acc_0 = a_0, acc_{r+1} = acc_r c0 + a_{r+1})
   and acc2 (a copy of acc); gates q_first (acc - a) and q (acc_next - acc c0 - a_next); a lookup whose input a c0 + b and table t1 c0 + t2 both hold the
   challenge; copy constraints a[0] = acc[0] (phase 0 with phase 1) and acc[r] = acc2[r] for two rows (two phase-1 columns).
B  three phases, a gate of degree 5 (four pieces of h(X): the key keeps its extended forms): a in phase 0, c0 after it; b1 = a c0 in phase 1, c1 and c2 after it (two challenges of
   one phase: their squeeze order is pinned); d = b1 c1 + c2 = a c0 c1 + c2 and e = d in phase 2; c3 after the last phase, in a gate only.
C  A with the phase-1 columns at indices 0, 1 and the phase-0 columns after them: the commitment order is not the index order.
D  A over m = 2 circuits with different witnesses.
k = 6 unless said otherwise: 58 usable rows at the minimum blinding of 5."""
import numpy as np

from zk_dcap_verifier_amd import plonk
from zk_dcap_verifier_amd.plonk import ADVICE, Advice, Fixed
from zk_dcap_verifier_amd.fields import R_MOD, fr_mont_array


class Case:
    """cs, fixed, asm: what keygen takes.  witness(challenges, circuit, tamper) -> every advice column as canonical ints, from the final challenge values;
    columns of phase p depend on the challenges of earlier phases only."""

    def __init__(self, name, k, m, cs, fixed, asm, witness):
        self.name, self.k, self.m, self.cs, self.fixed, self.asm, self._witness = name, k, m, cs, fixed, asm, witness
        self.phase_of = cs._advice_phases()
        self.instances = [[] for _ in range(m)]

    def witness(self, challenges, circuit=0, tamper=None):
        return self._witness(list(challenges), circuit, tamper)

    def columns(self, challenges, circuit, phase, tamper=None):
        """{column: (n, 4) Montgomery array} of one phase"""
        w = self.witness(challenges, circuit, tamper)
        return {i: fr_mont_array(w[i]) for i in range(len(w)) if self.phase_of[i] == phase}

    def phase0(self, tamper=None):
        """advices[c][column] for the prover's entry: phase-0 columns, None for the others"""
        zeros = [0] * self.cs.num_challenges
        out = []
        for c in range(self.m):
            cols = self.columns(zeros, c, 0, tamper)
            out.append([cols.get(i) for i in range(self.cs.num_advice_columns)])
        return out

    def next_phase(self, tamper=None, shift=0):
        """the caller's synthesis of the later phases; shift: added to every challenge before the witness is computed (a prover that ignores the transcript)"""
        def fn(phase, challenges, circuit=0):
            return self.columns([(c + shift) % R_MOD for c in challenges], circuit, phase, tamper)
        return fn


def _rlc_circuit(k, order, m, name, single_phase=False):
    """A / C / D.  order: the column indices of (a, b, acc, acc2).  single_phase: the same columns, gates, lookup and copies with every column in phase 0 and the
    constant 7 in c0's place (the single-phase proof of the same column count that timings are set beside)"""
    n = 1 << k
    ia, ib, iacc, iacc2 = order
    cs = plonk.ConstraintSystem(num_fixed_columns=4)
    # (halo2 hands out indices in call order and refuses a phase-1 column before a phase-0 one exists, so C's layout cannot come from advice_column_in calls in index
    #  order: the lists are filled the way ConstraintSystem stores them)
    cs.num_advice_columns = 4
    cs.advice_column_phase = [0] * 4
    if single_phase:
        cs.advice_column_phase = []
        c0 = plonk.Constant(7)
    else:
        cs.advice_column_phase[iacc] = cs.advice_column_phase[iacc2] = 1
        c0 = cs.challenge_usable_after(0)
    a, b, acc, acc2 = Advice(ia), Advice(ib), Advice(iacc), Advice(iacc2)
    q_first, q, t1, t2 = Fixed(0), Fixed(1), Fixed(2), Fixed(3)
    cs.create_gate(q_first * (acc - a))
    cs.create_gate(q * (Advice(iacc, 1) - acc * c0 - Advice(ia, 1)))
    cs.lookup([(a * c0 + b, t1 * c0 + t2)])
    for col in (ia, iacc, iacc2):
        cs.enable_equality(ADVICE, col)
    u = cs.usable_rows(k)
    assert cs.blinding_factors() == 5 and cs.degree() == 4 and (k != 6 or u == 58)

    def ab(circuit):
        rng = np.random.default_rng(100 + circuit)
        return [int(v) for v in rng.integers(1, 1 << 40, n)], [int(v) for v in rng.integers(1, 1 << 40, n)]
    A0, B0 = ab(0)
    rows = [(A0[r], B0[r]) for r in range(u)]                        # the table: circuit 0's tuples (a_r, b_r), r < u, in reversed order
    T1 = [rows[u - 1 - r][0] if r < u else 0 for r in range(n)]
    T2 = [rows[u - 1 - r][1] if r < u else 0 for r in range(n)]
    fixed = [[1] + [0] * (n - 1), [1 if r + 1 < u else 0 for r in range(n)], T1, T2]
    asm = plonk.Assembly(cs, k)
    asm.copies = []                                                   # logged for the independent CPU prover (oracle/prover.py)
    asm.copy((ADVICE, ia, 0), (ADVICE, iacc, 0))
    asm.copy((ADVICE, iacc, 3), (ADVICE, iacc2, 3))
    asm.copy((ADVICE, iacc2, 10), (ADVICE, iacc, 10))

    def witness(ch, circuit, tamper):
        ch = [7] if single_phase else ch
        # circuit c > 0: circuit 0's (a, b) tuples rotated by 7 c rows — a different witness whose lookup inputs are still in the table
        s = (7 * circuit) % u
        A = [A0[(r + s) % u] if r < u else 0 for r in range(n)]
        B = [B0[(r + s) % u] if r < u else 0 for r in range(n)]
        if tamper == "lookup":
            B[4] = (B[4] + 1000) % R_MOD
        acc_ = [0] * n
        acc_[0] = A[0]
        for r in range(1, u):
            acc_[r] = (acc_[r - 1] * ch[0] + A[r]) % R_MOD
        acc2_ = list(acc_)
        if tamper == "acc":
            acc_[u - 1] = (acc_[u - 1] + 1) % R_MOD                   # the last usable row: only gate 1 on row u - 2 reads it
        cols = [None] * 4
        cols[ia], cols[ib], cols[iacc], cols[iacc2] = A, B, acc_, acc2_
        return cols
    return Case(name, k, m, cs, fixed, asm, witness)


def case_a(k=6):
    return _rlc_circuit(k, (0, 1, 2, 3), 1, "A")


def case_a_single_phase(k=6):
    return _rlc_circuit(k, (0, 1, 2, 3), 1, "A1", single_phase=True)


def case_c(k=6):
    return _rlc_circuit(k, (2, 3, 0, 1), 1, "C")


def case_d(k=6):
    return _rlc_circuit(k, (0, 1, 2, 3), 2, "D")


def case_b(k=6):
    n = 1 << k
    cs = plonk.ConstraintSystem(num_fixed_columns=1)
    ia = cs.advice_column_in(0)
    c0 = cs.challenge_usable_after(0)
    ib1 = cs.advice_column_in(1)
    c1 = cs.challenge_usable_after(1)
    c2 = cs.challenge_usable_after(1)
    idd = cs.advice_column_in(2)
    ie = cs.advice_column_in(2)
    c3 = cs.challenge_usable_after(2)
    a, b1, d = Advice(ia), Advice(ib1), Advice(idd)
    q = Fixed(0)
    cs.create_gate(q * (b1 - a * c0))
    cs.create_gate(q * (d - a * (c0 * c1) - c2))
    cs.create_gate(q * c3 * (a * a * a) * (d - b1 * c1 - c2))          # degree 5: four pieces of h(X), none of them zero
    for col in (idd, ie):
        cs.enable_equality(ADVICE, col)
    u = cs.usable_rows(k)
    assert cs.degree() == 5 and cs.phases() == [0, 1, 2] and cs.challenge_phase == [0, 1, 1, 2]
    fixed = [[1 if r < u else 0 for r in range(n)]]
    asm = plonk.Assembly(cs, k)
    asm.copies = []                                                   # logged for the independent CPU prover (oracle/prover.py)
    asm.copy((ADVICE, idd, 2), (ADVICE, ie, 2))
    asm.copy((ADVICE, ie, 9), (ADVICE, idd, 9))
    A = [int(v) for v in np.random.default_rng(200).integers(1, 1 << 40, n)]

    def witness(ch, circuit, tamper):
        B1 = [v * ch[0] % R_MOD for v in A]
        D = [(v * ch[1] + ch[2]) % R_MOD for v in B1]
        return [A, B1, D, list(D)]
    return Case("B", k, 1, cs, fixed, asm, witness)


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d}
