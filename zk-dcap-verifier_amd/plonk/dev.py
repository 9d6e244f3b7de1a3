"""halo2_proofs::dev::MockProver — the constraint check the reference runs before proving
(`MockProver::run(k, &circuit, vec![]).unwrap().assert_satisfied()`, circuits/src/sgx_dcap_verifier.rs:790-794).

Host-only and O(rows x constraints) in Python integers: meant for the small circuits of the tests, exactly as MockProver is
meant for debugging — it bypasses the commitment scheme (and therefore the GPU path) completely."""
from __future__ import annotations

from collections import namedtuple
from typing import List, Sequence

import numpy as np

from ..fields import R_MOD, fr_int_array, fr_mont_array
from . import expression as ex
from .circuit import ADVICE, FIXED, INSTANCE, Assembly, ConstraintSystem


class VerifyFailure(Exception):
    pass


class MockProver:
    def __init__(self, k: int, cs: ConstraintSystem, fixed: Sequence, advice: Sequence, instances: Sequence[Sequence[int]], assembly: Assembly | None = None,
                 challenges: Sequence[int] | None = None):
        self.k, self.n, self.cs, self.assembly = k, 1 << k, cs, assembly
        self.challenges = None if challenges is None else [int(c) % R_MOD for c in challenges]     # the values of cs's user challenges (halo2's MockProver derives its own)
        conv = lambda c: [int(v) % R_MOD for v in c] if not hasattr(c, "dtype") else fr_int_array(c)
        self.fixed = [conv(c) for c in fixed]
        self.advice = [conv(c) for c in advice]
        self.instance = [list(c) + [0] * (self.n - len(c)) for c in instances]

    @classmethod
    def run(cls, k, cs, fixed, advice, instances, assembly=None, challenges=None) -> "MockProver":
        return cls(k, cs, fixed, advice, instances, assembly, challenges)

    def verify(self) -> List[str]:
        cs, n = self.cs, self.n
        u = cs.usable_rows(self.k)
        failures: List[str] = []
        ch = None if self.challenges is None else (lambda i: self.challenges[i])
        for row in range(u):
            fx = lambda c, r, row=row: self.fixed[c][(row + r) % n]
            ad = lambda c, r, row=row: self.advice[c][(row + r) % n]
            ins = lambda c, r, row=row: self.instance[c][(row + r) % n]
            for gi, g in enumerate(cs.gates):
                if ex.evaluate(g, fx, ad, ins, ch) != 0:
                    failures.append(f"gate {gi} not satisfied on row {row}")
        for li, lk in enumerate(cs.lookups):
            rows = []
            for row in range(u):
                fx = lambda c, r, row=row: self.fixed[c][(row + r) % n]
                ad = lambda c, r, row=row: self.advice[c][(row + r) % n]
                ins = lambda c, r, row=row: self.instance[c][(row + r) % n]
                rows.append((tuple(ex.evaluate(e, fx, ad, ins, ch) for e in lk.input_expressions),
                             tuple(ex.evaluate(e, fx, ad, ins, ch) for e in lk.table_expressions)))
            table = {t for _, t in rows}
            for row, (inp, _) in enumerate(rows):
                if inp not in table:
                    failures.append(f"lookup {li}: input of row {row} is not in the table")
        if self.assembly is not None:
            cols = {ADVICE: self.advice, FIXED: self.fixed, INSTANCE: self.instance}
            for j, (t, i) in enumerate(self.assembly.columns):
                for row in range(n):
                    cj, rj = int(self.assembly.map_c[j, row]), int(self.assembly.map_r[j, row])
                    if (cj, rj) != (j, row):
                        t2, i2 = self.assembly.columns[cj]
                        if cols[t][i][row] != cols[t2][i2][rj]:
                            failures.append(f"copy constraint violated: column {j} row {row} != column {cj} row {rj}")
        return failures

    def assert_satisfied(self) -> None:
        f = self.verify()
        if f:
            raise VerifyFailure("; ".join(f[:5]) + (f" (+{len(f) - 5} more)" if len(f) > 5 else ""))


MockFailure = namedtuple("MockFailure", "kind index row other_column other_row")   # kind: "gate" | "lookup" | "copy"; other_*: the mapped cell of a copy


class NativeMockProver:
    """MockProver on the GPU: zk_mock_prover_verify (csrc/mockprover.hip) checks the gates, lookups and copy constraints of the witness with HIP kernels over
    all 2^k rows and returns MockProver.verify()'s failures in MockProver.verify()'s order.  Built from what keygen builds: the Evaluator's ZKQ1 blob
    (keygen.compile_program; only its custom gates are read), the lookup compressor programs, and Assembly.map_c / map_r as the copy mapping.
    Gates and lookups are detected through random folds the library draws per call (a failure is missed with probability at most E / |Fr|
    for E gate polynomials, (m - 1) / |Fr| for a lookup tuple of m expressions).  A circuit with user challenges takes their values as `challenges` (zk_mock_prover_verify_phased)."""

    KINDS = ("gate", "lookup", "copy")

    def __init__(self, k: int, cs: ConstraintSystem, fixed: Sequence, advice: Sequence, instances: Sequence[Sequence[int]], assembly: Assembly | None = None,
                 backend=None, challenges: Sequence[int] | None = None):
        from .._lib import default_backend
        from .keygen import compile_program, compressor_program
        self.k, self.n, self.cs, self.assembly = k, 1 << k, cs, assembly
        self.backend = backend or default_backend()
        dev = lambda c: not isinstance(c, (np.ndarray, list, tuple))
        conv = lambda c: c if dev(c) else (np.ascontiguousarray(c).reshape(-1, 4) if isinstance(c, np.ndarray) and c.dtype == np.uint64 else fr_mont_array([int(v) % R_MOD for v in c]))
        self.fixed = [conv(c) for c in fixed]
        self.advice = [conv(c) for c in advice]
        self.instances = [[int(v) for v in c] for c in instances]
        ek = k
        while (1 << ek) < self.n * (cs.degree() - 1):                       # EvaluationDomain::new(cs.degree(), k): the blob zk_plonk_pk_build takes
            ek += 1
        perm = list(assembly.columns) if assembly is not None else []
        self.args = dict(k=k, blinding_factors=cs.blinding_factors(), n_fixed=cs.num_fixed_columns, n_advice=cs.num_advice_columns, n_instance=cs.num_instance_columns,
                         perm_columns=perm, evaluator_blob=compile_program(cs, k, ek).to_blob(),
                         lookup_input_blobs=[compressor_program(cs, k, lk.input_expressions).to_blob() for lk in cs.lookups],
                         lookup_table_blobs=[compressor_program(cs, k, lk.table_expressions).to_blob() for lk in cs.lookups],
                         fixed=self.fixed, advice=self.advice, instances=self.instances,
                         perm_map_column=assembly.map_c if perm else None, perm_map_row=assembly.map_r if perm else None)
        if challenges is not None:
            self.args["challenges"] = [int(c) % R_MOD for c in challenges]
        self._records, self._counts = None, None

    @classmethod
    def run(cls, k, cs, fixed, advice, instances, assembly=None, backend=None, challenges=None) -> "NativeMockProver":
        return cls(k, cs, fixed, advice, instances, assembly, backend, challenges)

    def _check(self, cap: int):
        recs, counts = self.backend.mock_prover_verify(cap=cap, **self.args)
        return [MockFailure(self.KINDS[r[0]], *r[1:]) for r in recs], counts

    def failures(self, cap: int | None = None) -> List[MockFailure]:
        """the structured records: all of them, or the first `cap` (one device check per call with a cap)"""
        if cap is not None:
            return self._check(cap)[0]
        if self._records is None:
            recs, counts = self._check(4096)
            if sum(counts) > len(recs):
                recs, counts = self._check(sum(counts))
            self._records, self._counts = recs, counts
        return self._records

    @property
    def counts(self):
        """(gate, lookup, copy) failures, exact"""
        if self._counts is None:
            self.failures()
        return self._counts

    def verify(self) -> List[str]:
        """MockProver.verify()'s strings, one per record, in its order"""
        out = []
        for f in self.failures():
            if f.kind == "gate":
                out.append(f"gate {f.index} not satisfied on row {f.row}")
            elif f.kind == "lookup":
                out.append(f"lookup {f.index}: input of row {f.row} is not in the table")
            else:
                out.append(f"copy constraint violated: column {f.index} row {f.row} != column {f.other_column} row {f.other_row}")
        return out

    def assert_satisfied(self) -> None:
        f = self.verify()
        if f:
            raise VerifyFailure("; ".join(f[:5]) + (f" (+{len(f) - 5} more)" if len(f) > 5 else ""))


class NativeMockSession:
    """One circuit resident on the GPU, any number of witnesses checked against it: zk_mock_prover_open once, zk_mock_prover_check per witness (csrc/mockprover.hip,
    DESIGN.md 3.6).  open uploads the fixed columns, reduces Assembly.map_c / map_r to the copy edges, compiles the gate and lookup programs and sorts the lookup
    tables that read fixed columns only; a check then costs its kernels.  The records are NativeMockProver's, record for record.  Advice may be host arrays, integer
    lists or device buffers - the buffers a following prove adopts are read, never written.  Use as a context manager, or close() it."""

    KINDS = NativeMockProver.KINDS

    def __init__(self, k: int, cs: ConstraintSystem, fixed: Sequence, assembly: Assembly | None = None, backend=None):
        from .._lib import default_backend
        from .keygen import compile_program, compressor_program
        self.k, self.n, self.cs, self.assembly = k, 1 << k, cs, assembly
        self.backend = backend or default_backend()
        self.fixed = [self._conv(c) for c in fixed]                          # (device-resident fixed columns are borrowed by the handle: kept alive here)
        ek = k
        while (1 << ek) < self.n * (cs.degree() - 1):
            ek += 1
        perm = list(assembly.columns) if assembly is not None else []
        self._counts = None
        self.handle = 0
        self.handle = self.backend.mock_prover_open(
            k=k, blinding_factors=cs.blinding_factors(), n_fixed=cs.num_fixed_columns, n_advice=cs.num_advice_columns, n_instance=cs.num_instance_columns,
            perm_columns=perm, evaluator_blob=compile_program(cs, k, ek).to_blob(),
            lookup_input_blobs=[compressor_program(cs, k, lk.input_expressions).to_blob() for lk in cs.lookups],
            lookup_table_blobs=[compressor_program(cs, k, lk.table_expressions).to_blob() for lk in cs.lookups],
            fixed=self.fixed, perm_map_column=assembly.map_c if perm else None, perm_map_row=assembly.map_r if perm else None)

    @staticmethod
    def _conv(c):
        if not isinstance(c, (np.ndarray, list, tuple)):
            return c                                                         # a device buffer
        if isinstance(c, np.ndarray) and c.dtype == np.uint64:
            return np.ascontiguousarray(c).reshape(-1, 4)
        return fr_mont_array([int(v) % R_MOD for v in c])

    def _run(self, advice, instances, challenges, cap):
        recs, counts = self.backend.mock_prover_check(self.handle, [self._conv(c) for c in advice], [[int(v) for v in c] for c in instances], cap=cap,
                                                      challenges=None if challenges is None else [int(c) % R_MOD for c in challenges])
        return [MockFailure(self.KINDS[r[0]], *r[1:]) for r in recs], counts

    def check(self, advice: Sequence, instances: Sequence[Sequence[int]], challenges: Sequence[int] | None = None, cap: int | None = None) -> List[MockFailure]:
        """the structured records of one witness: all of them (a second device check when there are more than 4096), or the first `cap`"""
        if cap is not None:
            recs, self._counts = self._run(advice, instances, challenges, cap)
            return recs
        recs, counts = self._run(advice, instances, challenges, 4096)
        if sum(counts) > len(recs):
            recs, counts = self._run(advice, instances, challenges, sum(counts))
        self._counts = counts
        return recs

    @property
    def counts(self):
        """(gate, lookup, copy) failures of the last check, exact"""
        return self._counts

    def verify(self, advice, instances, challenges=None) -> List[str]:
        """MockProver.verify()'s strings for this witness, one per record, in its order"""
        out = []
        for f in self.check(advice, instances, challenges):
            if f.kind == "gate":
                out.append(f"gate {f.index} not satisfied on row {f.row}")
            elif f.kind == "lookup":
                out.append(f"lookup {f.index}: input of row {f.row} is not in the table")
            else:
                out.append(f"copy constraint violated: column {f.index} row {f.row} != column {f.other_column} row {f.other_row}")
        return out

    def assert_satisfied(self, advice, instances, challenges=None) -> None:
        f = self.verify(advice, instances, challenges)
        if f:
            raise VerifyFailure("; ".join(f[:5]) + (f" (+{len(f) - 5} more)" if len(f) > 5 else ""))

    @property
    def info(self) -> dict:
        """zk_mock_prover_info: copy edges kept against mapping cells, distinct / resident tables, compiled programs, device bytes"""
        return self.backend.mock_prover_info(self.handle)

    def close(self):
        if self.handle and self.backend.ctx:
            h, self.handle = self.handle, 0
            self.backend.mock_prover_close(h)
        self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
