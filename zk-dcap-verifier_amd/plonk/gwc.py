"""halo2_proofs::poly::kzg::multiopen::ProverGWC, MI355X edition — the second multi-open argument halo2 ships for KZG, beside ProverSHPLONK (shplonk.py).

Mirrors ([3P-MEM] PSE halo2_proofs v2023_01_20; the crate is not in this tree) src/poly/kzg/multiopen/gwc{.rs,/prover.rs}: `plonk::create_proof` is generic over
the argument, snark-verifier-sdk exposes it as gen_proof_gwc / gen_evm_proof_gwc, and an EVM verifier generated for GWC accepts GWC proofs only.

    v = squeeze; group the queries by point, in order of FIRST APPEARANCE (a linear scan: points are not sorted, queries are not deduplicated and keep their order
    inside a group); per group i with point z_i:  B(X) = sum_j v^j poly_j(X)  (v^0 for the group's first query),  W_i = commit(kate_division(B - e, z_i)),
    write_point(W_i).  Nothing is squeezed after v (u is the verifier's), no rng draw is made (Blind::default()).

kate_division reads a[1..n), so the constant term — hence the "- e" — never enters the quotient.  This twin composes the SINGLE calls, one zk_fr_lincomb_dev and one
zk_kate_division_dev per point; the native prover (csrc/prover.hip gwc_create_proof) runs one batched combination and one batched division for all points, so
comparing the two compares two compositions (tests/test_gwc.py).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

from ..fields import R_MOD, fr_mont, fr_mont_array, g1_affine_ints
from .shplonk import ProverQuery


def group_by_point(queries: Sequence) -> List[Tuple[int, list]]:
    """gwc.rs construct_intermediate_sets: [(point, [queries])], groups in order of first appearance, queries in their own order"""
    groups: List[Tuple[int, list]] = []
    for q in queries:
        for point, members in groups:
            if point == q.point:
                members.append(q)
                break
        else:
            groups.append((q.point, [q]))
    return groups


class ProverGWC:
    def __init__(self, params):
        self.params = params

    def create_proof(self, transcript, queries: Sequence[ProverQuery]) -> None:
        be, n = self.params.backend, self.params.n
        v = transcript.squeeze_challenge()
        witnesses = []
        batch = be.alloc(n * 32)
        for point, members in group_by_point(queries):
            be.fr_lincomb_dev([q.poly for q in members], fr_mont_array([pow(v, j, R_MOD) for j in range(len(members))]), n, batch)
            w = be.alloc(n * 32)
            be.kate_division_dev(batch, n, fr_mont(point), w)
            w.zero((n - 1) * 32, 32)                                  # n - 1 coefficients; the commitment reads n
            witnesses.append(w)
        for pt in self.params.commit_columns("g", witnesses):          # one MSM batch, the points in group order
            transcript.write_point(g1_affine_ints(pt))
        for d in witnesses + [batch]:
            d.free()
