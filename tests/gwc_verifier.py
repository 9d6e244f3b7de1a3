"""TEST INFRASTRUCTURE ONLY — verify_proof with the GWC multi-open (halo2's VerifierGWC), restated from the KZG opening equation for ONE proof over m circuits with
advice in phases, through any of the three transcript readers.

[3P-MEM] halo2_proofs v2023_01_20 (PSE) src/plonk/verifier.rs and src/poly/kzg/multiopen/gwc{.rs,/verifier.rs}, restated from memory (the crate is not on this
machine).  Everything up to the query list is tests/phased_verifier.py (which is tests/multi_circuit_verifier.py with phases, which is oracle/verifier.py over m
circuits): the same reads, the same squeezes, the same quotient identity on the evaluations — its value is the evaluation the verifier asks of the h commitment — and
the same query order (oracle/verifier.py:214-235).  Then GWC: squeeze v; group the queries by point IN ORDER OF FIRST APPEARANCE (a linear scan; points are not sorted,
queries not deduplicated); read one point W_i per group; the proof must end there.

halo2's verifier folds all groups with a challenge u of its own into one pairing.  This one knows the test's trapdoor tau and checks every group on its own:

        (tau - z_i) W_i  ==  sum_j v^j C_j  -  (sum_j v^j e_j) G            (j over the queries of group i, from v^0)

which is the KZG opening equation of B_i(X) = sum_j v^j poly_j(X) at z_i, written in G1.  tau != z_i (a Fiat-Shamir point), so W_i is UNIQUELY determined by the
equation: acceptance pins the bytes of each W_i, not a random combination of them.  Shares no arithmetic with the product: oracle/pyref.py and the helpers of
oracle/verifier.py only; the verifying key and its constraint system are read as plain data.
"""
from __future__ import annotations

import pyref as p
import verifier as v1
from phased_verifier import _eval_expr, phase_lists

R = p.R


def group_by_first_appearance(Q):
    """[(point, [queries])]: a query joins the group whose point equals its own, otherwise it opens a new group at the end"""
    groups = []
    for q in Q:
        for point, members in groups:
            if point == q[2]:
                members.append(q)
                break
        else:
            groups.append((q[2], [q]))
    return groups


def verify_proof_gwc(vk, tau: int, instances_list, proof: bytes, reader=None, info: dict | None = None) -> bool:
    """plonk::verify_proof with VerifierGWC over m = len(instances_list) circuits.  Returns True / False; malformed proofs (too short, trailing bytes, a word that is no
    point or no canonical scalar) raise ValueError.  `reader`: oracle/verifier.py's _Reader (Blake2b, the default), poseidon_ref.Reader or evm_ref.Reader.
    info, when given, receives {"points": the opening points in group order, "sizes": queries per group, "witness_at": byte offset of W_0, "v": v,
    "first_eval_at": byte offset of the first evaluation}."""
    cs, k = vk.cs, vk.k
    m = len(instances_list)
    n = 1 << k
    w = p.omega(k)
    bf = cs.blinding_factors()
    L = len(cs.lookups)
    chunk = cs.permutation_chunk_len()
    n_perm = len(cs.permutation_columns)
    n_sets = (n_perm + chunk - 1) // chunk if n_perm else 0
    tr = (reader or v1._Reader)(proof)
    tr.common_scalar(vk.transcript_repr)
    for instances in instances_list:
        assert len(instances) == cs.num_instance_columns
        for col in instances:
            for val in col:
                tr.common_scalar(val)
    adv_phase, chal_phase = phase_lists(cs)
    advice_c = [[None] * cs.num_advice_columns for _ in range(m)]
    chal = [0] * len(chal_phase)
    for phase in range(max([0] + adv_phase) + 1):
        for c in range(m):
            for col in range(cs.num_advice_columns):
                if adv_phase[col] == phase:
                    advice_c[c][col] = tr.read_point()
        for i, cp in enumerate(chal_phase):
            if cp == phase:
                chal[i] = tr.squeeze()
    theta = tr.squeeze()
    permuted_c = [[(tr.read_point(), tr.read_point()) for _ in range(L)] for _ in range(m)]
    beta, gamma = tr.squeeze(), tr.squeeze()
    perm_z_c = [[tr.read_point() for _ in range(n_sets)] for _ in range(m)]
    lookup_z_c = [[tr.read_point() for _ in range(L)] for _ in range(m)]
    random_c = tr.read_point()
    y = tr.squeeze()
    h_c = [tr.read_point() for _ in range(cs.degree() - 1)]
    x = tr.squeeze()
    xn = pow(x, n, R)
    rot = lambda r: x * pow(w, r % n, R) % R

    first_eval_at = tr.pos
    aq, fq, iq = cs.advice_queries(), cs.fixed_queries(), cs.instance_queries()
    advice_evals = [{q: tr.read_scalar() for q in aq} for _ in range(m)]
    fixed_evals = {q: tr.read_scalar() for q in fq}
    random_eval = tr.read_scalar()
    sigma_evals = [tr.read_scalar() for _ in range(n_perm)]
    perm_evals = []
    for _ in range(m):
        per = []
        for i in range(n_sets):
            e = {"z": tr.read_scalar(), "z_next": tr.read_scalar()}
            if i + 1 < n_sets:
                e["z_last"] = tr.read_scalar()
            per.append(e)
        perm_evals.append(per)
    lookup_evals = [[dict(zip(("z", "z_next", "a", "a_inv", "s"), [tr.read_scalar() for _ in range(5)])) for _ in range(L)] for _ in range(m)]

    # ---- the quotient identity on the evaluations: what h(x) must be --------------------------------------------------------------------------------------
    l_0 = v1._lagrange_at(0, x, xn, k)
    l_last = v1._lagrange_at(n - bf - 1, x, xn, k)
    l_blind = sum(v1._lagrange_at(n - bf + i, x, xn, k) for i in range(bf)) % R
    l_active = (1 - l_last - l_blind) % R
    exprs = []
    for c in range(m):
        instance_evals = {}
        for (col, r) in iq:
            pt = rot(r)
            ptn = pow(pt, n, R)
            instance_evals[(col, r)] = sum(val * v1._lagrange_at(i, pt, ptn, k) for i, val in enumerate(instances_list[c][col])) % R
        ae, pe = advice_evals[c], perm_evals[c]
        exprs += [_eval_expr(g, fixed_evals, ae, instance_evals, chal) for g in cs.gates]
        col_eval = lambda t, i: {0: ae, 1: fixed_evals, 2: instance_evals}[t][(i, 0)]
        if n_sets:
            exprs.append(l_0 * (1 - pe[0]["z"]) % R)
            zl = pe[-1]["z"]
            exprs.append(l_last * (zl * zl - zl) % R)
            for i in range(1, n_sets):
                exprs.append(l_0 * (pe[i]["z"] - pe[i - 1]["z_last"]) % R)
            for i in range(n_sets):
                cols = cs.permutation_columns[i * chunk:(i + 1) * chunk]
                left, right = pe[i]["z_next"], pe[i]["z"]
                cur_delta = beta * x % R * pow(p.DELTA, i * chunk, R) % R
                for j, (t, ci) in enumerate(cols):
                    val = col_eval(t, ci)
                    left = left * (val + beta * sigma_evals[i * chunk + j] + gamma) % R
                    right = right * (val + cur_delta + gamma) % R
                    cur_delta = cur_delta * p.DELTA % R
                exprs.append((left - right) * l_active % R)
        for lk, e in zip(cs.lookups, lookup_evals[c]):
            def compress(es):
                acc_ = 0
                for ex_ in es:
                    acc_ = (acc_ * theta + _eval_expr(ex_, fixed_evals, ae, instance_evals, chal)) % R
                return acc_
            exprs.append(l_0 * (1 - e["z"]) % R)
            exprs.append(l_last * (e["z"] * e["z"] - e["z"]) % R)
            left = e["z_next"] * (e["a"] + beta) % R * (e["s"] + gamma) % R
            right = e["z"] * (compress(lk.input_expressions) + beta) % R * (compress(lk.table_expressions) + gamma) % R
            exprs.append((left - right) * l_active % R)
            exprs.append(l_0 * (e["a"] - e["s"]) % R)
            exprs.append((e["a"] - e["s"]) * (e["a"] - e["a_inv"]) % R * l_active % R)
    acc = 0
    for val in exprs:
        acc = (acc * y + val) % R
    expected_h_eval = acc * pow(xn - 1, -1, R) % R
    h_commitment = None
    for c in reversed(h_c):
        h_commitment = p.g1_add(p.g1_mul(h_commitment, xn), c)

    # ---- the queries, in the prover's order (oracle/verifier.py:214-235, per circuit where halo2 loops over the circuits) -------------------------------
    x_next, x_inv, x_last = rot(1), rot(-1), rot(-(bf + 1))
    Q = []                                                           # (what, commitment, point, eval)
    for c in range(m):
        for (col, r) in aq:
            Q.append((("adv", c, col), advice_c[c][col], rot(r), advice_evals[c][(col, r)]))
        for i in range(n_sets):
            Q.append((("pz", c, i), perm_z_c[c][i], x, perm_evals[c][i]["z"]))
            Q.append((("pz", c, i), perm_z_c[c][i], x_next, perm_evals[c][i]["z_next"]))
        for i in reversed(range(n_sets - 1)):
            Q.append((("pz", c, i), perm_z_c[c][i], x_last, perm_evals[c][i]["z_last"]))
        for i, e in enumerate(lookup_evals[c]):
            Q.append((("lz", c, i), lookup_z_c[c][i], x, e["z"]))
            Q.append((("la", c, i), permuted_c[c][i][0], x, e["a"]))
            Q.append((("ls", c, i), permuted_c[c][i][1], x, e["s"]))
            Q.append((("la", c, i), permuted_c[c][i][0], x_inv, e["a_inv"]))
            Q.append((("lz", c, i), lookup_z_c[c][i], x_next, e["z_next"]))
    for (col, r) in fq:
        Q.append((("fix", col), vk.fixed_commitments[col], rot(r), fixed_evals[(col, r)]))
    for j in range(n_perm):
        Q.append((("sig", j), vk.permutation_commitments[j], x, sigma_evals[j]))
    Q.append((("h",), h_commitment, x, expected_h_eval))
    Q.append((("rand",), random_c, x, random_eval))

    # ---- VerifierGWC, one opening equation per point ------------------------------------------------------------------------------------------------------
    v = tr.squeeze()
    groups = group_by_first_appearance(Q)
    witness_at = tr.pos
    witnesses = [tr.read_point() for _ in groups]
    if tr.pos != len(tr.proof):
        raise ValueError("trailing bytes in proof")
    if info is not None:
        info.update(points=[z for z, _ in groups], sizes=[len(qs) for _, qs in groups], witness_at=witness_at, first_eval_at=first_eval_at, v=v)
    ok = True
    for (z_i, members), W in zip(groups, witnesses):
        com, ev, vp = None, 0, 1
        for _, C, _, e in members:
            com = p.g1_add(com, p.g1_mul(C, vp))
            ev = (ev + vp * e) % R
            vp = vp * v % R
        rhs = p.g1_add(com, p.g1_mul(p.G1_GEN, (-ev) % R))
        ok = ok and p.g1_mul(W, (tau - z_i) % R) == rhs
    return ok
