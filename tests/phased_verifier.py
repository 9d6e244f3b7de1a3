"""TEST INFRASTRUCTURE ONLY — oracle/verifier.py's verify_proof restated for ONE proof over m circuits with advice in several phases and halo2's Challenge API.

[3P-MEM] halo2_proofs v2023_01_20 (PSE) src/plonk/{circuit,verifier}.rs, restated from memory (the crate is not on this machine).  After the vk and the instances
the verifier reads, for phase = 0, 1, .. (the phases in use: 0 ..= max(advice_column_phase)), for circuit 0 .. m-1, the commitments of the advice columns of that phase
in ascending column index, and after the last circuit of the phase squeezes one challenge per i with challenge_phase[i] == phase, in ascending i.  Then theta and
everything else as for m single-phase circuits (tests/multi_circuit_verifier.py): advice evaluations, the query list and SHPLONK follow the query log, not the
phases.  Expression::Challenge(i) evaluates to challenge i (degree 0, no query) in gates, lookup inputs and lookup tables.  Like the single-circuit oracle it
replaces the pairing by the G1 identity [tau] h2 == outer, with the test's tau.  Shares no arithmetic with the product: oracle/pyref.py and the helpers of
oracle/verifier.py only; the verifying key and its constraint system are read as plain data (attribute and class NAMES, as oracle/verifier.py reads them).
With every column in phase 0 and no challenge it accepts what oracle/verifier.py accepts (tests/test_phased.py runs it on the three committed goldens).
"""
from __future__ import annotations

import functools

import pyref as p
import verifier as v1

R = p.R


def proof_length(cs, m: int, unit: int = 32) -> int:
    """bytes of an m-circuit proof: per circuit (A + 3 L + n_sets) points and (|advice queries| + 3 n_sets - 1 + 5 L) scalars; shared (1 + (d - 1) + 2) points and
    (|fixed queries| + 1 + n_perm) scalars"""
    L, n_perm = len(cs.lookups), len(cs.permutation_columns)
    chunk = cs.permutation_chunk_len()
    n_sets = (n_perm + chunk - 1) // chunk if n_perm else 0
    per_points = cs.num_advice_columns + 3 * L + n_sets
    per_scalars = len(cs.advice_queries()) + (3 * n_sets - 1 if n_sets else 0) + 5 * L
    shared = (1 + (cs.degree() - 1) + 2) + len(cs.fixed_queries()) + 1 + n_perm
    return unit * (m * (per_points + per_scalars) + shared)


def identities_per_circuit(cs) -> int:
    """E: the identities halo2 folds with y for one circuit — gate polynomials, 2 + (n_sets - 1) + n_sets of the permutation, 5 per lookup"""
    n_perm = len(cs.permutation_columns)
    chunk = cs.permutation_chunk_len()
    n_sets = (n_perm + chunk - 1) // chunk if n_perm else 0
    return len(cs.gates) + (2 + (n_sets - 1) + n_sets if n_sets else 0) + 5 * len(cs.lookups)


def _eval_expr(e, fixed, advice, instance, challenges) -> int:
    """oracle/verifier.py's _eval_expr with Expression::Challenge"""
    t = type(e).__name__
    if t == "Challenge":
        return challenges[e.index] % R
    if t in ("Constant", "Fixed", "Advice", "Instance"):
        return v1._eval_expr(e, fixed, advice, instance)
    sub = lambda s: _eval_expr(s, fixed, advice, instance, challenges)
    if t == "Negated":
        return -sub(e.a) % R
    if t == "Sum":
        return (sub(e.a) + sub(e.b)) % R
    if t == "Product":
        return sub(e.a) * sub(e.b) % R
    if t == "Scaled":
        return sub(e.a) * e.f % R
    raise TypeError(t)


def phase_lists(cs):
    """(advice_column_phase padded with phase 0, challenge_phase) of a constraint system, read as data"""
    ap = list(getattr(cs, "advice_column_phase", []) or [])
    ap += [0] * (cs.num_advice_columns - len(ap))
    return ap, list(getattr(cs, "challenge_phase", []) or [])


def verify_proof_phased(vk, tau: int, instances_list, proof: bytes, challenges_out: list | None = None) -> bool:
    """plonk::verify_proof with VerifierSHPLONK over m = len(instances_list) circuits whose advice is committed in phases.  Returns True / False; malformed proofs
    raise ValueError.  challenges_out, when given, receives every value squeezed: the user challenges in index order, then theta, beta, gamma, y, x, SHPLONK's y, v, u."""
    cs, k = vk.cs, vk.k
    m = len(instances_list)
    n = 1 << k
    w = p.omega(k)
    bf = cs.blinding_factors()
    L = len(cs.lookups)
    chunk = cs.permutation_chunk_len()
    n_perm = len(cs.permutation_columns)
    n_sets = (n_perm + chunk - 1) // chunk if n_perm else 0
    tr = v1._Reader(proof)
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

    l_0 = v1._lagrange_at(0, x, xn, k)
    l_last = v1._lagrange_at(n - bf - 1, x, xn, k)
    l_blind = sum(v1._lagrange_at(n - bf + i, x, xn, k) for i in range(bf)) % R
    l_active = (1 - l_last - l_blind) % R

    exprs = []                                                       # every circuit's identities, circuit by circuit, in one fold
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

    x_next, x_inv, x_last = rot(1), rot(-1), rot(-(bf + 1))
    Q = []                                                           # (commitment key, commitment point, point, eval)
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

    yy = tr.squeeze()
    super_points = sorted({q[2] for q in Q})
    order, info = [], {}
    for key, com, pt, ev in Q:
        if key not in info:
            info[key] = {"c": com, "pts": {}}
            order.append(key)
        info[key]["pts"].setdefault(pt, ev)
    sets = []
    for key in order:
        pts = tuple(sorted(info[key]["pts"]))
        for s in sets:
            if s[0] == pts:
                s[1].append(key)
                break
        else:
            sets.append((pts, [key]))
    vv = tr.squeeze()
    h1 = tr.read_point()
    u = tr.squeeze()
    h2 = tr.read_point()
    if tr.pos != len(tr.proof):
        raise ValueError("trailing bytes in proof")
    if challenges_out is not None:
        challenges_out[:] = chal + [theta, beta, gamma, y, x, yy, vv, u]
    vanish = lambda roots, z: functools.reduce(lambda a, r: a * (z - r) % R, roots, 1)
    outer, r_outer = None, 0
    z_0 = z_0_diff_inv = 0
    vpow = 1
    for i, (pts, keys) in enumerate(sets):
        z_diff = vanish([q for q in super_points if q not in pts], u)
        if i == 0:
            z_0 = vanish(pts, u)
            z_0_diff_inv = pow(z_diff, -1, R)
            z_diff = 1
        else:
            z_diff = z_diff * z_0_diff_inv % R
        inner, r_inner, ypow = None, 0, 1
        for key in keys:
            evals = [info[key]["pts"][q] for q in pts]
            r_x = v1._interpolate(list(pts), evals)
            r_inner = (r_inner + ypow * p.poly_eval(r_x, u)) % R
            inner = p.g1_add(inner, p.g1_mul(info[key]["c"], ypow))
            ypow = ypow * yy % R
        outer = p.g1_add(outer, p.g1_mul(inner, vpow * z_diff % R))
        r_outer = (r_outer + vpow * r_inner % R * z_diff) % R
        vpow = vpow * vv % R
    outer = p.g1_add(outer, p.g1_mul(p.G1_GEN, (-r_outer) % R))
    outer = p.g1_add(outer, p.g1_mul(h1, (-z_0) % R))
    outer = p.g1_add(outer, p.g1_mul(h2, u))
    return p.g1_mul(h2, tau) == outer
