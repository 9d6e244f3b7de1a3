"""TEST INFRASTRUCTURE ONLY — copy mappings for zk_plonk_keygen_vk (tests/test_keygen_native.py) and their reference.

A mapping is two (m, n) uint32 planes (column, row), n = 2^k: cell (j, i) is sent to (map_c[j, i], map_r[j, i]) — halo2's permutation::keygen::Assembly::mapping,
as zk_mock_desc and zk_plonk_keygen_desc carry it.  Every mapping here is a permutation of the m * n cells.  The reference of the sigma columns is oracle/prover.py:
its Assembly for the mapping built from copies, and the line of its keygen that turns a mapping into sigma values (sigma_j[i] = DELTA^c * omega^r), restated in
sigma_ints() on the same constants (oracle/pyref.py) for mappings that no list of copies produces; for the mapping built from copies the test also runs the oracle's own
keygen (oracle_keygen_sigma) and requires the two to agree, so a drift of the restatement from the oracle's definition is noticed."""
import random

import numpy as np


def identity(m, n):
    return (np.repeat(np.arange(m, dtype=np.uint32)[:, None], n, axis=1).copy(), np.repeat(np.arange(n, dtype=np.uint32)[None, :], m, axis=0).copy())


def _cycle(m, n, cells):
    """the identity except that every cell of `cells` is sent to the next one, the last to the first"""
    mc, mr = identity(m, n)
    for (j, i), (cj, ci) in zip(cells, cells[1:] + cells[:1]):
        mc[j, i], mr[j, i] = cj, ci
    return mc, mr


def column_cycle(m, n):
    """one cycle through every cell of one column (the middle one)"""
    j = m // 2
    return _cycle(m, n, [(j, i) for i in range(n)])


def full_cycle(m, n):
    """one cycle through every cell of all columns: cell e = j * n + i is sent to cell e + 1"""
    return _cycle(m, n, [(j, i) for j in range(m) for i in range(n)])


def corner_swaps(m, n):
    """2-cycles across the first and the last column at rows 0 and n - 1: (0, 0) <-> (m-1, n-1) and (0, n-1) <-> (m-1, 0) (one 2-cycle when m = 1)"""
    mc, mr = identity(m, n)
    for pair in {frozenset(((0, 0), (m - 1, n - 1))), frozenset(((0, n - 1), (m - 1, 0)))}:
        (ja, ia), (jb, ib) = sorted(pair)
        mc[ja, ia], mr[ja, ia], mc[jb, ib], mr[jb, ib] = jb, ib, ja, ia
    return mc, mr


def last_edges(m, n):
    """every cell of the last column and of the last row is sent to another cell of the last column or the last row — as far as "every cell mapped into the last column
    or last row" goes while the mapping stays a permutation (all of it when m = 1): one cycle down the last column and back along the last row, so both planes carry their
    largest legal value (m - 1, n - 1) in as many entries as a permutation allows"""
    return _cycle(m, n, [(m - 1, i) for i in range(n)] + [(j, n - 1) for j in range(m - 2, -1, -1)])


def random_copies_list(m, n):
    """a seeded list of copies ((type, index, row), (type, index, row)) between m advice columns of n rows"""
    rnd = random.Random(1000 * m + n)
    return [((0, rnd.randrange(m), rnd.randrange(n)), (0, rnd.randrange(m), rnd.randrange(n))) for _ in range(rnd.randint(m * n // 2, 2 * m * n))]


def random_copies(m, n):
    """those copies replayed through the oracle's Assembly.copy (cycle merge by swapping successors)"""
    import prover as op
    asm = op.Assembly([(0, j) for j in range(m)], n)
    for left, right in random_copies_list(m, n):
        asm.copy(left, right)
    mc = np.array([[c for c, _ in col] for col in asm.mapping], dtype=np.uint32).reshape(m, n)
    mr = np.array([[r for _, r in col] for col in asm.mapping], dtype=np.uint32).reshape(m, n)
    return mc, mr


MAPPINGS = {
    "identity": identity,
    "column_cycle": column_cycle,
    "full_cycle": full_cycle,
    "corner_swaps": corner_swaps,
    "random_copies": random_copies,
    "last_edges": last_edges,
}


def is_permutation(mc, mr):
    m, n = mc.shape
    return bool((mc < m).all() and (mr < n).all() and np.unique(mc.astype(np.int64) * n + mr).size == m * n)


def sigma_ints(mc, mr, k):
    """oracle/prover.py keygen: sigma_values[j][i] = DELTA^c * omega^r for (c, r) = mapping[j][i], canonical ints"""
    import pyref as p
    w = p.omega(k)
    wp = [pow(w, i, p.R) for i in range(1 << k)]
    dp = [pow(p.DELTA, j, p.R) for j in range(mc.shape[0])]
    return [[dp[int(c)] * wp[int(r)] % p.R for c, r in zip(mc[j], mr[j])] for j in range(mc.shape[0])]


def oracle_keygen_sigma(m, k, copies):
    """keys.sigma_values of oracle/prover.py's own keygen for m equality-enabled advice columns and these copies (no fixed columns; the commitments, which
    tests/test_keygen_native.py takes from the oracle's Params column by column, are left out here: its SRS costs 2^(k+1) point multiplications)"""
    import prover as op
    from zk_dcap_verifier_amd import plonk

    class NoCommit:
        def __init__(self):
            self.k, self.n = k, 1 << k

        def commit_lagrange(self, values):
            return None
    cs = plonk.ConstraintSystem(num_fixed_columns=0, num_advice_columns=m, num_instance_columns=0)
    for j in range(m):
        cs.enable_equality(plonk.ADVICE, j)
    return op.keygen(NoCommit(), cs, [], copies).sigma_values


def fixed_columns(n, count, seed):
    """`count` fixed columns as canonical ints: an all-zero column (its commitment is the identity), a 0/1 selector, a full-width random one, then more of the last two kinds"""
    import pyref as p
    rnd = random.Random(seed)
    kinds = [lambda: [0] * n, lambda: [rnd.randrange(2) for _ in range(n)], lambda: [rnd.randrange(p.R) for _ in range(n)]]
    if count == 1:
        return [kinds[0]()] if seed % 2 else [kinds[2]()]
    return [kinds[i % 3 if i < 3 else 1 + i % 2]() for i in range(count)]
