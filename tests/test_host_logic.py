"""The product's __host__ __device__ limb routines (field.cuh / ec.cuh) compiled for the CPU,
checked against the oracle.  Covers the arithmetic the kernels inline; no GPU needed.  The rows and the
checks live in tests/limb_cases.py, which tests/test_limbs_device.py runs again on the GPU."""
import ctypes as C

import pytest

import limb_cases as lc
from conftest import HOST_SO


@pytest.fixture(scope="module")
def hh(built):
    return lc.HostRunner(C.CDLL(HOST_SO))


def test_field_limb_ops(hh, orc, pyref):
    lc.check_field_limb_ops(hh, orc, pyref)


def test_fused_two_product_reduction(hh, orc, pyref):
    lc.check_fused_two_product_reduction(hh, orc, pyref)


def test_xyzz_group_law_including_special_cases(hh, orc, pyref):
    lc.check_xyzz_group_law_including_special_cases(hh, orc, pyref)


def test_redundant_range_arithmetic_on_the_range_boundaries(hh, orc, pyref):
    """field.cuh's lazy forms (the NTT butterflies in [0, 4p), the bucket accumulation in [0, 2p)): for inputs ON the boundaries of the documented ranges —
    0, 1, p - 1, p, p + 1, 2p - 1, 2p, 4p - 1 — and random ones, every result lies in the documented output range and is congruent to the exact answer."""
    lc.check_redundant_range_arithmetic_on_the_range_boundaries(hh, orc, pyref)


def test_lazy_mixed_addition_chain_equals_the_canonical_one(hh, orc, pyref):
    lc.check_lazy_mixed_addition_chain_equals_the_canonical_one(hh, orc, pyref)


def test_fast_chain_filter_refuses_every_same_x_addition(hh, orc, pyref):
    """xyzz29_madd_fast must return false — accumulator untouched — whenever the point shares its x with the accumulator (P = U2 - X1 + 8p is then j p for some j in 2 .. 9
    by the bounds of ec.cuh; the filter looks at one limb of it).  600 seeded chains of 1 .. 128 steps (the longest sub-bucket) through the fast step itself, so the
    accumulator's limbs sit wherever a real chain leaves them — a freshly entered point (ZZ = 1, X1 below p: j = 8, 9) up to X1 near its bound (small j); before EVERY
    step the accumulator's own point is offered with +y (a doubling) and -y (a cancellation): about 77000 collisions, not one may pass.  On the chain's own additions (x
    differs, asserted on the inputs) the result after every step equals the canonical xyzz_madd chain bit for bit, whether or not the filter raised a false alarm (ec.cuh
    expects 2^-25 per addition: 11 residues of 2^29; the observed count is printed — at this size it is almost surely 0)."""
    lc.check_fast_chain_filter_refuses_every_same_x_addition(hh, orc, pyref)


def test_chained_copy_rows_equals_scalar_copy_and_is_a_bijection():
    """Assembly.copy_rows must only take its vectorised path for cells that are their own (singleton) cycle: `sizes` is kept for cycle
    representatives only, so after copy_rows(A, B) the B cells still read size 1 — a chained copy_rows(B, C) has to fall back to copy()."""
    import numpy as np
    from zk_dcap_verifier_amd import plonk
    from zk_dcap_verifier_amd.plonk import ADVICE
    cs = plonk.ConstraintSystem(num_advice_columns=4)
    for c in range(4):
        cs.enable_equality(ADVICE, c)
    rows = [0, 1, 2, 3, 5]
    fast, slow = plonk.Assembly(cs, 3), plonk.Assembly(cs, 3)
    fast.copy_rows((ADVICE, 0), (ADVICE, 1), rows)
    fast.copy_rows((ADVICE, 1), (ADVICE, 2), rows)
    fast.copy_rows((ADVICE, 3), (ADVICE, 0), [5, 6])
    for r in rows:
        slow.copy((ADVICE, 0, r), (ADVICE, 1, r))
    for r in rows:
        slow.copy((ADVICE, 1, r), (ADVICE, 2, r))
    for r in (5, 6):
        slow.copy((ADVICE, 3, r), (ADVICE, 0, r))
    assert (fast.map_c == slow.map_c).all() and (fast.map_r == slow.map_r).all()
    succ = set(zip(fast.map_c.ravel().tolist(), fast.map_r.ravel().tolist()))
    assert len(succ) == 4 * 8                                       # the successor map is a permutation of the cells
    # the cycle through (0, 0) is A -> B -> C -> A in some rotation: three cells
    seen, cell = [], (0, 0)
    while cell not in seen:
        seen.append(cell)
        cell = (int(fast.map_c[cell]), int(fast.map_r[cell]))
    assert sorted(seen) == [(0, 0), (1, 0), (2, 0)]


def test_rand_fr_array_is_uniform_below_r_and_reproducible():
    import numpy as np
    from zk_dcap_verifier_amd import fields as F
    a = F.rand_fr_array(np.random.default_rng(5), 4000)
    b = F.rand_fr_array(np.random.default_rng(5), 4000)
    assert (a == b).all()
    vals = [F.unlimbs(x) for x in a]
    assert all(v < F.R_MOD for v in vals)
    top = sum(v >= (1 << 253) for v in vals) / len(vals)            # (r - 2^253) / r = 0.339 of the field lies above 2^253
    assert 0.30 < top < 0.38
    edge = np.array([F.limbs(F.R_MOD), F.limbs(F.R_MOD - 1), F.limbs(F.R_MOD + 1), F.limbs(0)], dtype=np.uint64)
    assert F._below_r(edge).tolist() == [False, True, False, True]
    c = F.rand_fr_array(F.OsRng(), 100)
    assert c.shape == (100, 4) and all(F.unlimbs(x) < F.R_MOD for x in c)
