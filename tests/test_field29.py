"""csrc/field29.cuh — the carry-free arithmetic on 9 limbs of 29 bits (Montgomery radix 2^261) that the bucket accumulation runs on — compiled for the CPU and driven
on RAW limbs against an exact Python model: the model recomputes every column sum of a product as a Python integer, asserts it fits the 64-bit accumulator for the
operand shapes the kernel produces (xyzz29_madd_fast: ec.cuh lists them), and the C result must equal the model's, limb for limb.  Then the chain itself: a bucket's
mixed additions on 29-bit limbs give the coordinates of the canonical chain, special cases included.  The rows, the models and the checks live in tests/limb_cases.py, which
tests/test_limbs_device.py runs again on the GPU."""
import ctypes as C

import pytest

import limb_cases as lc
from conftest import HOST_SO


@pytest.fixture(scope="module")
def hh(built):
    return lc.HostRunner(C.CDLL(HOST_SO))


@pytest.mark.parametrize("field", [0, 1])
def test_products_on_raw_limbs_match_the_exact_model_at_the_limb_bounds(hh, pyref, field):
    lc.check_products_on_raw_limbs(hh, pyref, field)


@pytest.mark.parametrize("field", [0, 1])
def test_biased_differences_and_the_carry_round(hh, pyref, field):
    lc.check_biased_differences_and_the_carry_round(hh, pyref, field)


@pytest.mark.parametrize("field", [0, 1])
def test_between_the_two_montgomery_forms(hh, orc, pyref, field):
    lc.check_between_the_two_montgomery_forms(hh, orc, pyref, field)


@pytest.mark.parametrize("field", [0, 1])
def test_shoup_product_with_a_precomputed_quotient(hh, orc, pyref, field):
    """mul_shoup: a * w mod p for a constant w, wq = floor(w 2^261 / p) — what the NTT butterflies multiply their twiddles with.  shoup_quotient is exact; the product equals the
    column model limb for limb, is congruent to a * w, below 3 p, for every a below 2^261 with limbs up to 3 * 2^30 — a biased difference of N-form values, the loosest operand a
    butterfly multiplies (q is the true quotient or one below).  mul_shoup = shoup_r(shoup_q(..)), the two halves the NTT kernels call."""
    lc.check_shoup_product_with_a_precomputed_quotient(hh, orc, pyref, field)


def test_bucket_chain_on_29_bit_limbs_equals_the_canonical_chain(hh, orc, pyref):
    """the coordinates — not only the point — of the 29-bit chain equal the canonical chain's (the same rational formulas over the same field), through the fast step
    and through every rare case: identity bases, the first point, a doubling, P then -P (cancellation to the identity) and a chain that continues after it"""
    lc.check_bucket_chain_on_29_bit_limbs(hh, orc, pyref)
