"""The limb routines on the GPU: tests/csrc/device_harness.hip runs the very functions of tests/csrc/limb_cases.h that tests/test_field29.py and tests/test_host_logic.py run
on the CPU — there the plain C++ branches of field_mac.inc / field29_mac.inc, here the inline assembly that ships (v_mad_u64_u32 with and without its carry counter on vcc).
Every test below is the twin of the CPU test of the same name: the same seeds and rows (tests/limb_cases.py), the same exact column models, Python integers, oracle and
group law as the reference.  What only a GPU has comes from the runner (limb_cases.DeviceRunner): every element-wise op is launched with its rows under a fixed stride
permutation, so each wave mixes boundary rows with random ones, at the test's own row count (61, 81, 245, ... never a multiple of 64) and continued to 293 rows, with
block 64 and block 256; chains run one per thread, many to a launch.  After the models, every device output must equal the host harness's on all limbs.
test_divergent_chains_in_one_launch has no CPU namesake: 135 chains of 1 .. 128 points in ONE launch, planted doublings / cancellations / identity bases next to plain
chains in the same wave — the divergence of the MSM's accumulate loop; its check runs on the CPU harness too (the last test, no GPU needed)."""
import ctypes as C
import os

import pytest

import limb_cases as lc
from conftest import HOST_SO, ROOT

DEV_SO = os.path.join(ROOT, "tests", "csrc", "libdevharness.so")


@pytest.fixture(scope="module")
def dev(built):
    """one DeviceRunner for the module: after a non-zero HIP status it launches nothing more, so every later test fails at once"""
    return lc.DeviceRunner(C.CDLL(DEV_SO), lc.HostRunner(C.CDLL(HOST_SO)))


def twin(dev, check, *args):
    dev.differs = []
    check(dev, *args)
    dev.assert_equal_to_host()                                        # device == host bit for bit: the second check, after the models inside `check`


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_products_on_raw_limbs_match_the_exact_model_at_the_limb_bounds(dev, pyref, field):
    twin(dev, lc.check_products_on_raw_limbs, pyref, field)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_biased_differences_and_the_carry_round(dev, pyref, field):
    twin(dev, lc.check_biased_differences_and_the_carry_round, pyref, field)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_between_the_two_montgomery_forms(dev, orc, pyref, field):
    twin(dev, lc.check_between_the_two_montgomery_forms, orc, pyref, field)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1])
def test_shoup_product_with_a_precomputed_quotient(dev, orc, pyref, field):
    """the rows with limbs up to 3 * 2^30 (loose = 31.58) and the two all-limbs-at-bound rows included: 263 rows, more than one block of 256"""
    twin(dev, lc.check_shoup_product_with_a_precomputed_quotient, orc, pyref, field)


@pytest.mark.gpu
def test_bucket_chain_on_29_bit_limbs_equals_the_canonical_chain(dev, orc, pyref):
    twin(dev, lc.check_bucket_chain_on_29_bit_limbs, orc, pyref)


@pytest.mark.gpu
def test_field_limb_ops(dev, orc, pyref):
    twin(dev, lc.check_field_limb_ops, orc, pyref)


@pytest.mark.gpu
def test_fused_two_product_reduction(dev, orc, pyref):
    twin(dev, lc.check_fused_two_product_reduction, orc, pyref)


@pytest.mark.gpu
def test_xyzz_group_law_including_special_cases(dev, orc, pyref):
    twin(dev, lc.check_xyzz_group_law_including_special_cases, orc, pyref)


@pytest.mark.gpu
def test_redundant_range_arithmetic_on_the_range_boundaries(dev, orc, pyref):
    twin(dev, lc.check_redundant_range_arithmetic_on_the_range_boundaries, orc, pyref)


@pytest.mark.gpu
def test_lazy_mixed_addition_chain_equals_the_canonical_one(dev, orc, pyref):
    twin(dev, lc.check_lazy_mixed_addition_chain_equals_the_canonical_one, orc, pyref)


@pytest.mark.gpu
def test_fast_chain_filter_refuses_every_same_x_addition(dev, orc, pyref):
    """the 600 seeded chains and oracle prefixes of the CPU test in ONE launch (twice: block 64, block 256), one chain per thread; the false-alarm count is printed, not
    asserted"""
    twin(dev, lc.check_fast_chain_filter_refuses_every_same_x_addition, orc, pyref)


@pytest.mark.gpu
def test_divergent_chains_in_one_launch(dev, orc, pyref):
    twin(dev, lc.check_divergent_chains_in_one_launch, orc, pyref)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_anything_is_launched(dev):
    """validation comes first: a null pointer, a block size that is no multiple of 64 or above 256, offsets that do not tile the point buffer — each returns
    hipErrorInvalidValue (1) without a launch, and the runner stays usable"""
    import numpy as np
    a = np.zeros((3, 4), dtype=np.uint64)
    o = np.zeros_like(a)
    P, n = lc.P, C.c_size_t(3)
    lib = dev.lib
    for fn in (lib.dh_fq_mul, lib.dh_xyzz_sum):
        fn.restype = C.c_int
    assert dev.status == 0
    assert lib.dh_fq_mul(P(a), None, P(o), n, C.c_int(64)) == 1
    assert lib.dh_fq_mul(P(a), P(a), P(o), n, C.c_int(96)) == 1
    assert lib.dh_fq_mul(P(a), P(a), P(o), n, C.c_int(512)) == 1
    assert lib.dh_fq_mul(P(a), P(a), P(o), C.c_size_t(1 << 40), C.c_int(64)) == 1
    pts, neg, out = np.zeros((4, 8), dtype=np.uint64), np.zeros(4, dtype=np.uint8), np.zeros((2, 16), dtype=np.uint64)
    for off in ([1, 2, 4], [0, 3, 2]):                                # does not start at 0; not monotone
        assert lib.dh_xyzz_sum(P(pts), P(neg), P(np.array(off, dtype=np.uint64)), C.c_size_t(2), P(out), C.c_int(64)) == 1
    assert lib.dh_fq_mul(P(a), P(a), P(o), n, C.c_int(64)) == 0 and not o.any()


def test_divergent_chains_check_on_the_cpu_harness(built, orc, pyref):
    """the same 135 chains through libhostharness.so: the chains, the expected n_rare and the group-law reference are right before a GPU sees them"""
    lc.check_divergent_chains_in_one_launch(lc.HostRunner(C.CDLL(HOST_SO)), orc, pyref)
