"""The field-vector kernels on STRUCTURED columns (parity_cases.structured_fr): exact zeros, constants, r - 1 everywhere, single non-zero elements, operands that cancel or
add up to exactly r, selectors, sparse witnesses.  The kernels run on lazy representatives (values in [0, 2p) or [0, 4p), biased differences, 64-bit accumulator columns) and
normalise once at the end; on uniform columns an intermediate is never exactly 0, p, 2p or 3p, a denominator is never zero and no accumulator comes near its bound, so a '>'
for a '>=' in a conditional subtraction, a missing normalisation on one exit or a dropped zero guard passes every uniform test.  Everything here is compared bit for bit with
the CPU oracle, which returns canonical values: equality on all limbs also proves that every output word is canonical.  Emulator (CPU, small) and product C ABI on the GPU."""
import random

import numpy as np
import pytest

import parity_cases as pc
import quotient_cases as qc
import test_coset as tco
import test_eval_phase as tep
import test_grand_product as tgp
import zk_dcap_verifier_amd as z

KINDS = pc.STRUCTURED_KINDS
DOMAIN_KINDS = ("zeros", "const", "minus_one", "delta_first", "delta_mid", "delta_last", "selector", "selector_sparse", "witness")
QUOTIENT_KINDS = ("zeros", "selector", "const", "minus_one", "witness")
NONZERO_OUTPUTS = {"zeros": 0, "ones": 1, "const": 1, "neg_one": 1, "alt_pm": 1, "geometric": 1}      # closed forms: how many outputs of a transform of that kind are not 0


def _mont(orc, v):
    return orc.fr_from_ints([v])[0]


# ---- NTT ------------------------------------------------------------------------------------------------------------------------------------------------------
def _ntt_device_forms(be, orc, pyref, log_n, kinds, seed=7, single=True):
    """zk_ntt_batch_dev on ONE batch that mixes the kinds (a zero column beside r - 1 beside uniform noise ...) and zk_ntt_dev column by column, forward and inverse"""
    n = 1 << log_n
    cols = [pc.column(orc, pyref, n, seed + i, kd) for i, kd in enumerate(kinds)]
    for inverse in (False, True):
        w = _mont(orc, pow(pyref.omega(log_n), -1 if inverse else 1, pyref.R))
        want = [orc.best_fft(c, w, log_n) for c in cols]
        d = [be.to_device(c) for c in cols]
        be.ntt_batch_dev(d, log_n, w)
        for kd, dd, wnt in zip(kinds, d, want):
            got = dd.download((n, 4))
            assert (got == wnt).all(), ("batch", log_n, kd, inverse)
            if kd in NONZERO_OUTPUTS and n >= 2:
                assert int(got.any(axis=1).sum()) == NONZERO_OUTPUTS[kd], (log_n, kd)
                if kd in ("ones", "const", "neg_one"):
                    assert got[0].any()
                if kd == "alt_pm":
                    assert got[n // 2].any()
        if single:
            for kd, dd, c, wnt in zip(kinds, d, cols, want):
                dd.upload(c)
                be.ntt_dev(dd, log_n, w)
                assert (dd.download((n, 4)) == wnt).all(), ("single", log_n, kd, inverse)
        for dd in d:
            dd.free()


@pytest.mark.parametrize("kind", KINDS)
def test_emulated_ntt(emu, orc, pyref, kind):
    """zk_ntt under the fixture's plan (radix 2^4): one pass (2^3), two (2^7), three (2^10)"""
    for log_n in (3, 7, 10):
        pc.check_ntt(emu, orc, pyref, log_n, seed=log_n, kind=kind)
    for log_n in (4, 9):
        pc.check_ntt(emu, orc, pyref, log_n, seed=log_n, kind=kind, inverse=True)


@pytest.mark.parametrize("log_n", [2, 4, 8, 10])
def test_emulated_ntt_device_forms_mixed_batch(emu, orc, pyref, log_n):
    _ntt_device_forms(emu, orc, pyref, log_n, ("uniform",) + KINDS, single=log_n in (4, 8))


@pytest.mark.parametrize("tile,radix", [(4, 2), (5, 5), (8, 3)])
def test_emulated_ntt_other_plans(emu, orc, pyref, tile, radix):
    emu.tune(ntt_tile_log=tile, ntt_max_radix_log=radix)
    try:
        for kind in KINDS:
            pc.check_ntt(emu, orc, pyref, 6, seed=6, kind=kind, inverse=kind in ("const", "minus_one", "geometric", "half_negated"))
        _ntt_device_forms(emu, orc, pyref, 8, ("uniform",) + KINDS, single=False)
    finally:
        emu.tune(ntt_tile_log=6, ntt_max_radix_log=4)


def test_emulated_ntt_two_level_twiddle_path(emu, orc, pyref):
    emu.tune(ntt_full_twiddle_max_log=0)
    try:
        for kind in KINDS:
            pc.check_ntt(emu, orc, pyref, 5, seed=105, kind=kind)
        _ntt_device_forms(emu, orc, pyref, 9, ("uniform",) + KINDS, single=False)
        for kind in ("const", "minus_one", "geometric"):
            pc.check_ntt(emu, orc, pyref, 12, seed=112, kind=kind, inverse=kind == "geometric")
    finally:
        emu.tune(ntt_full_twiddle_max_log=24)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_ntt(gpu, orc, pyref, kind):
    """zk_ntt under the default plan (radix 2^8): one pass (2^8), two (2^13), three (2^17)"""
    for log_n in (3, 8, 13, 17):
        pc.check_ntt(gpu, orc, pyref, log_n, seed=log_n, kind=kind)
        pc.check_ntt(gpu, orc, pyref, log_n, seed=log_n + 1, kind=kind, inverse=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["const", "minus_one", "geometric"])
def test_gpu_ntt_2p20(gpu, orc, pyref, kind):
    pc.check_ntt(gpu, orc, pyref, 20, seed=20, kind=kind, inverse=kind == "minus_one")
    _ntt_device_forms(gpu, orc, pyref, 20, (kind,), seed=21)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [2, 8, 11, 16, 17])
def test_gpu_ntt_device_forms_mixed_batch(gpu, orc, pyref, log_n):
    _ntt_device_forms(gpu, orc, pyref, log_n, ("uniform",) + KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("tile,radix", [(10, 5), (11, 11), (12, 10), (12, 6)])
def test_gpu_ntt_other_plans(gpu, orc, pyref, tile, radix):
    gpu.tune(ntt_tile_log=tile, ntt_max_radix_log=radix)
    try:
        for kind in KINDS:
            for log_n in (4, 10, 14):
                pc.check_ntt(gpu, orc, pyref, log_n, seed=log_n, kind=kind, inverse=log_n == 10)
        _ntt_device_forms(gpu, orc, pyref, 16, ("uniform",) + KINDS, single=False)
    finally:
        gpu.tune(ntt_tile_log=10, ntt_max_radix_log=8)


@pytest.mark.gpu
def test_gpu_ntt_two_level_twiddle_path(gpu, orc, pyref):
    gpu.tune(ntt_full_twiddle_max_log=0)
    try:
        for kind in KINDS:
            for log_n in (9, 14):
                pc.check_ntt(gpu, orc, pyref, log_n, seed=100 + log_n, kind=kind, inverse=log_n == 9)
        _ntt_device_forms(gpu, orc, pyref, 17, ("uniform",) + KINDS, single=False)
    finally:
        gpu.tune(ntt_full_twiddle_max_log=24)


# ---- domain and coset forms -----------------------------------------------------------------------------------------------------------------------------------
def _domain_case(be, orc, pyref, j, k, kind, seed=51):
    """check_domain on columns of that kind (lagrange_to_coeff, coeff_to_extended, divide_by_vanishing_poly, extended_to_coeff: the fused-scaling and ZETA exits of the last
    store), coeff_to_lagrange, and the closed forms of a constant"""
    pc.check_domain(be, orc, pyref, j, k, seed=seed, kind=kind)
    od = orc.Domain(j, k)
    n, en = 1 << k, 1 << od.extended_k
    a = pc.column(orc, pyref, n, seed, kind)
    d = be.to_device(a)
    be.coeff_to_lagrange_dev(d, k)
    assert (d.download((n, 4)) == od.coeff_to_lagrange(a)).all(), kind
    if kind == "const":
        d.upload(a)
        be.lagrange_to_coeff_dev(d, k)                                 # a constant Lagrange column is the constant polynomial: a delta_first coefficient column
        coeff = d.download((n, 4))
        assert (coeff[0] == a[0]).all() and not coeff[1:].any()
        ext = be.alloc(en * 32)
        be.coeff_to_extended_dev(d, k, od.extended_k, ext)             # ... which takes that constant on every row of the extended domain
        assert (ext.download((en, 4)) == np.repeat(a[:1], en, axis=0)).all()
        ext.free()
    d.free()


@pytest.mark.parametrize("kind", DOMAIN_KINDS)
def test_emulated_domain(emu, orc, pyref, kind):
    _domain_case(emu, orc, pyref, 4, 5, kind)
    _domain_case(emu, orc, pyref, 5, 3, kind, seed=52)


def test_emulated_domain_batch_and_cosets(emu, orc, pyref):
    pc.check_domain_batch(emu, orc, pyref, 4, 5, len(DOMAIN_KINDS) + 1, kinds=("uniform",) + DOMAIN_KINDS)
    pc.check_domain_batch(emu, orc, pyref, 3, 2, len(DOMAIN_KINDS), kinds=DOMAIN_KINDS)
    for i in range(0, len(DOMAIN_KINDS), 3):
        tco._check(emu, orc, pyref, 7, 2, seed=7 + i, kinds=DOMAIN_KINDS[i:i + 3])       # coeff_to_coset_batch against coeff_to_extended, fr_interleave (k above the tile: the pre-scaling table)
    tco._check(emu, orc, pyref, 4, 1, seed=4, kinds=("zeros", "const", "minus_one"))
    tco._check_pieces(emu, orc, pyref, 4, 3, 8, seed=36, kinds=DOMAIN_KINDS)            # cosets_to_pieces: eight pieces of eight kinds
    tco._check_pieces(emu, orc, pyref, 5, 2, 3, seed=38, kinds=("witness", "zeros", "minus_one"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DOMAIN_KINDS)
def test_gpu_domain(gpu, orc, pyref, kind):
    _domain_case(gpu, orc, pyref, 4, 10, kind)
    _domain_case(gpu, orc, pyref, 5, 12, kind, seed=52)
    _domain_case(gpu, orc, pyref, 9, 8, kind, seed=53)


@pytest.mark.gpu
def test_gpu_domain_batch_and_cosets(gpu, orc, pyref):
    pc.check_domain_batch(gpu, orc, pyref, 5, 12, len(DOMAIN_KINDS) + 1, kinds=("uniform",) + DOMAIN_KINDS)
    pc.check_domain_batch(gpu, orc, pyref, 4, 6, len(DOMAIN_KINDS), kinds=DOMAIN_KINDS)
    for i in range(0, len(DOMAIN_KINDS), 3):
        tco._check(gpu, orc, pyref, 16 if i == 0 else 10, 2, seed=7 + i, kinds=DOMAIN_KINDS[i:i + 3])
    tco._check_pieces(gpu, orc, pyref, 16, 3, 7, seed=36, kinds=DOMAIN_KINDS)
    tco._check_pieces(gpu, orc, pyref, 12, 2, 3, seed=38, kinds=("witness", "selector_sparse", "minus_one"))


# ---- evaluations, kate_division -------------------------------------------------------------------------------------------------------------------------------
def _times_x_minus_b(q, b, R):
    """the coefficients of (X - b) * q(X), in Python integers"""
    a = [0] * (len(q) + 1)
    for i, c in enumerate(q):
        a[i + 1] = c
    for i, c in enumerate(q):
        a[i] = (a[i] - b * c) % R
    return a


def _eval_cases(be, orc, pyref, n, seed, full=True):
    R, rnd = pyref.R, random.Random(seed)
    M = orc.fr_from_ints
    zero = np.zeros(4, dtype=np.uint64)
    b = rnd.randrange(1, R)
    if n >= 2:
        # a polynomial with a root at the point: every value is 0 and every quotient is q itself — dense q, and a sparse q whose zero coefficients are exact cancellations
        for sparse in (False, True):
            q = [0 if sparse and rnd.random() < 0.8 else rnd.randrange(R) for _ in range(n - 1)]
            if sparse:
                q[-1] = q[0] = 0
                q[(n - 1) // 2] = 1
            a = M(_times_x_minus_b(q, b, R))
            got, quot = tep._check(be, orc, pyref, n, 1, seed, points=[M([b])[0]], polys=[a])
            assert not got[0].any(), "the value at a root is the canonical zero"
            assert (quot == M(q)).all()
    # the points 0, 1, r - 1 and omega; r - 1 everywhere at the point -1; zeros; one top coefficient
    log_n = max(n - 1, 1).bit_length()
    kinds = ["uniform", "uniform", "uniform", "uniform", "minus_one", "minus_one", "neg_one", "zeros", "delta_last", "delta_last", "delta_first"]
    points = [zero, M([1])[0], M([R - 1])[0], M([pyref.omega(log_n)])[0], M([R - 1])[0], pc._raw([R - 1])[0], M([R - 1])[0], M([b])[0], M([b])[0], zero, M([R - 1])[0]]
    if full:
        kinds += ["witness", "selector", "top", "alt_pm", "geometric"]
        points += [M([b])[0], M([1])[0], pc._raw([R - 1])[0], M([R - 1])[0], M([pow(pyref.omega(log_n), -3, R)])[0]]
    got, _ = tep._check(be, orc, pyref, n, len(kinds), seed + 1, kinds=kinds, points=points)
    assert not got[kinds.index("zeros")].any()
    if n >= 2:
        assert not got[9].any()                                        # delta_last at the point 0
    # kate_division: the point 0 (the quotient is the coefficients shifted down), and zeros / r - 1 everywhere / one top coefficient at a uniform point
    if n >= 2:
        u = pc.rand_fr(orc, pyref, n, seed + 2)
        assert (z.arithmetic.kate_division(u, zero, backend=be) == u[1:]).all()
        for kind in ("zeros", "minus_one", "delta_last", "witness"):
            a = pc.structured_fr(orc, pyref, n, kind, seed + 3)
            for pt in (M([b])[0], M([R - 1])[0]):
                got_q = z.arithmetic.kate_division(a, pt, backend=be)
                assert (got_q == orc.kate_division(a, pt)).all(), (kind, n)
            if kind == "zeros":
                assert not got_q.any()


@pytest.mark.parametrize("n", [1, 2, 100, 2048, 2049, 32255, 32256, 32257])      # 2048: one workgroup of kate_division; 32256 = 256 x 126: the span of a workgroup of eval_polynomial
def test_emulated_evaluations(emu, orc, pyref, n):
    _eval_cases(emu, orc, pyref, n, seed=n, full=n <= 2049)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 2049, 32255, 32256, 32257, 100003, (1 << 20) + 4099])      # the last one: kate_division carries over two rounds of workgroups
def test_gpu_evaluations(gpu, orc, pyref, n):
    _eval_cases(gpu, orc, pyref, n, seed=n, full=n < (1 << 20))


# ---- fr_lincomb -----------------------------------------------------------------------------------------------------------------------------------------------
def _lincomb_cases(be, orc, pyref, n, seed):
    R, rnd = pyref.R, random.Random(seed)
    M = orc.fr_from_ints
    u, v, w = (pc.rand_fr(orc, pyref, n, seed + i) for i in range(3))
    s, t = rnd.randrange(1, R), rnd.randrange(1, R)
    L = lambda polys, scalars: tep._check_lincomb(be, orc, pyref, n, len(polys), seed, polys=polys, scalars=scalars)
    L([u, u], M([s, R - s]))                                           # s * u + (r - s) * u: exactly 0 on every row
    L([u, v, u, v], M([s, t, R - s, R - t]))
    L([u, v, w], M([s, 0, t]))                                         # a zero scalar
    L([u, v, w], M([0, 0, 0]))
    L([u, v, w], M([s, 1, t]))                                         # the scalar 1 in other positions than the first
    L([u, v, w], M([s, t, 1]))
    L([pc.structured_fr(orc, pyref, n, "zeros", 0), pc.structured_fr(orc, pyref, n, "witness", seed), pc.structured_fr(orc, pyref, n, "selector", seed)], M([s, t, R - 1]))
    # r - 1 everywhere under the scalar -1 (and under the scalar whose limbs are r - 1): a full chunk of six, a chunk of one, the reduction that runs every 16 chunks (96 terms),
    # one term past it, and counts whose running total would pass the 32 p the reduction keeps it under
    m1 = pc.structured_fr(orc, pyref, n, "minus_one", 0)
    for count in (6, 7, 96, 97, 200, 600):
        L([m1] * count, np.repeat(M([R - 1]), count, axis=0))
    L([m1] * 200, np.repeat(pc._raw([R - 1]), 200, axis=0))
    L([m1, u] * 100, M([R - 1, s] * 100))


def _lincomb_long(be, orc, pyref, n, seed):
    """20000 terms.  The periodic reduction keeps the running total below 32 p; what it protects is the top limb of the 9 x 29-bit total, which holds 2^264 (about 1000 p: the
    quotient estimate of the final reduction stays right up to there).  A chunk of six adds half a p on average, so a total that is never reduced wraps after some 2000 chunks:
    nothing shorter than about 12000 terms can tell whether the reduction runs."""
    R, rnd = pyref.R, random.Random(seed)
    m1, u = pc.structured_fr(orc, pyref, n, "minus_one", 0), pc.rand_fr(orc, pyref, n, seed)
    tep._check_lincomb(be, orc, pyref, n, 20000, seed, polys=[m1, u] * 10000, scalars=orc.fr_from_ints([rnd.randrange(R) for _ in range(20000)]))


def test_emulated_lincomb(emu, orc, pyref):
    _lincomb_cases(emu, orc, pyref, 77, seed=3)                        # (three workgroups of the fixture's 32 threads, the last one partial)
    _lincomb_long(emu, orc, pyref, 33, seed=4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 10007])
def test_gpu_lincomb(gpu, orc, pyref, n):
    _lincomb_cases(gpu, orc, pyref, n, seed=n % 1000)
    if n == 1:
        _lincomb_long(gpu, orc, pyref, 257, seed=4)


# ---- grand products -------------------------------------------------------------------------------------------------------------------------------------------
def _division_rows(n, bf, place, dblk):
    """rows of a column of n rows (a batch of one: gp_batch_divide_kernel runs ceil(n / 32) threads, thread g chains the rows g, g + threads, ..: 32 strided rows)"""
    nth = (n + 31) // 32
    if place == "row0_last":
        return [0, n - bf - 2]
    if place == "chain":                                               # two inside one thread's chain; the first and the last row of another thread's chain
        g, h = min(5, nth - 1), min(9, nth - 1)
        return [g + 3 * nth, g + 7 * nth, h, h + 31 * nth]
    if place == "workgroup":                                           # every row of the second workgroup of the division kernel (the first, when there is only one)
        wg = 1 if nth >= 2 * dblk else 0
        return [g + j * nth for g in range(wg * dblk, min((wg + 1) * dblk, nth)) for j in range(32) if g + j * nth < n]
    if place == "column":
        return list(range(n))
    raise ValueError(place)


def _gp_inputs(orc, pyref, k, count, seed, zero_den=(), zero_num=(), identity=False, equal_pair=False, j0=3, num_col=0):
    """test_grand_product._inputs with zero denominators (sigma = -(v + gamma) / beta in the last column, whose value is -beta there: the lookup's denominator is zero too),
    zero numerators (column num_col: v = -gamma - delta^(j0 + num_col) omega^i beta; sigma of column 0 = -gamma: the lookup's numerator), sigma = the identity permutation
    (every fraction exactly 1), or a second column equal to the first (the lookup's permuted pair equals its compressed pair)"""
    R = pyref.R
    n = 1 << k
    vals, sig, beta, gamma = tgp._inputs(orc, pyref, k, count, seed)
    b, g = orc.fr_to_ints(beta)[0], orc.fr_to_ints(gamma)[0]
    M = orc.fr_from_ints
    w = pyref.omega(k)
    if identity:
        wp = pc.fr_powers(orc, M([w])[0], n)
        sig = [orc.fr_mul(wp, np.repeat(M([pow(pyref.DELTA, j0 + j, R)]), n, axis=0)) for j in range(count)]
    if equal_pair:
        vals[-1], sig[-1] = vals[0].copy(), sig[0].copy()
    zero_den, zero_num = sorted(set(zero_den)), sorted(set(zero_num))
    if zero_num:
        vals[num_col][zero_num] = M([(-g - pow(pyref.DELTA, j0 + num_col, R) * pow(w, i, R) * b) % R for i in zero_num])
        sig[0][zero_num] = M([(-g) % R])[0]
    if zero_den:
        vals[-1][zero_den] = M([(-b) % R])[0]
        sig[-1][zero_den] = M([(-(g - b) * pow(b, -1, R)) % R])[0]
    return vals, sig, beta, gamma


def _grand_product_cases(be, orc, pyref, k, dblk, seed, k2):
    n, bf = 1 << k, 5
    M = orc.fr_from_ints
    for place in ("row0_last", "chain", "workgroup", "column"):
        rows = _division_rows(n, bf, place, dblk)
        want, want_l = tgp._check_backend(be, orc, pyref, k, 2, seed, inputs=_gp_inputs(orc, pyref, k, 2, seed, zero_den=rows))
        if place == "column":                                           # every fraction is 0: z = z0, 0, 0, ...
            assert not want[1:n - bf].any() and not want_l[1:n - bf].any()
    # zero numerators: z is 0 from there on — inside a scan span, and (k2: more than one span per column) through the workgroup totals
    for kk, row in ((k, (1 << k) // 3), (k2, 100)):
        nn = 1 << kk
        want, want_l = tgp._check_backend(be, orc, pyref, kk, 3, seed + 1, inputs=_gp_inputs(orc, pyref, kk, 3, seed + 1, zero_num=[row], zero_den=[row + 7]))
        assert want[row].any() and not want[row + 1:nn - bf].any() and not want_l[row + 1:nn - bf].any()
    # the satisfied shapes: sigma = identity (every fraction exactly 1, z stays at z0); a lookup whose permuted pair equals its compressed pair (z stays at 1)
    want, _ = tgp._check_backend(be, orc, pyref, k, 3, seed + 2, inputs=_gp_inputs(orc, pyref, k, 3, seed + 2, identity=True))
    assert (want[:n - bf] == want[0]).all()
    _, want_l = tgp._check_backend(be, orc, pyref, k, 2, seed + 3, inputs=_gp_inputs(orc, pyref, k, 2, seed + 3, equal_pair=True))
    assert (want_l[:n - bf] == M([1])[0]).all()
    # permutation_commit (all sets in one call, chained through inits[s]): zero denominators, a zero numerator in set 0 resp. set 1 (every later set starts at 0), the identity
    for kk in (k, k2):
        nn = 1 << kk
        tgp._check_commit(be, orc, pyref, kk, inputs=_gp_inputs(orc, pyref, kk, 5, 21, zero_den=[0, nn - bf - 2, nn // 2], j0=0))
        zs = tgp._check_commit(be, orc, pyref, kk, inputs=_gp_inputs(orc, pyref, kk, 5, 22, zero_num=[nn // 2 + 3], j0=0, num_col=0))
        assert not zs[0][nn // 2 + 4:nn - bf].any() and not zs[1][:nn - bf].any() and not zs[2][:nn - bf].any()
        zs = tgp._check_commit(be, orc, pyref, kk, inputs=_gp_inputs(orc, pyref, kk, 5, 23, zero_num=[nn - bf - 2], j0=0, num_col=3))
        assert zs[1][nn - bf - 2].any() and not zs[1][nn - bf - 1].any() and not zs[2][:nn - bf].any()
    zs = tgp._check_commit(be, orc, pyref, k, inputs=_gp_inputs(orc, pyref, k, 5, 24, identity=True, j0=0))
    for zz in zs:
        assert (zz[:n - bf] == M([1])[0]).all()
    zs = tgp._check_commit(be, orc, pyref, k, inputs=_gp_inputs(orc, pyref, k, 5, 25, zero_den=range(n), j0=0))


def test_emulated_grand_products(emu, orc, pyref):
    _grand_product_cases(emu, orc, pyref, 11, 32, seed=113, k2=12)     # 2^11: 64 division threads in two workgroups of the fixture's 32, one scan span; 2^12: two spans


@pytest.mark.gpu
def test_gpu_grand_products(gpu, orc, pyref):
    _grand_product_cases(gpu, orc, pyref, 16, 256, seed=163, k2=13)    # 2^16: 2048 division threads in eight workgroups, 32 scan spans


# ---- quotient -------------------------------------------------------------------------------------------------------------------------------------------------
def _shapes():
    from test_quotient import SHAPES
    return SHAPES


@pytest.mark.parametrize("kind", QUOTIENT_KINDS)
def test_emulated_quotient(emu, orc, pyref, kind):
    for seed, shape in _shapes():
        qc.run_case(emu, orc, pyref, pc, qc.build_program(orc, pyref, seed=seed, **shape), seed=seed, kind=kind)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
@pytest.mark.parametrize("kind", QUOTIENT_KINDS)
def test_gpu_quotient(gpu, orc, pyref, kind, jit):
    """the interpreter, and the generated kernels (cut after every 6 products: accumulator and slots cross many kernel boundaries)"""
    gpu.tune(quot_jit=jit, quot_jit_group=6)
    try:
        for seed, shape in _shapes() + [(5, dict(k=8, cs_degree=5, n_fixed=4, n_advice=6, n_instance=1, n_challenges=1, n_perm=7, n_lookups=3))]:
            qc.run_case(gpu, orc, pyref, pc, qc.build_program(orc, pyref, seed=seed, **shape), seed=seed, kind=kind, expect_kernels=1 if jit else False)
    finally:
        gpu.tune(quot_jit=0, quot_jit_group=200)


def _accumulate_cancels(be, orc, k, kinds):
    """zk_quotient_run_acc_dev with the previous value -N * y^(-E): previous * y^E + N is exactly 0 on every row, every route and part"""
    import test_create_proof as tcp
    import test_multi_circuit as tmc
    cs, fixed, asm, _, _ = tcp.toy_circuit(k)
    for i, kind in enumerate(kinds):
        tmc._acc_kernel(be, k, (cs, fixed, asm), 11 + i, cancel=True, kind=kind, orc=orc)


def test_emulated_accumulate_mode_cancels(emu, orc, pyref):
    _accumulate_cancels(emu, orc, 5, ("uniform", "witness"))


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
def test_gpu_accumulate_mode_cancels(gpu, orc, pyref, jit):
    gpu.tune(quot_jit=jit, quot_jit_group=64)
    try:
        _accumulate_cancels(gpu, orc, 9, ("uniform", "witness", "minus_one", "zeros"))
    finally:
        gpu.tune(quot_jit=0, quot_jit_group=200)


# ---- vector operations ----------------------------------------------------------------------------------------------------------------------------------------
def test_emulated_vec_ops(emu, orc, pyref):
    for pair in pc.structured_vec_pairs(orc, pyref, 77):               # three workgroups of 32, the last one partial
        pc.check_vec_ops(emu, orc, pyref, 77, operands=pair)


@pytest.mark.gpu
def test_gpu_vec_ops(gpu, orc, pyref):
    for pair in pc.structured_vec_pairs(orc, pyref, 100003):
        pc.check_vec_ops(gpu, orc, pyref, 100003, operands=pair)
