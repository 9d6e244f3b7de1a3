"""Point cases shared by the emulator tests (CPU, small) and the GPU tests (through the product C ABI): STRUCTURED G1 tables — one point on every row, P / -P
alternating, a few small multiples of G, pairs, mostly identities — and the scalar columns that make the group law's exceptional cases (P + P, P + (-P), identity
operands) happen at every level of the MSM, of the G1 NTT and of the affine conversion.  Every base is [k_i] G for a KNOWN k_i, so every MSM has two independent
references, both compared bit for bit over all 12 output limbs: the oracle's best_multiexp on the same table, and the closed form [sum s_i k_i mod r] G through one
g1_mul (which does not share the oracle's bucket method)."""
import ctypes as C
import random

import numpy as np

import parity_cases as pc
import zk_dcap_verifier_amd as z
from zk_dcap_verifier_amd.transcript import point_to_bytes

POINT_KINDS = ("all_equal", "alt_neg", "few", "small_multiples", "pairs", "neg_pairs", "identity_heavy", "all_identity")
SCALAR_KINDS = ("uniform", "ones", "minus_one", "witness", "zeros", "paired", "neg_paired", "byte", "one_digit")
IDENTITY_CASES = (("alt_neg", "ones"), ("neg_pairs", "paired"), ("pairs", "neg_paired"), ("all_identity", "uniform"), ("all_identity", "ones"), ("all_identity", "minus_one"))


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------------
def neg_rows(orc, rows):
    """-P for every affine row (the oracle's Fq subtraction: 0 - y; an identity row (0, 0) stays the identity)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 8).copy()
    rows[:, 4:] = orc.fq_sub(np.zeros((rows.shape[0], 4), dtype=np.uint64), np.ascontiguousarray(rows[:, 4:]))
    return rows


def g_times(orc, k):
    """the affine row of [k] G (k = 0: the identity row)"""
    return orc.g1_to_affine(orc.g1_mul(orc.g1_generator(), orc.fr_from_ints([k])[0]))[0]


def structured_bases(orc, pyref, n, kind, seed=0):
    """(table, ks): an (n, 8) affine table of one of POINT_KINDS and the integers k_i in [0, r) with table[i] = [k_i] G (0 = the identity row)
    all_equal        one seeded point on every row
    alt_neg          P, -P, P, -P, ..
    few              k_i drawn from {+-1, +-2, +-3, +-4}: equal and opposite points at every level, against accumulators that are sums (ZZ != 1)
    small_multiples  k_i = i + 1
    pairs/neg_pairs  row 2i + 1 equals, resp. negates, row 2i; the even rows are an arithmetic progression of generic points
    identity_heavy   about 90 % identity rows — row 0, the last row and whole runs of rows among them — the others generic
    all_identity     nothing else"""
    R, rnd = pyref.R, random.Random(seed * 104729 + 7)
    if kind == "all_identity":
        return np.zeros((n, 8), dtype=np.uint64), [0] * n
    if kind in ("all_equal", "alt_neg"):
        k = rnd.randrange(1, R)
        row = g_times(orc, k)
        tab = np.ascontiguousarray(np.repeat(row.reshape(1, 8), n, axis=0))
        ks = [k] * n
        if kind == "alt_neg":
            tab[1::2] = neg_rows(orc, row)[0]
            ks[1::2] = [R - k] * len(ks[1::2])
        return tab, ks
    if kind == "few":
        pos = np.stack([g_times(orc, m) for m in (1, 2, 3, 4)])
        rows = np.concatenate([pos, neg_rows(orc, pos)])              # index j < 4: [j + 1] G, else -[j - 3] G
        vals = [1, 2, 3, 4, R - 1, R - 2, R - 3, R - 4]
        pick = [rnd.randrange(8) for _ in range(n)]
        return np.ascontiguousarray(rows[pick]), [vals[j] for j in pick]
    if kind == "small_multiples":
        return orc.gen_bases_arith(1, 1, n), list(range(1, n + 1))
    if kind in ("pairs", "neg_pairs"):
        h = (n + 1) // 2
        a0, d = rnd.randrange(1, R), rnd.randrange(1, R)
        half = orc.gen_bases_arith(a0, d, h)
        tab = np.empty((2 * h, 8), dtype=np.uint64)
        tab[0::2] = half
        tab[1::2] = half if kind == "pairs" else neg_rows(orc, half)
        ks = []
        for i in range(h):
            k = (a0 + i * d) % R
            ks += [k, k if kind == "pairs" else (R - k) % R]
        return np.ascontiguousarray(tab[:n]), ks[:n]
    if kind == "identity_heavy":
        a0, d = rnd.randrange(1, R), rnd.randrange(1, R)
        tab = orc.gen_bases_arith(a0, d, n)
        ks = [(a0 + i * d) % R for i in range(n)]
        dead = np.zeros(n, dtype=bool)
        for lo in range(0, n, 8):                                      # whole runs of eight, and single rows inside the others
            if rnd.random() < 0.85:
                dead[lo:lo + 8] = True
            else:
                dead[lo:lo + 8] = [rnd.random() < 0.35 for _ in range(min(8, n - lo))]
        dead[0] = dead[n - 1] = True
        if n >= 4:
            dead[n // 2] = False                                      # (never the empty table)
        tab[dead] = 0
        return np.ascontiguousarray(tab), [0 if dd else k for dd, k in zip(dead.tolist(), ks)]
    raise ValueError(kind)


def delta_points(orc, pyref, n, where, seed=0):
    """one non-identity point, at row 0, n / 2 or n - 1 (where = 'first' / 'mid' / 'last')"""
    k = random.Random(seed * 31 + 5).randrange(1, pyref.R)
    tab, ks = np.zeros((n, 8), dtype=np.uint64), [0] * n
    i = {"first": 0, "mid": n // 2, "last": n - 1}[where]
    tab[i], ks[i] = g_times(orc, k), k
    return tab, ks


# ---- scalar columns -------------------------------------------------------------------------------------------------------------------------------------------
def scalar_column(orc, pyref, n, kind, seed=0, c=16):
    """an (n, 4) column of Montgomery forms: the kinds of parity_cases.msm_inputs, and
    paired      s[2i + 1] = s[2i], uniform otherwise (over `pairs`: every chain doubles; over `neg_pairs`: every bucket cancels)
    neg_paired  s[2i + 1] = -s[2i] (over `pairs`: the windows differ, only the total cancels — in the fold over the class sums)
    byte        values below 256: only the lowest window(s) are populated, every other class sum is the identity
    one_digit   2^(c w) for w in {0, 1, the middle window, the top window}: one non-zero digit, a 1, per scalar"""
    R, rnd = pyref.R, random.Random(seed * 7919 + 3)
    if kind == "uniform":
        return pc.rand_fr(orc, pyref, n, seed)
    if kind in ("ones", "zeros", "minus_one"):
        return np.ascontiguousarray(np.repeat(orc.fr_from_ints([{"ones": 1, "zeros": 0, "minus_one": R - 1}[kind]]), n, axis=0))
    if kind == "witness":
        return pc.structured_fr(orc, pyref, n, "witness", seed)
    if kind in ("paired", "neg_paired"):
        s = pc.rand_fr(orc, pyref, n, seed)
        m = n // 2
        if m:
            ev = np.ascontiguousarray(s[0:2 * m:2])
            s[1:2 * m:2] = ev if kind == "paired" else orc.fr_sub(np.zeros((m, 4), dtype=np.uint64), ev)
        return s
    if kind == "byte":
        return orc.fr_from_ints([rnd.randrange(256) for _ in range(n)])
    if kind == "one_digit":
        top = 254 // c
        while (1 << (c * top)) >= R:
            top -= 1
        ws = sorted({0, min(1, top), top // 2, top})
        return orc.fr_from_ints([1 << (c * ws[rnd.randrange(len(ws))]) for _ in range(n)])
    raise ValueError(kind)


# ---- the two references ---------------------------------------------------------------------------------------------------------------------------------------
def _g1_12(orc, pyref, jac):
    """Jacobian -> the 12 limbs the library returns: affine x, y and z = mont(1), or all zero for the identity"""
    aff = orc.g1_to_affine(jac)[0]
    out = np.zeros(12, dtype=np.uint64)
    if aff.any():
        out[:8] = aff
        out[8:] = orc.ints_to_limbs([pyref.mont_r(pyref.P)])[0]
    return out


def closed_form(orc, pyref, sc, ks):
    """[sum s_i k_i mod r] G by one g1_mul"""
    total = sum(s * k for s, k in zip(orc.fr_to_ints(sc), ks) if s and k) % pyref.R
    return _g1_12(orc, pyref, orc.g1_mul(orc.g1_generator(), orc.fr_from_ints([total])[0])), total


def expected(orc, pyref, sc, bases, ks, closed_only=False):
    """the 12 expected limbs; unless closed_only, the oracle's best_multiexp must give the very same limbs (a disagreement is the oracle's bug)"""
    want, total = closed_form(orc, pyref, sc, ks)
    if not closed_only:
        me = _g1_12(orc, pyref, orc.best_multiexp(sc, bases))
        assert (me == want).all(), "the oracle's best_multiexp disagrees with its own g1_mul"
    return want, total


def assert_point(got, want, what):
    assert np.asarray(got).shape == (12,) and (np.asarray(got) == want).all(), what


# ---- MSM cases ------------------------------------------------------------------------------------------------------------------------------------------------
def check_structured_msm(be, orc, pyref, n, bkind, skind, seed=1, c=16, closed_only=False, entries=("host", "dev"), table=None):
    """zk_msm (host scalars) and zk_msm_dev (device scalars) on a structured table; returns the integer the result is a multiple of G by"""
    bases, ks = table if table is not None else structured_bases(orc, pyref, n, bkind, seed)
    sc = scalar_column(orc, pyref, n, skind, seed + 1, c=c)
    want, total = expected(orc, pyref, sc, bases, ks, closed_only)
    if (bkind, skind) in IDENTITY_CASES and (bkind != "alt_neg" or n % 2 == 0) and (bkind not in ("pairs", "neg_pairs") or n % 2 == 0):
        assert total == 0 and not want.any(), (bkind, skind)
    h = z.arithmetic.BasesHandle(be, bases)
    try:
        if "host" in entries:
            assert_point(be.msm(h.handle, sc), want, ("zk_msm", n, bkind, skind))
        if "dev" in entries:
            d = be.to_device(sc)
            assert_point(be.msm(h.handle, d, n), want, ("zk_msm_dev", n, bkind, skind))
            d.free()
    finally:
        h.release()
    return total


def check_structured_batch(be, orc, pyref, n, bkind, seed=2, device=False, c=16, skinds=SCALAR_KINDS):
    """zk_msm_batch / zk_msm_batch_dev: ONE batch that mixes the scalar kinds over one structured table; every column against both references and against the single call"""
    bases, ks = structured_bases(orc, pyref, n, bkind, seed)
    cols = [scalar_column(orc, pyref, n, sk, seed + 3 * i, c=c) for i, sk in enumerate(skinds)]
    h = z.arithmetic.BasesHandle(be, bases)
    try:
        if device:
            dcols = [be.to_device(col) for col in cols]
            got = be.msm_batch(h.handle, dcols, n)
            for d in dcols:
                d.free()
        else:
            got = z.arithmetic.best_multiexp_batch(cols, h)
        for i, (sk, col) in enumerate(zip(skinds, cols)):
            want, _ = expected(orc, pyref, col, bases, ks)
            assert_point(got[i], want, ("batch", n, bkind, sk))
            assert (z.arithmetic.best_multiexp(col, h) == got[i]).all(), ("single != batch", bkind, sk)
    finally:
        h.release()


def check_partials(be, orc, pyref, n, bkind, seed=3, skind="uniform"):
    """zk_msm_partial_dev + zk_g1_sum_xyzz and zk_msm_batch_partial_dev + zk_g1_sum_xyzz_batch: two EQUAL partial sums (the host sum doubles), partial sums of s and
    of -s (it cancels), three equal ones, identity partial sums"""
    R = pyref.R
    bases, ks = structured_bases(orc, pyref, n, bkind, seed)
    s = scalar_column(orc, pyref, n, skind, seed + 1)
    neg = orc.fr_sub(np.zeros((n, 4), dtype=np.uint64), s)
    zero = np.zeros((n, 4), dtype=np.uint64)
    _, total = expected(orc, pyref, s, bases, ks)
    mul = lambda m: _g1_12(orc, pyref, orc.g1_mul(orc.g1_generator(), orc.fr_from_ints([m * total % R])[0]))
    ident = np.zeros(12, dtype=np.uint64)
    h = z.arithmetic.BasesHandle(be, bases)
    ds, dn, dz = be.to_device(s), be.to_device(neg), be.to_device(zero)
    try:
        p1, p2, pn, pz = be.msm_partial(h.handle, ds, n), be.msm_partial(h.handle, ds, n), be.msm_partial(h.handle, dn, n), be.msm_partial(h.handle, dz, n)
        assert_point(be.g1_sum_xyzz(np.stack([p1])), mul(1), ("one partial", bkind))
        assert_point(be.g1_sum_xyzz(np.stack([p1, p2])), mul(2), ("s + s", bkind))
        assert_point(be.g1_sum_xyzz(np.stack([p1, pn])), ident, ("s + (-s)", bkind))
        assert_point(be.g1_sum_xyzz(np.stack([p1, p2, p1])), mul(3), ("s + s + s", bkind))
        assert_point(be.g1_sum_xyzz(np.stack([pz, p1, pz, pn, p2])), mul(1), ("0 + s + 0 - s + s", bkind))
        assert_point(be.g1_sum_xyzz(np.stack([pz, pz])), ident, ("0 + 0", bkind))
        bp = be.msm_batch_partial(h.handle, [ds, dn, ds, dz], n)       # columns s, -s, s, 0
        for i, want in enumerate((mul(1), mul(R - 1), mul(1), ident)):  # (a partial sum is any XYZZ form of its point: only normalised results are compared)
            assert_point(be.g1_sum_xyzz(bp[i:i + 1]), want, ("one batch partial", bkind, i))
        got = be.g1_sum_xyzz_batch(np.stack([bp, bp[[1, 0, 2, 3]], bp[[3, 3, 0, 3]]]))      # s - s + 0, -s + s + 0, s + s + s, 0 + 0 + 0
        for i, want in enumerate((ident, ident, mul(3), ident)):
            assert_point(got[i], want, ("batch partial", bkind, i))
        got = be.g1_sum_xyzz_batch(np.stack([bp, bp]))
        for i, want in enumerate((mul(2), mul(R - 2), mul(2), ident)):
            assert_point(got[i], want, ("batch partial doubled", bkind, i))
    finally:
        for d in (ds, dn, dz):
            d.free()
        h.release()


def check_prefix(be, orc, pyref, n, bkind, skind, seed=4):
    """a prefix of a registered structured table, several MSMs on one registration"""
    bases, ks = structured_bases(orc, pyref, n, bkind, seed)
    sc = scalar_column(orc, pyref, n, skind, seed + 1)
    h = z.arithmetic.BasesHandle(be, bases)
    try:
        for m in (n, n - 1, max(1, n // 3), 2, 1):
            want, _ = expected(orc, pyref, sc[:m], bases[:m], ks[:m])
            assert_point(z.arithmetic.best_multiexp(np.ascontiguousarray(sc[:m]), h), want, ("prefix", bkind, skind, m))
    finally:
        h.release()


def check_runs(be, orc, pyref, n, bkind, seed=5):
    """zk_bases_enable_runs on a structured table: the prefix-sum table then has identity entries (alt_neg: P, 0, P, 0, ..), doubling steps (all_equal: P, 2P, 3P, ..)
    or long constant stretches (identity_heavy).  A constant column, a constant column with a uniform tail and a sorted column go through it (msm_runs = 2), next to a
    uniform column that stays direct; then msm_runs = 0 must give the same answers."""
    R, rnd = pyref.R, random.Random(seed)
    bases, ks = structured_bases(orc, pyref, n, bkind, seed)
    big = [rnd.randrange(1, R) for _ in range(6)]
    cols = [orc.fr_from_ints(col) for col in ([big[0]] * n, [big[1]] * (n - 3) + [rnd.randrange(R) for _ in range(3)], sorted(rnd.choice(big) for _ in range(n)))]
    cols.append(pc.rand_fr(orc, pyref, n, seed))
    wants = [expected(orc, pyref, col, bases, ks)[0] for col in cols]
    h = z.arithmetic.BasesHandle(be, bases).enable_runs()
    be.timing(True)
    be.tune(msm_runs=2)
    try:
        got = z.arithmetic.best_multiexp_batch(cols, h)
        assert be.stat_get("msm_run_columns") >= 2
        for i, want in enumerate(wants):
            assert_point(got[i], want, ("runs", bkind, i))
        for i in (0, 2):
            assert_point(z.arithmetic.best_multiexp(cols[i], h), wants[i], ("runs, single", bkind, i))
        m = n - n // 3
        want, _ = expected(orc, pyref, cols[0][:m], bases[:m], ks[:m])
        assert_point(z.arithmetic.best_multiexp(np.ascontiguousarray(cols[0][:m]), h), want, ("runs, prefix", bkind))
        be.tune(msm_runs=0)
        got0 = z.arithmetic.best_multiexp_batch(cols, h)
        assert (got0 == got).all(), ("msm_runs = 0", bkind)
    finally:
        be.tune(msm_runs=1)
        be.timing(False)
        h.release()


# ---- G1 NTT ---------------------------------------------------------------------------------------------------------------------------------------------------
NTT_POINT_KINDS = ("all_equal", "alt_neg", "all_identity", "few", "identity_heavy", "delta_first", "delta_mid", "delta_last")


def check_g1_ntt(be, orc, pyref, log_n, kind, seed=6):
    """zk_g1_ntt_dev with and without scale against orc.g1_fft, and the closed forms: a constant column transforms to [n scale] P at index 0 and identities, P, -P, ..
    to [n scale] P at index n / 2 and identities (every butterfly on the way is a doubling next to a cancellation)"""
    R, n = pyref.R, 1 << log_n
    pts, ks = delta_points(orc, pyref, n, kind[6:], seed) if kind.startswith("delta_") else structured_bases(orc, pyref, n, kind, seed)
    w = orc.fr_from_ints([pow(pyref.omega(log_n), -1, R)])[0]
    scale = pow(n, -1, R) if seed % 2 else random.Random(seed).randrange(2, R)
    d, o = be.to_device(pts), be.alloc(n * 64)
    try:
        for sc_int in (scale, None):
            sc = orc.fr_from_ints([sc_int])[0] if sc_int is not None else None
            be.g1_ntt_dev(d, log_n, w, sc, o)
            got = o.download((n, 8))
            assert (got == orc.g1_fft(pts, log_n, w, sc)).all(), (log_n, kind, sc_int is not None)
            if kind in ("all_equal", "alt_neg", "all_identity") and n >= 2:
                at = {"all_equal": 0, "alt_neg": n // 2, "all_identity": None}[kind]
                want = np.zeros((n, 8), dtype=np.uint64)
                if at is not None:
                    want[at] = g_times(orc, n * ks[0] * (sc_int if sc_int is not None else 1) % R)
                assert (got == want).all(), ("closed form", log_n, kind)
    finally:
        d.free()
        o.free()


# ---- fixed-base multiplication --------------------------------------------------------------------------------------------------------------------------------
def fixed_base_scalars(orc, pyref, seed=7):
    """0, 1, r - 1; 256^w, 256^w - 1 and d 256^w for every byte window w (one table row alone; every lower row at its last entry; a seeded entry); witness / top / low"""
    R, rnd = pyref.R, random.Random(seed)
    vals = [0, 1, R - 1]
    for w in range(32):
        vals += [v % R for v in ((1 << (8 * w)), (1 << (8 * w)) - 1, rnd.randrange(2, 256) * (1 << (8 * w)), 255 * (1 << (8 * w)))]
    col = orc.fr_from_ints(vals)
    return np.ascontiguousarray(np.concatenate([col] + [pc.structured_fr(orc, pyref, 40, kd, seed) for kd in ("witness", "top", "low")]))


def check_fixed_base_structured(be, orc, pyref, seed=7, pad_to=None):
    """zk_g1_fixed_base_mul_dev on fixed_base_scalars (padded with uniform scalars to pad_to rows), every output against orc.g1_mul"""
    sc = fixed_base_scalars(orc, pyref, seed)
    if pad_to and pad_to > sc.shape[0]:
        sc = np.ascontiguousarray(np.concatenate([sc, pc.rand_fr(orc, pyref, pad_to - sc.shape[0], seed)]))
    n = sc.shape[0]
    ds, dout = be.to_device(sc), be.alloc(n * 64)
    try:
        be.g1_fixed_base_mul(ds, n, dout)
        got = dout.download((n, 8))
        g = orc.g1_generator()
        want = orc.g1_to_affine(np.stack([orc.g1_mul(g, s) for s in sc]))
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, bad[:8]
        assert not got[0].any() and (got[1] == g[0]).all()
    finally:
        ds.free()
        dout.free()
    return n


# ---- point codec ----------------------------------------------------------------------------------------------------------------------------------------------
def _encode(pt, sign_bit):
    """the definition in Python integers: x little-endian, the parity of y in the flag bit; identity = all zero (255) or bit 255 alone (254)"""
    if pt is None:
        return bytes(32) if sign_bit == 255 else bytes(31) + b"\x80"
    b = bytearray(pt[0].to_bytes(32, "little"))
    b[31] |= (pt[1] & 1) << (7 if sign_bit == 255 else 6)
    return bytes(b)


def _words(raw):
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def decompress_counting(be, words, sign_bit, out_dev):
    """zk_g1_decompress_dev through the C ABI itself: (return code, *n_invalid) — the Python wrapper only raises"""
    n = words.shape[0]
    b = be.to_device(words)
    bad = C.c_uint32(0xFFFFFFFF)
    rc = be.lib.zk_g1_decompress_dev(be.ctx, C.c_void_p(b.ptr), C.c_size_t(n), C.c_uint32(sign_bit), C.c_void_p(out_dev.ptr), C.byref(bad))
    b.free()
    return rc, bad.value


def check_codec(be, orc, pyref, n, sign_bit, seed=8):
    """n encodings, n not a multiple of the block: the points of a `few` table and of a generic one (both parities of y in bulk), identities at the head, in the middle
    and at the tail — decompressed against Python integers, compressed back to the same bytes.  Then the same batch with bad words planted (x = p, p + 1, 2^254 - 1,
    x with no square root; first row, last row, neighbours, both flag values): the count is exactly the number planted, every other row still decompresses."""
    P, rnd = pyref.P, random.Random(seed)
    few, _ = structured_bases(orc, pyref, n // 2, "few", seed)
    tab = np.concatenate([few, orc.gen_bases_arith(rnd.randrange(1, pyref.R), rnd.randrange(1, pyref.R), n - n // 2)])
    for i in (0, 1, n // 2, n - 1):
        tab[i] = 0
    pts = orc.g1_affine_to_ints(tab)
    par = [p[1] & 1 for p in pts if p is not None]
    assert min(par.count(0), par.count(1)) >= len(par) // 4, "both parities in bulk"
    raw = b"".join(_encode(p, sign_bit) for p in pts)
    if sign_bit == 255:
        assert raw == b"".join(point_to_bytes(p) for p in pts)
    assert raw == b"".join(point_to_bytes(p, sign_bit) for p in pts)
    out, back = be.alloc(n * 64), be.alloc(n * 32)
    try:
        rc, bad = decompress_counting(be, _words(raw), sign_bit, out)
        assert (rc, bad) == (0, 0)
        assert (out.download((n, 8)) == tab).all()
        be.g1_compress_dev(out, n, sign_bit, back)
        assert back.download((n, 4)).tobytes() == raw
        d = be.to_device(tab)                                          # compress from the table itself (not from decompress's output)
        be.g1_compress_dev(d, n, sign_bit, back)
        d.free()
        assert back.download((n, 4)).tobytes() == raw
        # bad words
        nonres = []
        while len(nonres) < 6:
            x = rnd.randrange(P)
            if pow((x * x * x + 3) % P, (P - 1) // 2, P) == P - 1:
                nonres.append(x)
        flag = 1 << sign_bit                                           # the parity flag's bit in the 256-bit word
        bad_x = [P, P + 1, (1 << 254) - 1, P | flag, (P + 1) | flag] + nonres[:3] + [x | flag for x in nonres[3:]]
        rows = [0, 1, 2, n // 2, n // 2 + 1, n - 1] + rnd.sample(range(3, n // 2), len(bad_x) - 6)
        assert len(set(rows)) == len(bad_x)
        words = _words(raw)
        want = tab.copy()
        for r, x in zip(rows, bad_x):
            words[r] = _words(x.to_bytes(32, "little"))[0]
            want[r] = 0
        rc, bad = decompress_counting(be, words, sign_bit, out)
        assert rc != 0 and bad == len(bad_x), (rc, bad, len(bad_x))
        assert (out.download((n, 8)) == want).all()
        b = be.to_device(words)
        try:
            be.g1_decompress_dev(b, n, sign_bit, out)
            raise AssertionError("the wrapper accepted bad encodings")
        except z.ZkError as e:
            assert "%d encodings" % len(bad_x) in str(e), str(e)
        finally:
            b.free()
        rc, bad = decompress_counting(be, _words(raw), sign_bit, out)  # the count starts from zero again on the next call
        assert (rc, bad) == (0, 0)
    finally:
        out.free()
        back.free()
