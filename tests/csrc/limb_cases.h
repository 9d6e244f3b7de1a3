// TEST-ONLY: the per-element cases of the two limb harnesses, written once.  host_harness.hip loops over them on the CPU (the `#else` branches of field_mac.inc /
// field29_mac.inc); device_harness.hip instantiates one kernel per (field, op) and runs the very same functions on the GPU (the inline-assembly branches).  The op is a
// template parameter so that each case is compiled as it is when inlined in a product kernel; LC_DISPATCH turns the harnesses' run-time op number into that parameter.
#pragma once
#include "../../zk-dcap-verifier_amd/csrc/ec.cuh"

namespace zk {

// ---- field29.cuh on raw limbs.  Ops 0 .. 10; every other number runs op 9 (one()) --------------------------------------------------------------------------------
#define LC_F29_RAW_OPS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(10)
constexpr int LC_F29_RAW_DEFAULT = 9;
template <class F29, int OP>
ZK_HD u261 lc_f29_raw(const u261& a, const u261& b, const u261& c, const u261& d) {
    if constexpr (OP == 0) return F29::mul(a, b);
    else if constexpr (OP == 1) return F29::sqr(a);
    else if constexpr (OP == 2) return F29::mul2(a, b, c, d);
    else if constexpr (OP == 3) return F29::carry(a);
    else if constexpr (OP == 4) return F29::template sub_bias<8, 30>(a, b);
    else if constexpr (OP == 5) return F29::template sub_bias<3, 30>(a, b);
    else if constexpr (OP == 6) return F29::template sub_bias<5, 31>(a, b);
    else if constexpr (OP == 7) return F29::template neg_bias<3, 30>(a);
    else if constexpr (OP == 8) return F29::add(a, F29::dbl(b));
    else if constexpr (OP == 10) return F29::mul_shoup(a, b, c);                                          // a * w with w's precomputed quotient
    else return F29::one();
}

// ---- field29.cuh through the two Montgomery forms.  Ops 0 .. 5; every other number runs op 4 (the square) ----------------------------------------------------------
#define LC_F29_FORMS_OPS(X) X(0) X(1) X(2) X(3) X(5)
constexpr int LC_F29_FORMS_DEFAULT = 4;
template <class F29, int OP>
ZK_HD void lc_f29_forms(const u256& a, const u256& b, u256& o, u261& o9) {
    if constexpr (OP == 0) { o9 = F29::enter(a); o = F29::leave(o9); }                                    // there and back
    else if constexpr (OP == 1) { o9 = F29::mul(F29::enter(a), F29::enter(b)); o = F29::leave(o9); }      // a * b in the library's form
    else if constexpr (OP == 2) { o9 = F29::mul(F29::template from32<5>(a), F29::enter(b)); o = F29::leave(o9); }   // the shifted conversion as one operand
    else if constexpr (OP == 3) { o9 = F29::template from32<0>(a); o = F29::to32(o9); }                   // limb conversion alone
    else if constexpr (OP == 5) { o9 = F29::shoup_quotient(a); o = a; }                                   // floor(a 2^261 / p)
    else { o9 = F29::sqr(F29::enter(a)); o = F29::leave(o9); }
}

// ---- the redundant-range forms (field.cuh): inputs may be anywhere in the range each function documents.  Ops 0 .. 15; every other number runs op 11 ---------------
#define LC_FQ_LAZY_OPS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(12) X(13) X(14) X(15)
constexpr int LC_FQ_LAZY_DEFAULT = 11;
template <int OP>
ZK_HD u256 lc_fq_lazy(const u256& a, const u256& b, const u256& c, const u256& d) {
    if constexpr (OP == 0) return Fq::mul_lazy(a, b);
    else if constexpr (OP == 1) return Fq::sqr_lazy(a);
    else if constexpr (OP == 2) return Fq::sub2(a, b);
    else if constexpr (OP == 3) return Fq::dbl2(a);
    else if constexpr (OP == 4) return Fq::neg2(a);
    else if constexpr (OP == 5) return Fq::mul2_add_2p(a, b, c, d);
    else if constexpr (OP == 6) return Fq::red2p(a);
    else if constexpr (OP == 7) return Fq::add_lazy(a, b);
    else if constexpr (OP == 8) return Fq::sub_lazy(a, b);
    else if constexpr (OP == 9) return Fq::normalize(a);
    else if constexpr (OP == 10) { u256 o = Fq::zero(); o.v[0] = Fq::is_zero_mod(a) ? 1 : 0; return o; }
    else if constexpr (OP == 14) return Fq::shoup_quotient(a);                // floor(w 2^256 / p) from w's library form
    else if constexpr (OP == 15) return Fr::shoup_quotient(a);
    else if constexpr (OP == 12) return Fq::mul_shoup_lazy(a, b, c);          // a * w with wq = floor(w 2^256 / p): no Montgomery factor, [0, 2p)
    else if constexpr (OP == 13) return Fr::mul_shoup_lazy(a, b, c);
    else return Fq::mul(a, b);                                                // 11: the full product on inputs up to 4p
}

// ---- the canonical ops (hh_fr_* / hh_fq_*): one number each, operands the op does not take are ignored ------------------------------------------------------------
enum { LC_MUL = 0, LC_ADD = 1, LC_SUB = 2, LC_NEG = 3, LC_INV = 4, LC_FROM_MONT = 5, LC_MUL2_SUB = 6 };
template <class F, int OP>
ZK_HD u256 lc_field(const u256& a, const u256& b, const u256& c, const u256& d) {
    if constexpr (OP == LC_MUL) return F::mul(a, b);
    else if constexpr (OP == LC_ADD) return F::add(a, b);
    else if constexpr (OP == LC_SUB) return F::sub(a, b);
    else if constexpr (OP == LC_NEG) return F::neg(a);
    else if constexpr (OP == LC_INV) return F::inv(a);
    else if constexpr (OP == LC_FROM_MONT) return F::from_mont(a);
    else return F::mul2_sub(a, b, c, d);
}

// run-time op number -> template parameter.  The user defines LC_DISPATCH_CALL_(N), a statement that takes the op as a literal, around each use.
#define LC_DISPATCH_CASE_(N) case N: LC_DISPATCH_CALL_(N); break;
#define LC_DISPATCH(op, OPS, DEFAULT)       \
    switch (op) {                           \
        OPS(LC_DISPATCH_CASE_)              \
        default: LC_DISPATCH_CALL_(DEFAULT); break; \
    }

// ---- the full additions and the doubling, one element ---------------------------------------------------------------------------------------------------------------
enum { LC_XYZZ_ADD = 0, LC_XYZZ_ADD_LAZY = 1, LC_XYZZ_DBL = 2 };
template <int OP>
ZK_HD XYZZ lc_xyzz_pair(const XYZZ& a, const XYZZ& b) {
    if constexpr (OP == LC_XYZZ_ADD) { XYZZ t = a; xyzz_add(t, b); return t; }
    else if constexpr (OP == LC_XYZZ_ADD_LAZY) { XYZZ t = a; xyzz_add_lazy(t, b); xyzz_add_lazy(t, b); xyzz_normalize(t); return t; }   // a + b + b: the second addition meets lazy coordinates
    else return xyzz_dbl(a);
}

// ---- chains ---------------------------------------------------------------------------------------------------------------------------------------------------------
// acc (XYZZ) += sign * p for a list of affine points; acc starts at identity
ZK_HD XYZZ lc_xyzz_sum(const Affine* pts, const uint8_t* neg, size_t n) {
    XYZZ acc = xyzz_identity();
    for (size_t i = 0; i < n; i++) xyzz_madd_signed(acc, pts[i], neg[i] != 0);
    return acc;
}
ZK_HD XYZZ lc_xyzz_sum_lazy(const Affine* pts, const uint8_t* neg, size_t n) {
    XYZZ acc = xyzz_identity();
    for (size_t i = 0; i < n; i++) xyzz_madd_signed_lazy(acc, pts[i], neg[i] != 0);
    xyzz_normalize(acc);
    return acc;
}
// the bucket chain on 29-bit limbs, complete form (rare cases through the canonical formulas), result in canonical coordinates
ZK_HD XYZZ lc_xyzz29_sum(const Affine* pts, const uint8_t* neg, size_t n, uint32_t* n_rare) {
    XYZZ29 acc = xyzz29_identity();
    uint32_t rare = 0;
    for (size_t i = 0; i < n; i++) {
        if (affine_is_identity(pts[i])) continue;
        const u256 y = neg[i] ? Fq::neg(pts[i].y) : pts[i].y;
        if (acc.ident || !xyzz29_madd_fast(acc, pts[i].x, y)) { rare++; xyzz29_madd(acc, pts[i].x, y); }
    }
    *n_rare = rare;
    return xyzz29_leave(acc);
}
ZK_HD bool lc_same_words(const uint32_t* a, const uint32_t* b, int words) {
    uint32_t o = 0;
    for (int i = 0; i < words; i++) o |= a[i] ^ b[i];
    return o == 0;
}
ZK_HD bool lc_same_xyzz29(const XYZZ29& a, const XYZZ29& b) {
    return lc_same_words(a.x.l, b.x.l, 9) && lc_same_words(a.y.l, b.y.l, 9) && lc_same_words(a.zz.l, b.zz.l, 9) && lc_same_words(a.zzz.l, b.zzz.l, 9) && a.ident == b.ident;
}
ZK_HD bool lc_same_xyzz(const XYZZ& a, const XYZZ& b) {
    return lc_same_words(a.x.v, b.x.v, 8) && lc_same_words(a.y.v, b.y.v, 8) && lc_same_words(a.zz.v, b.zz.v, 8) && lc_same_words(a.zzz.v, b.zzz.v, 8);
}
// the one-limb filter of xyzz29_madd_fast.  One chain from `start` through the fast step itself, adding steps[i % n_steps] (points whose x differs from the
// accumulator's) `len` times.  Before step i the accumulator is the point prefix[i] (the caller's, from the oracle): the fast step is offered (prefix[i].x, +y) and
// (prefix[i].x, -y) — the same x, a doubling and a cancellation — and must refuse both and leave the accumulator as it was.  prefix == null: no probes.
// counts[0] = collisions the filter let through, [1] = refusals that touched the accumulator, [2] = false alarms (refusals on the chain's own distinct-x additions, which
// then take the complete step), [3] = steps after which the chain, left to canonical coordinates, differs from the same chain through xyzz_madd (check != 0).
ZK_HD XYZZ lc_xyzz29_filter_probe(const Affine* start, const Affine* steps, size_t n_steps, const Affine* prefix, size_t len, int check, uint64_t* counts) {
    XYZZ29 acc = xyzz29_identity();
    xyzz29_madd(acc, start->x, start->y);
    XYZZ ref = xyzz_from_affine(*start);
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (size_t i = 0; i < len; i++) {
        if (prefix) {
            for (int sign = 0; sign < 2; sign++) {
                XYZZ29 t = acc;
                if (xyzz29_madd_fast(t, prefix[i].x, sign ? Fq::neg(prefix[i].y) : prefix[i].y)) c0++;
                else if (!lc_same_xyzz29(t, acc)) c1++;
            }
        }
        const Affine& s = steps[i % n_steps];
        if (!xyzz29_madd_fast(acc, s.x, s.y)) { c2++; xyzz29_madd(acc, s.x, s.y); }
        if (check) {
            xyzz_madd(ref, s.x, s.y);
            const XYZZ l = xyzz29_leave(acc);
            if (!lc_same_xyzz(l, ref)) c3++;
        }
    }
    counts[0] = c0; counts[1] = c1; counts[2] = c2; counts[3] = c3;
    return xyzz29_leave(acc);
}

}  // namespace zk
