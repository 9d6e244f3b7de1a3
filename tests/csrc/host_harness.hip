// TEST-ONLY: runs the product's __host__ __device__ field / curve routines on the CPU so the
// limb logic can be checked against the oracle without a GPU (tests/test_host_logic.py, tests/test_field29.py).
// It is not a CPU fallback: the product library never links this file.
// The cases themselves live in limb_cases.h; this file only loops over them.  Its twin device_harness.hip (libdevharness.so, dh_* for every hh_* here) runs the same
// functions on the GPU, where the inline-assembly branches of field_mac.inc / field29_mac.inc are compiled instead of the plain C++ ones (tests/test_limbs_device.py).
#include "limb_cases.h"
using namespace zk;
template <class F29>
static void f29_raw(int op, const u261* a, const u261* b, const u261* c, const u261* d, u261* o, size_t n) {
#define LC_DISPATCH_CALL_(N) o[i] = lc_f29_raw<F29, N>(a[i], b[i], c[i], d[i])
    for (size_t i = 0; i < n; i++) LC_DISPATCH(op, LC_F29_RAW_OPS, LC_F29_RAW_DEFAULT)
#undef LC_DISPATCH_CALL_
}
template <class F29>
static void f29_forms(int op, const u256* a, const u256* b, u256* o, u261* o9, size_t n) {
#define LC_DISPATCH_CALL_(N) lc_f29_forms<F29, N>(a[i], b[i], o[i], o9[i])
    for (size_t i = 0; i < n; i++) LC_DISPATCH(op, LC_F29_FORMS_OPS, LC_F29_FORMS_DEFAULT)
#undef LC_DISPATCH_CALL_
}
template <class F, int OP>
static void field_op(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n) {
    for (size_t i = 0; i < n; i++) o[i] = lc_field<F, OP>(a[i], b ? b[i] : a[i], c ? c[i] : a[i], d ? d[i] : a[i]);
}
extern "C" {
void hh_fr_mul(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fr, LC_MUL>(a, b, nullptr, nullptr, o, n); }
void hh_fr_add(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fr, LC_ADD>(a, b, nullptr, nullptr, o, n); }
void hh_fr_sub(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fr, LC_SUB>(a, b, nullptr, nullptr, o, n); }
void hh_fr_neg(const u256* a, u256* o, size_t n) { field_op<Fr, LC_NEG>(a, nullptr, nullptr, nullptr, o, n); }
void hh_fr_inv(const u256* a, u256* o, size_t n) { field_op<Fr, LC_INV>(a, nullptr, nullptr, nullptr, o, n); }
void hh_fr_from_mont(const u256* a, u256* o, size_t n) { field_op<Fr, LC_FROM_MONT>(a, nullptr, nullptr, nullptr, o, n); }
void hh_fq_mul(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fq, LC_MUL>(a, b, nullptr, nullptr, o, n); }
void hh_fq_mul2_sub(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n) { field_op<Fq, LC_MUL2_SUB>(a, b, c, d, o, n); }
void hh_fq_add(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fq, LC_ADD>(a, b, nullptr, nullptr, o, n); }
void hh_fq_sub(const u256* a, const u256* b, u256* o, size_t n) { field_op<Fq, LC_SUB>(a, b, nullptr, nullptr, o, n); }
void hh_xyzz_sum(const Affine* pts, const uint8_t* neg, size_t n, XYZZ* out) { *out = lc_xyzz_sum(pts, neg, n); }
void hh_fq_lazy(int op, const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n) {
#define LC_DISPATCH_CALL_(N) o[i] = lc_fq_lazy<N>(a[i], b[i], c[i], d[i])
    for (size_t i = 0; i < n; i++) LC_DISPATCH(op, LC_FQ_LAZY_OPS, LC_FQ_LAZY_DEFAULT)
#undef LC_DISPATCH_CALL_
}
void hh_xyzz_sum_lazy(const Affine* pts, const uint8_t* neg, size_t n, XYZZ* out) { *out = lc_xyzz_sum_lazy(pts, neg, n); }
void hh_xyzz_add_lazy(const XYZZ* a, const XYZZ* b, XYZZ* out) { *out = lc_xyzz_pair<LC_XYZZ_ADD_LAZY>(*a, *b); }
void hh_xyzz_add(const XYZZ* a, const XYZZ* b, XYZZ* out) { *out = lc_xyzz_pair<LC_XYZZ_ADD>(*a, *b); }
void hh_xyzz_dbl(const XYZZ* a, XYZZ* out) { *out = lc_xyzz_pair<LC_XYZZ_DBL>(*a, *a); }

// ---- field29.cuh: the carry-free 29-bit-limb arithmetic, on raw limbs (the Python model of tests/limb_cases.py recomputes every column sum exactly and checks it fits
// 64 bits, so an overflow here would show as a difference) and through the two Montgomery forms
void hh_f29_raw(int field, int op, const u261* a, const u261* b, const u261* c, const u261* d, u261* o, size_t n) {
    if (field == 0) f29_raw<Fq29>(op, a, b, c, d, o, n); else f29_raw<Fr29>(op, a, b, c, d, o, n);
}
void hh_f29_forms(int field, int op, const u256* a, const u256* b, u256* o, u261* o9, size_t n) {
    if (field == 0) f29_forms<Fq29>(op, a, b, o, o9, n); else f29_forms<Fr29>(op, a, b, o, o9, n);
}
void hh_xyzz29_sum(const Affine* pts, const uint8_t* neg, size_t n, XYZZ* out, uint32_t* n_rare) { *out = lc_xyzz29_sum(pts, neg, n, n_rare); }
// lc_xyzz29_filter_probe (limb_cases.h) describes the probe and its four counts
void hh_xyzz29_filter_probe(const Affine* start, const Affine* steps, size_t n_steps, const Affine* prefix, size_t len, int check, uint64_t* counts, XYZZ* out) {
    *out = lc_xyzz29_filter_probe(start, steps, n_steps, prefix, len, check, counts);
}
}
