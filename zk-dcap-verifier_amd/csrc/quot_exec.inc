// What a quotient executor does to one row, stated once: the interpreter kernels of quotient.hip include this text and so do the kernels quotient_jit.hip generates
// (through build/jit_headers.inc, after field.cuh and quot_args.inc, inside namespace zk — so nothing here may need a system header).

constexpr uint32_t QUOT_NREG = 1;   // first slot of the allocator is a register, the rest LDS (3 -> 1: 128 -> 116 VGPRs, 9.74 -> 9.18 ms at k = 19: profiles/r02)

// The micro-ops (M_ADD .. M_FOLD2 of quotient.h), operands A, B, C and the accumulator.  Every value of a row (slots, accumulator) lives in [0, 2p] (field.cuh, redundant
// ranges): products skip their final subtraction, sums and differences are corrected by 2p (same cost as by p), memory operands arrive canonical, and the row's result is
// normalised once at the end (quot_finish).  Function-like macros, so that an operand an op does not use is never evaluated: in the interpreter an operand is an LDS read or
// a waited-for load, in generated text an LDCOL or LDC.
#define QOP_ADD(A, B, C, ACC) Fr::red2p(Fr::add_lazy(A, B))
#define QOP_SUB(A, B, C, ACC) Fr::sub2(A, B)
#define QOP_MUL(A, B, C, ACC) Fr::mul_lazy(A, B)
#define QOP_SQR(A, B, C, ACC) Fr::sqr_lazy(A)
#define QOP_DBL(A, B, C, ACC) Fr::dbl2(A)
#define QOP_NEG(A, B, C, ACC) Fr::neg2(A)
#define QOP_MOV(A, B, C, ACC) A
#define QOP_MULADD(A, B, C, ACC) Fr::red2p(Fr::add_lazy(Fr::mul_lazy(A, B), C))
#define QOP_FOLD2(A, B, C, ACC) Fr::mul2_add_2p(ACC, C, A, B)
// the interpreters' dispatch: RES = micro-op OP of (A, B, C, ACC); an opcode outside the table moves A
#define QOP_SWITCH(OP, RES, A, B, C, ACC)                          \
    switch (OP) {                                                  \
        case M_ADD: RES = QOP_ADD(A, B, C, ACC); break;            \
        case M_SUB: RES = QOP_SUB(A, B, C, ACC); break;            \
        case M_MUL: RES = QOP_MUL(A, B, C, ACC); break;            \
        case M_SQR: RES = QOP_SQR(A, B, C, ACC); break;            \
        case M_DBL: RES = QOP_DBL(A, B, C, ACC); break;            \
        case M_NEG: RES = QOP_NEG(A, B, C, ACC); break;            \
        case M_MULADD: RES = QOP_MULADD(A, B, C, ACC); break;      \
        case M_FOLD2: RES = QOP_FOLD2(A, B, C, ACC); break;        \
        default: RES = QOP_MOV(A, B, C, ACC); break;               \
    }

// memory operands of a row, for a kernel that holds QuotArgs q, the row idx0 and mask = 2^size_log - 1
#define LDC(i) load_u256(q.consts, (i))
#define LDCOL(c, r) load_u256(q.cols[(c)], (idx0 + q.rot_off[(r)]) & mask)

// thread gid of a launch -> idx0, the row it reads the columns at, and oidx, where its value goes in q.out (QuotArgs: row_base, strided)
ZK_HD void quot_row(const QuotArgs& q, uint32_t gid, uint32_t& idx0, uint32_t& oidx) {
    idx0 = q.row_base + gid;
    oidx = gid;
    if (q.strided) {
        const uint32_t j = idx0 & ((1u << q.sub_log) - 1u), i = idx0 >> q.sub_log;
        idx0 = (i << q.stride_log) + j;
        oidx = (j << q.k_log) + i;
    }
}
// X at row idx0: extended_omega^(position of the row in the extended domain), from the two-level power table
ZK_HD u256 quot_xpow(const QuotArgs& q, uint32_t idx0) {
    const uint32_t xi = idx0 * q.xpow_mul + q.xpow_add;
    u256 x = load_u256(q.tw_lo, xi & ((1u << q.lo_bits) - 1u));
    const uint32_t h = xi >> q.lo_bits;
    if (h) x = Fr::mul(x, load_u256(q.tw_hi, h));
    return x;
}
// the row's value leaves the executor: accumulate mode folds it into what q.out holds (previous * y^E + this numerator), then it is normalised and stored
ZK_HD void quot_finish(const QuotArgs& q, uint32_t oidx, u256 acc) {
    if (q.accumulate) acc = QOP_MULADD(load_u256(q.out, oidx), load_u256(q.consts, q.acc_const), acc, acc);
    store_u256(q.out, oidx, Fr::normalize(acc));
}
// LDS slot ls of thread tid in a workgroup of T threads: slot-major, two 16-byte halves, lane-consecutive (conflict free)
ZK_HD u256 quot_slot_load(const uint4* smem, uint32_t ls, uint32_t T, uint32_t tid) {
    const uint4 l = smem[(2 * ls) * T + tid], h = smem[(2 * ls + 1) * T + tid];
    u256 o;
    o.v[0] = l.x; o.v[1] = l.y; o.v[2] = l.z; o.v[3] = l.w; o.v[4] = h.x; o.v[5] = h.y; o.v[6] = h.z; o.v[7] = h.w;
    return o;
}
ZK_HD void quot_slot_store(uint4* smem, uint32_t ls, uint32_t T, uint32_t tid, const u256& v) {
    smem[(2 * ls) * T + tid] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    smem[(2 * ls + 1) * T + tid] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}
