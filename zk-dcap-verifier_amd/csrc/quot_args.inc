// Launch arguments of the quotient executors (quotient.hip interpreter; the kernels quotient_jit.hip generates include this very text, so the two cannot drift).
struct QuotArgs {
    const uint4* code;
    uint32_t n_instr;
    const void* consts;
    const void* const* cols;
    const uint32_t* rot_off;   // row offsets (already scaled, non-negative, < size)
    uint32_t size_log;
    const void* tw_lo;
    const void* tw_hi;
    uint32_t lo_bits;
    int uses_xpow;
    uint32_t xpow_mul, xpow_add;   // X of row idx = extended_omega^(idx * xpow_mul + xpow_add): (1, 0) on the whole extended domain, (2^(ek-k), j) on coset j
    uint32_t strided, sub_log, stride_log, k_log;   // strided: thread t works on row ((t >> sub_log) << stride_log) + (t & (2^sub_log - 1)) of extended-layout columns
                                                    // and writes out[((t & (2^sub_log - 1)) << k_log) + (t >> sub_log)]: the first 2^sub_log cosets, coset-major
    uint32_t row_base;             // first row of this launch (a launch may cover a slice of the rows: out[i] = numerator of row row_base + i)
    void* out;
    void* state;                   // generated kernels only: the slots that are live between two kernels of a program, plane s at state + s * state_stride (32 bytes per row)
    unsigned long long state_stride;
    // accumulate mode (zk_quotient_run_acc_dev): out holds halo2's PreviousValue on entry and receives out * consts[acc_const] + numerator, consts[acc_const] = y^E
    // (E = the identities of the whole program).  The generated kernels then carry their running value in acc_state instead of out.
    uint32_t accumulate, acc_const;
    void* acc_state;
};
