// The quotient micro-program as the compiler (quotient.hip) leaves it and as its two executors read it: the interpreter kernel (quotient.hip) and the
// per-program straight-line kernels generated from the same micro-ops (quotient_jit.hip).
#pragma once
#include "ctx.h"

namespace zk {
// micro-ops, in opcode order (what each one computes: quot_exec.inc, QOP_<name>).  M_FOLD2: acc = acc * c + a * b with ONE Montgomery reduction (value = value * y + product)
#define QUOT_OPS(X) X(ADD) X(SUB) X(MUL) X(SQR) X(DBL) X(NEG) X(MOV) X(MULADD) X(FOLD2)
#define QUOT_OP_ENUM(name) M_##name,
enum { QUOT_OPS(QUOT_OP_ENUM) M_COUNT };
enum { K_SLOT = 0, K_CONST, K_COL, K_ACC, K_XPOW, K_NONE = 7 };

struct QuotProgram {
    uint32_t k = 0, ek = 0, n_fixed = 0, n_advice = 0, n_instance = 0, n_challenges = 0, blinding = 0, degree = 0;
    uint32_t n_perm_cols = 0, n_sets = 0, n_lookups = 0;
    std::vector<uint32_t> perm_cols;      // pairs (type, index)
    std::vector<uint4> code;
    std::vector<u256> graph_consts;       // constants that come with the program
    std::vector<int32_t> rotations;       // distinct rotations (rows)
    uint32_t n_slots = 0, n_cols = 0;
    // constant table layout (indices)
    uint32_t c_zero = 0, c_one = 0, c_chal = 0, c_beta = 0, c_gamma = 0, c_theta = 0, c_y = 0, c_delta = 0, c_ypow = 0, n_consts = 0;
    // Degree split (compile_program, `mode`): h's numerator is sum_i y^(N-1-i) id_i over the N identities halo2 folds with y; an identity of degree d (in the columns)
    // contributes a share of h(X) of degree below (d - 1) n, which (d - 1) cosets of the size-n domain determine.  part_hi / part_lo are the SAME program restricted to the
    // identities of degree above / up to SPLIT_LOW_DEGREE (a skipped identity leaves a power of y on the next fold: ypow_exps, constants of the run at c_ypow): the low part
    // is evaluated on SPLIT_LOW_DEGREE - 1 cosets only and joins h(X) through zk_cosets_to_pieces_dev.  Exact for every witness that satisfies the circuit (each identity
    // then vanishes on the domain on its own, so both shares are polynomials).
    std::vector<uint32_t> ypow_exps;      // y^e constants this program reads, e >= 2
    uint32_t folds_taken = 0, folds_skipped = 0;
    std::shared_ptr<QuotProgram> part_hi, part_lo;
    // column ids
    uint32_t col_fixed = 0, col_advice = 0, col_instance = 0, col_l0 = 0, col_llast = 0, col_lactive = 0, col_sigma = 0, col_z = 0,
             col_lk_z = 0, col_lk_a = 0, col_lk_s = 0;
    bool uses_xpow = false;
    void* d_code = nullptr;               // immutable after the load; the constants / column pointers / rotation offsets of a RUN live in the calling context's ws_quot,
    int device = 0;                       // so contexts of one device can share a program (zk_quotient_program_share) and run it concurrently
    std::shared_ptr<struct QuotJit> jit;  // quotient_jit.hip: the same micro-ops as straight-line kernels generated for THIS program (hiprtc, tune quot_jit), or null: the interpreter runs it
    ~QuotProgram() { if (d_code) { (void)hipSetDevice(device); (void)hipFree(d_code); } }
};

#include "quot_args.inc"

// quotient_jit.hip
struct QuotJitKernel {                        // one generated kernel = a run of consecutive micro-ops
    uint32_t first = 0, count = 0;            // micro-ops [first, first + count)
    std::vector<uint32_t> live_in, live_out;  // slots whose values cross the kernel's boundaries (carried in QuotArgs::state, one row-major plane per slot)
    bool reads_acc = false;                   // the accumulator arrives from the previous kernel (in `out`, redundant form)
    std::string name;                         // zkq<program tag>_<index>
};
std::string quot_jit_source(const QuotProgram& P, uint32_t group_ops, std::vector<QuotJitKernel>* kernels, uint32_t waves_per_eu = 0);
int quot_jit_build(zk_ctx* ctx, QuotProgram& P);                                   // tune quot_jit: compile P (and its parts) into kernels; failure leaves the interpreter in charge
bool quot_jit_ready(const QuotProgram& P);
uint32_t quot_jit_kernel_count(const QuotProgram& P);
int quot_jit_launch(zk_ctx* ctx, const QuotProgram& P, const QuotArgs& q, uint64_t rows, uint32_t threads);

// The launch shape of a program of n_slots slots (quotient.hip): slot 0 is a register, the others take 32 bytes of LDS per thread; a workgroup has min(tune quot_threads,
// 256, rows) threads, halved down to 64 while its slots exceed 32 KiB; a program fits when 64 threads' slots fit the 160 KiB of a CU.
struct QuotShape { uint32_t threads; size_t lds_bytes; };
uint32_t quot_lds_slots(uint32_t n_slots);
bool quot_slots_fit(uint32_t n_slots);
QuotShape quot_launch_shape(uint32_t n_slots, int quot_threads, uint64_t rows);

// Row-list mode of quotient_run (mockprover.hip, gate attribution): the program runs on rows[0 .. n) of its domain only, and instead of the value every thread
// writes one bit per fold of the accumulator: bit f of bits[i * words + f / 32] = the f-th folded term of row rows[i] is non-zero after full reduction.  For the
// program of quotient_program_load_gates the folds are exactly the gate polynomials, in cs.gates order.
struct QuotRowList { const uint32_t* rows; uint32_t n; uint32_t* bits; uint32_t words; };
// Which rows of which program a run evaluates; the defaults are the whole extended domain and every identity.
// coset = j >= 0: only coset j of the extended domain — the rows j, j + 2^(ek-k), ... — with columns given as that coset's n = 2^k values (zk_coeff_to_coset_batch_dev);
// rotations then step by one row.  The 2^(ek-k) cosets are independent, which is what lets a proof's quotient be split over GPUs: out receives the n
// numerator values of the coset.
// row_count > 0: only rows [row_lo, row_lo + row_count) of that domain (the columns are complete, so rotations need no halo), out[i] = row row_lo + i — the unit that
// lets more ranks than cosets share a quotient.
// part: 0 = every identity; 1 / 2 = the high / low part of a program that has a degree split (QuotProgram::part_hi / part_lo).  low_cosets > 0 (part 2, coset < 0): the
// columns are the whole extended domain but only the rows of its cosets 0 .. low_cosets-1 are evaluated — thread i of coset j reads row i * 2^(ek-k) + j — and out
// receives low_cosets x n values, coset-major (what zk_cosets_to_pieces_dev takes).
// accumulate: out holds halo2's PreviousValue and receives out * y^E + numerator (quot_args.inc).  rows: row-list mode — a program of extended_k = k that does not
// read X, on the whole domain.
struct QuotRoute {
    int coset = -1;
    uint64_t row_lo = 0, row_count = 0;
    int part = 0;
    uint32_t low_cosets = 0;
    bool accumulate = false;
    const QuotRowList* rows = nullptr;
};
int quotient_run(zk_ctx* ctx, uint64_t prog, const zk_quotient_args* a, const QuotRoute& route);
// The custom gates of an Evaluator blob (ZKQ1) alone, compiled at extended_k = k: value(row) = sum_i y^(E-1-i) gate_i(row), rotations mod 2^k (the permutation and
// the lookups of the blob are dropped).  *n_polys = E, the parts of the blob's final Horner(previous, gates, y); E = 0 loads nothing (*prog = 0).
int quotient_program_load_gates(zk_ctx* ctx, const void* blob, size_t len, uint64_t* prog, uint32_t* n_polys);
}  // namespace zk
