// TEST-ONLY: the device twin of host_harness.hip.  One dh_* entry point per hh_* one, same host pointers; each call validates its arguments, allocates, copies in,
// launches, synchronises, copies out, frees, and returns the first non-zero HIP status (0 = the outputs are valid).  The kernels run the per-element functions of
// limb_cases.h — the very code host_harness.hip loops over — so on the GPU the inline-assembly branches of field_mac.inc / field29_mac.inc meet the same rows as the
// plain C++ ones do on the CPU (tests/test_limbs_device.py).  The product library never links this file.
//   * element-wise ops: one thread per row, one kernel instantiation per (field, op) — no run-time switch inside a kernel; `block` (a multiple of 64, at most 256) is
//     the caller's.
//   * chains: `chains` chains in one launch, one chain per thread, the points of all chains concatenated and off[c] .. off[c + 1] those of chain c: the lanes of a
//     wave run chains of different lengths and take the rare / complete step at different iterations, as the MSM's accumulate loop does.
// Every index a kernel forms is below a bound checked here on the host before the launch.
#include <vector>
#include "limb_cases.h"
using namespace zk;

namespace {

constexpr size_t DH_MAX_ROWS = size_t(1) << 22;        // rows / points / chains of one call: far above what the tests send, far below any 32-bit index

bool block_ok(int block) { return block >= 64 && block <= 256 && block % 64 == 0; }
unsigned grid_for(size_t n, int block) { return (unsigned)((n + (size_t)block - 1) / (size_t)block); }

// the device buffers of one call: the first failing HIP call is kept and everything after it is skipped; the destructor frees whatever was allocated
struct Call {
    hipError_t st = hipSuccess;
    std::vector<void*> bufs;
    template <class T>
    T* in(const T* host, size_t count) {               // device copy of host[0 .. count)
        T* d = out<T>(count);
        if (st == hipSuccess && count) st = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    T* out(size_t count) {                             // zeroed device buffer of count elements (at least one, so that the pointer is never null)
        void* d = nullptr;
        if (st != hipSuccess) return nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        st = hipMalloc(&d, bytes);
        if (st != hipSuccess) return nullptr;
        bufs.push_back(d);
        st = hipMemset(d, 0, bytes);
        return (T*)d;
    }
    void finish_launch() {                             // after the <<< >>>: launch error, then the kernel's own
        if (st == hipSuccess) st = hipGetLastError();
        if (st == hipSuccess) st = hipDeviceSynchronize();
    }
    template <class T>
    void back(T* host, const T* dev, size_t count) {
        if (st == hipSuccess && count) st = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    int done() {
        for (void* d : bufs) {
            const hipError_t e = hipFree(d);
            if (st == hipSuccess) st = e;
        }
        bufs.clear();
        return (int)st;
    }
    ~Call() { done(); }
};

// ---- element-wise kernels: thread i handles row i -----------------------------------------------------------------------------------------------------------------
template <class F29, int OP>
__global__ __launch_bounds__(256) void k_f29_raw(const u261* a, const u261* b, const u261* c, const u261* d, u261* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = lc_f29_raw<F29, OP>(a[i], b[i], c[i], d[i]);
}
template <class F29, int OP>
__global__ __launch_bounds__(256) void k_f29_forms(const u256* a, const u256* b, u256* o, u261* o9, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u256 r;
    u261 r9;
    lc_f29_forms<F29, OP>(a[i], b[i], r, r9);
    o[i] = r;
    o9[i] = r9;
}
template <int OP>
__global__ __launch_bounds__(256) void k_fq_lazy(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = lc_fq_lazy<OP>(a[i], b[i], c[i], d[i]);
}
template <class F, int OP>
__global__ __launch_bounds__(256) void k_field(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = lc_field<F, OP>(a[i], b[i], c[i], d[i]);
}
template <int OP>
__global__ __launch_bounds__(256) void k_xyzz_pair(const XYZZ* a, const XYZZ* b, XYZZ* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    o[i] = lc_xyzz_pair<OP>(a[i], b[i]);
}
// ---- chain kernels: thread c handles chain c ------------------------------------------------------------------------------------------------------------------------
enum { DH_SUM = 0, DH_SUM_LAZY = 1, DH_SUM29 = 2 };
template <int KIND>
__global__ __launch_bounds__(256) void k_chain(const Affine* pts, const uint8_t* neg, const uint64_t* off, size_t chains, XYZZ* out, uint32_t* n_rare) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chains) return;
    const size_t lo = off[c], n = off[c + 1] - lo;
    if constexpr (KIND == DH_SUM) out[c] = lc_xyzz_sum(pts + lo, neg + lo, n);
    else if constexpr (KIND == DH_SUM_LAZY) out[c] = lc_xyzz_sum_lazy(pts + lo, neg + lo, n);
    else {
        uint32_t rare;
        out[c] = lc_xyzz29_sum(pts + lo, neg + lo, n, &rare);
        n_rare[c] = rare;
    }
}
__global__ __launch_bounds__(256) void k_filter_probe(const Affine* start, const Affine* steps, size_t n_steps, const Affine* prefix, const uint64_t* off, size_t chains, int check,
                                                      uint64_t* counts, XYZZ* out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chains) return;
    uint64_t cnt[4];
    out[c] = lc_xyzz29_filter_probe(start + c, steps + c * n_steps, n_steps, prefix ? prefix + off[c] : nullptr, off[c + 1] - off[c], check, cnt);
    for (int j = 0; j < 4; j++) counts[4 * c + j] = cnt[j];
}

template <class F29>
int run_f29_raw(int op, const u261* a, const u261* b, const u261* c, const u261* d, u261* o, size_t n, int block) {
    Call k;
    const u261 *da = k.in(a, n), *db = k.in(b, n), *dc = k.in(c, n), *dd = k.in(d, n);
    u261* dout = k.out<u261>(n);
    if (k.st == hipSuccess) {
#define LC_DISPATCH_CALL_(N) k_f29_raw<F29, N><<<grid_for(n, block), block>>>(da, db, dc, dd, dout, n)
        LC_DISPATCH(op, LC_F29_RAW_OPS, LC_F29_RAW_DEFAULT)
#undef LC_DISPATCH_CALL_
        k.finish_launch();
    }
    k.back(o, dout, n);
    return k.done();
}
template <class F29>
int run_f29_forms(int op, const u256* a, const u256* b, u256* o, u261* o9, size_t n, int block) {
    Call k;
    const u256 *da = k.in(a, n), *db = k.in(b, n);
    u256* dout = k.out<u256>(n);
    u261* dout9 = k.out<u261>(n);
    if (k.st == hipSuccess) {
#define LC_DISPATCH_CALL_(N) k_f29_forms<F29, N><<<grid_for(n, block), block>>>(da, db, dout, dout9, n)
        LC_DISPATCH(op, LC_F29_FORMS_OPS, LC_F29_FORMS_DEFAULT)
#undef LC_DISPATCH_CALL_
        k.finish_launch();
    }
    k.back(o, dout, n);
    k.back(o9, dout9, n);
    return k.done();
}
// operands an op does not take arrive as null: the kernel is handed `a` in their place (it ignores them)
template <class F, int OP>
int run_field(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n, int block) {
    if (!a || !o || n > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    Call k;
    const u256* da = k.in(a, n);
    const u256 *db = b ? k.in(b, n) : da, *dc = c ? k.in(c, n) : da, *dd = d ? k.in(d, n) : da;
    u256* dout = k.out<u256>(n);
    if (k.st == hipSuccess) {
        k_field<F, OP><<<grid_for(n, block), block>>>(da, db, dc, dd, dout, n);
        k.finish_launch();
    }
    k.back(o, dout, n);
    return k.done();
}
template <int OP>
int run_xyzz_pair(const XYZZ* a, const XYZZ* b, XYZZ* o, size_t n, int block) {
    if (!a || !b || !o || n > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    Call k;
    const XYZZ *da = k.in(a, n), *db = k.in(b, n);
    XYZZ* dout = k.out<XYZZ>(n);
    if (k.st == hipSuccess) {
        k_xyzz_pair<OP><<<grid_for(n, block), block>>>(da, db, dout, n);
        k.finish_launch();
    }
    k.back(o, dout, n);
    return k.done();
}
// off[0] = 0 <= off[1] <= ... <= off[chains] = n_pts: every chain's slice lies inside the concatenated buffers
bool offsets_ok(const uint64_t* off, size_t chains, size_t n_pts) {
    if (!off || off[0] != 0 || off[chains] != n_pts) return false;
    for (size_t c = 0; c < chains; c++)
        if (off[c] > off[c + 1]) return false;
    return true;
}
template <int KIND>
int run_chain(const Affine* pts, const uint8_t* neg, const uint64_t* off, size_t chains, XYZZ* out, uint32_t* n_rare, int block) {
    if (!pts || !neg || !out || (KIND == DH_SUM29 && !n_rare) || chains > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (chains == 0) return (int)hipSuccess;
    if (!off || off[chains] > DH_MAX_ROWS || !offsets_ok(off, chains, (size_t)off[chains])) return (int)hipErrorInvalidValue;
    const size_t n_pts = (size_t)off[chains];
    Call k;
    const Affine* dp = k.in(pts, n_pts);
    const uint8_t* dn = k.in(neg, n_pts);
    const uint64_t* doff = k.in(off, chains + 1);
    XYZZ* dout = k.out<XYZZ>(chains);
    uint32_t* drare = k.out<uint32_t>(chains);
    if (k.st == hipSuccess) {
        k_chain<KIND><<<grid_for(chains, block), block>>>(dp, dn, doff, chains, dout, drare);
        k.finish_launch();
    }
    k.back(out, dout, chains);
    if (KIND == DH_SUM29) k.back(n_rare, drare, chains);
    return k.done();
}

}  // namespace

extern "C" {
int dh_fr_mul(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fr, LC_MUL>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fr_add(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fr, LC_ADD>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fr_sub(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fr, LC_SUB>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fr_neg(const u256* a, u256* o, size_t n, int block) { return run_field<Fr, LC_NEG>(a, nullptr, nullptr, nullptr, o, n, block); }
int dh_fr_inv(const u256* a, u256* o, size_t n, int block) { return run_field<Fr, LC_INV>(a, nullptr, nullptr, nullptr, o, n, block); }
int dh_fr_from_mont(const u256* a, u256* o, size_t n, int block) { return run_field<Fr, LC_FROM_MONT>(a, nullptr, nullptr, nullptr, o, n, block); }
int dh_fq_mul(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fq, LC_MUL>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fq_add(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fq, LC_ADD>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fq_sub(const u256* a, const u256* b, u256* o, size_t n, int block) { return b ? run_field<Fq, LC_SUB>(a, b, nullptr, nullptr, o, n, block) : (int)hipErrorInvalidValue; }
int dh_fq_mul2_sub(const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n, int block) {
    return b && c && d ? run_field<Fq, LC_MUL2_SUB>(a, b, c, d, o, n, block) : (int)hipErrorInvalidValue;
}
int dh_fq_lazy(int op, const u256* a, const u256* b, const u256* c, const u256* d, u256* o, size_t n, int block) {
    if (!a || !b || !c || !d || !o || n > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    Call k;
    const u256 *da = k.in(a, n), *db = k.in(b, n), *dc = k.in(c, n), *dd = k.in(d, n);
    u256* dout = k.out<u256>(n);
    if (k.st == hipSuccess) {
#define LC_DISPATCH_CALL_(N) k_fq_lazy<N><<<grid_for(n, block), block>>>(da, db, dc, dd, dout, n)
        LC_DISPATCH(op, LC_FQ_LAZY_OPS, LC_FQ_LAZY_DEFAULT)
#undef LC_DISPATCH_CALL_
        k.finish_launch();
    }
    k.back(o, dout, n);
    return k.done();
}
int dh_f29_raw(int field, int op, const u261* a, const u261* b, const u261* c, const u261* d, u261* o, size_t n, int block) {
    if (!a || !b || !c || !d || !o || n > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    return field == 0 ? run_f29_raw<Fq29>(op, a, b, c, d, o, n, block) : run_f29_raw<Fr29>(op, a, b, c, d, o, n, block);
}
int dh_f29_forms(int field, int op, const u256* a, const u256* b, u256* o, u261* o9, size_t n, int block) {
    if (!a || !b || !o || !o9 || n > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    return field == 0 ? run_f29_forms<Fq29>(op, a, b, o, o9, n, block) : run_f29_forms<Fr29>(op, a, b, o, o9, n, block);
}
// the single-element hh_xyzz_add / _add_lazy / _dbl, on n rows
int dh_xyzz_add(const XYZZ* a, const XYZZ* b, XYZZ* out, size_t n, int block) { return run_xyzz_pair<LC_XYZZ_ADD>(a, b, out, n, block); }
int dh_xyzz_add_lazy(const XYZZ* a, const XYZZ* b, XYZZ* out, size_t n, int block) { return run_xyzz_pair<LC_XYZZ_ADD_LAZY>(a, b, out, n, block); }
int dh_xyzz_dbl(const XYZZ* a, XYZZ* out, size_t n, int block) { return run_xyzz_pair<LC_XYZZ_DBL>(a, a, out, n, block); }
// the chains, batched: pts / neg hold off[chains] points, chain c is off[c] .. off[c + 1]; out[c] (and n_rare[c]) are chain c's
int dh_xyzz_sum(const Affine* pts, const uint8_t* neg, const uint64_t* off, size_t chains, XYZZ* out, int block) { return run_chain<DH_SUM>(pts, neg, off, chains, out, nullptr, block); }
int dh_xyzz_sum_lazy(const Affine* pts, const uint8_t* neg, const uint64_t* off, size_t chains, XYZZ* out, int block) {
    return run_chain<DH_SUM_LAZY>(pts, neg, off, chains, out, nullptr, block);
}
int dh_xyzz29_sum(const Affine* pts, const uint8_t* neg, const uint64_t* off, size_t chains, XYZZ* out, uint32_t* n_rare, int block) {
    return run_chain<DH_SUM29>(pts, neg, off, chains, out, n_rare, block);
}
// hh_xyzz29_filter_probe, batched: start[c], steps[c * n_steps .. + n_steps), chain c takes off[c + 1] - off[c] steps and (prefix != null) reads prefix[off[c] ..
// off[c + 1]); counts[4 c .. 4 c + 4) and out[c] are chain c's
int dh_xyzz29_filter_probe(const Affine* start, const Affine* steps, size_t n_steps, const Affine* prefix, const uint64_t* off, size_t chains, int check, uint64_t* counts,
                           XYZZ* out, int block) {
    if (!start || !steps || n_steps == 0 || n_steps > DH_MAX_ROWS || !counts || !out || chains > DH_MAX_ROWS || !block_ok(block)) return (int)hipErrorInvalidValue;
    if (chains == 0) return (int)hipSuccess;
    if (!off || off[chains] > DH_MAX_ROWS || chains * n_steps > DH_MAX_ROWS || !offsets_ok(off, chains, (size_t)off[chains])) return (int)hipErrorInvalidValue;
    const size_t n_prefix = (size_t)off[chains];
    Call k;
    const Affine* ds = k.in(start, chains);
    const Affine* dst = k.in(steps, chains * n_steps);
    const Affine* dp = prefix ? k.in(prefix, n_prefix) : nullptr;
    const uint64_t* doff = k.in(off, chains + 1);
    uint64_t* dcnt = k.out<uint64_t>(4 * chains);
    XYZZ* dout = k.out<XYZZ>(chains);
    if (k.st == hipSuccess) {
        k_filter_probe<<<grid_for(chains, block), block>>>(ds, dst, n_steps, dp, doff, chains, check, dcnt, dout);
        k.finish_launch();
    }
    k.back(counts, dcnt, 4 * chains);
    k.back(out, dout, chains);
    return k.done();
}
}
