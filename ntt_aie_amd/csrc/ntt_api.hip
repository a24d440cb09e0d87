// ntt_api.hip -- C-ABI of libntt_hip.so (include/ntt_hip.h): plan, validation,
// twiddle preparation and the launchers behind the sequences of sequence.h.  Host side of what the reference
// does in src/test.cpp:62-190 (buffers, table, launch) minus XRT.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ntt_hip.h"
#include "guard.h"
#include "kernels.h"
#include "negacyclic_map.h"
#include "plan.h"
#include "sequence.h"

using namespace ntt::host;

namespace {

struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void) hipSetDevice(prev);
    }
};

// ROCTX ranges around every transform and every HBM pass when NTT_ROCTX=1 (rocprofv3 --marker-trace):
// the role of the reference's trace_event0() / trace_event1() brackets (src/aie_core.cc:129-131,
// src/aie2.py:182,312).  The ROCTX library is looked up at run time: no link-time profiler dependency.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char *e = getenv("NTT_ROCTX");
        if (!e || atoi(e) == 0) return;
        // rocprofv3 listens to the rocprofiler-sdk ROCTX; libroctx64 is the older roctracer one (rocprof v1/v2)
        void *h = nullptr;
        for (const char *name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) return;
        push = (int (*)(const char *)) dlsym(h, "roctxRangePushA");
        pop = (int (*)()) dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx &roctx() {
    static const Roctx r;
    return r;
}
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx().push != nullptr) {
        if (on) roctx().push(name);
    }
    RoctxRange(const char *what, int contig, int s0, int log_m) : on(roctx().push != nullptr) {
        if (!on) return;
        char buf[96];
        snprintf(buf, sizeof(buf), "%s %s stages %d-%d", what, contig ? "contig" : "column", s0, s0 + log_m - 1);
        roctx().push(buf);
    }
    ~RoctxRange() {
        if (on) roctx().pop();
    }
};

}  // namespace

// what the sequences read of a plan is its ntt::PlanFacts base (sequence.h); the rest is the C-ABI's own
struct ntt_plan : ntt::PlanFacts {
    int device = 0;
    bool has_table = false, has_inv = false;
    int fused = 0;           // experiment build only (NTT_FUSED=1): N = 2^16 Goldilocks forward through the XCD-local fused launch
    void *d_fused_ctl = nullptr;  // counters of the fused launch (plan-owned; null in the product)
    size_t fused_max_batch = 0;
    unsigned long long *d_counter = nullptr;  // one device word for ntt_count_noncanonical (no allocation per call)
    std::mutex counter_mu;                    // ... which is the only entry point that writes plan-owned state after creation
    std::vector<PassDesc> passes;  // = alts[0].passes: the default decomposition (ntt_plan_info 3 / 32+ / 64+)
    std::vector<PlanAlt> alts;     // launch-time alternatives, ascending min_batch (plan.h: plan_alternatives)
    std::vector<PassDesc> col_passes;  // ntt_forward_columns / ntt_inverse_columns: every stage as a column pass (plan.h: plan_column_passes)
    int forced_alt = -1;           // ntt_plan_set_policy: -1 = by batch, k >= 0 = always alternative k
    uint64_t lde_shift = 0;   // ntt_plan_set_coset / ntt_plan_set_coset_inverse: the shifts the vectors were made from
    uint64_t cinv_shift = 0;
};

static_assert(NTT_E_NOMEM == NTT_E_NOMEM_GUARD && NTT_E_INTERNAL == NTT_E_INTERNAL_GUARD, "guard.h codes = include/ntt_hip.h codes");

namespace {

// frees what a (possibly half-built) plan owns; the device must be current
void free_plan(ntt_plan *pl) {
    if (!pl) return;
    if (pl->tw_fwd) (void) hipFree(pl->tw_fwd);
    if (pl->tw_inv) (void) hipFree(pl->tw_inv);
    if (pl->tw_inv_sc) (void) hipFree(pl->tw_inv_sc);
    if (pl->d_fused_ctl) (void) hipFree(pl->d_fused_ctl);
    if (pl->d_counter) (void) hipFree(pl->d_counter);
    if (pl->lde_s) (void) hipFree(pl->lde_s);
    if (pl->cinv_u) (void) hipFree(pl->cinv_u);
    delete pl;
}
// ntt_plan_create builds the plan under this holder: an exception (std::bad_alloc from the alternatives' vectors)
// unwinds through it, so the guard's error return leaks neither the struct nor device memory
struct PlanDeleter {
    void operator()(ntt_plan *pl) const {
        if (!pl) return;
        DeviceGuard g(pl->device);
        free_plan(pl);
    }
};
using PlanHolder = std::unique_ptr<ntt_plan, PlanDeleter>;

size_t table_bytes(const ntt_plan *pl) { return ((size_t) 1 << pl->logn) * pl->word_bytes; }
size_t sc_table_bytes(const ntt_plan *pl) { return pl->word_bytes == 8 ? table_bytes(pl) / 2 : 0; }
// words of the coset vector for a blow-up of 2^beta (kept periodic up to one 16-byte chunk of 4-byte words)
size_t lde_s_words(const ntt_plan *pl, int beta) {
    const size_t n = (size_t) 1 << (pl->logn - beta);
    return n < 4 ? 4 : n;
}
// words of the coset-interpolation vector (periodic up to one 16-byte chunk of 4-byte words, like the coset vector)
size_t cinv_u_words(const ntt_plan *pl) {
    const size_t n = (size_t) 1 << pl->logn;
    return n < 4 ? 4 : n;
}
// the decomposition the launchers run for this batch
const std::vector<PassDesc> &passes_for(const ntt_plan *pl, size_t batch) { return ntt::passes_for(pl->alts, pl->forced_alt, batch); }
// ntt_plan_info 12
bool cinv_fused(const ntt_plan *pl) { return ntt::cinv_fused(*pl, pl->alts, pl->forced_alt); }

// batch == 0 is a valid no-op whatever the pointers are (an empty torch tensor has a null data_ptr)
int check_io(const ntt_plan *pl, const void *a, const void *b, size_t batch) {
    if (!pl) return NTT_E_ARG;
    if (batch == 0) return NTT_OK;
    if (!a || !b) return NTT_E_ARG;
    if (((uintptr_t) a | (uintptr_t) b) & 15u) return NTT_E_ARG;  // 16-byte vector accesses
    if (batch > 0x7FFFFFFFull) return NTT_E_ARG;
    return NTT_OK;
}

int check_layout(const ntt_plan *pl, int layout) {
    if (layout != NTT_LAYOUT_NATURAL && layout != NTT_LAYOUT_AIE_BLOCK16) return NTT_E_ARG;
    if (layout == NTT_LAYOUT_AIE_BLOCK16 && pl->logn < 4) return NTT_E_LAYOUT;
    return NTT_OK;
}

// the map arguments the three *_map entry points share (batch > 0): NTT_OK and *q = the word the kernel takes (the exponent of every
// row, or g^-1 mod 2N), or NTT_E_ARG
int check_map(const ntt_plan *pl, int kind, uint32_t param, const uint32_t *d_exp, int flags, uint32_t *q) {
    if (kind != NTT_MAP_MONOMIAL && kind != NTT_MAP_AUTOMORPHISM) return NTT_E_ARG;
    if (flags & ~NTT_MAP_MINUS_IDENTITY) return NTT_E_ARG;
    if ((uintptr_t) d_exp & 3u) return NTT_E_ARG;
    *q = param;
    if (kind == NTT_MAP_AUTOMORPHISM) {
        if (d_exp || !(param & 1u) || param >= (2u << pl->logn)) return NTT_E_ARG;
        *q = ntt::map_ginv(param, pl->logn);
    }
    return NTT_OK;
}
using u128 = unsigned __int128;
// d_exp[0 .. batch) against a written range [lo, hi)
bool exps_overlap(const uint32_t *d_exp, size_t batch, u128 lo, u128 hi) {
    const u128 e0 = (uintptr_t) d_exp, e1 = e0 + (u128) batch * 4;
    return d_exp && e0 < hi && lo < e1;
}

// One step of a sequence (sequence.h) to its launcher, inside the ROCTX range of that pass
int launch_step(const char *what, const ntt::Step &st, hipStream_t s) {
    RoctxRange pass(what, st.contig, st.args.s0 - st.args.mat_w, st.log_m);
    switch (st.family) {
        case ntt::STEP_MAT: return (int) ntt::launch_mat_pass(st.inverse, st.log_m, st.args, s);
        case ntt::STEP_PRODUCT: return (int) ntt::launch_product_mid(st.log_m, st.args, s);
        default: return (int) ntt::launch_pass(st.inverse, st.contig, st.log_m, st.args, s);
    }
}

// in2 != null: transform in[j] * in2[j] * pw_scale (plain) instead of in[j] (sequence.h: seq_forward)
// `forced`: the decomposition to run (a product picks ONE for all of its transforms); null = passes_for(batch)
int run_forward(ntt_plan *pl, const void *d_in, void *d_out, size_t batch, int layout, hipStream_t s,
                const void *in2 = nullptr, uint64_t pw_scale_plain = 1, const std::vector<PassDesc> *forced = nullptr) {
    RoctxRange whole(in2 ? "ntt_forward(product)" : "ntt_forward");
    const void *skip_if = nullptr;
#if defined(NTT_EXPERIMENT)
    if (pl->d_fused_ctl && !in2 && d_in != d_out && layout == NTT_LAYOUT_NATURAL && batch >= 64 && batch % 8 == 0 &&
        batch <= pl->fused_max_batch) {
        // one persistent XCD-local launch; the ordinary passes below then only run (device-side
        // decision, no host sync) if its check kernel did not certify the result
        hipError_t e = ntt::launch_fused_gl16(d_in, d_out, pl->tw_fwd, batch, pl->d_fused_ctl, s, pl->dbg);
        if (e != hipSuccess) return (int) e;
        skip_if = ntt::fused_gl16_ok_word(pl->d_fused_ctl);
        if (pl->dbg & (16 | 32 | 64)) return NTT_OK;  // timing experiments: fused launch alone
    }
#endif
    return ntt::seq_forward(*pl, forced ? *forced : passes_for(pl, batch), d_in, d_out, batch, layout, in2, pw_scale_plain, skip_if,
                            [&](const ntt::Step &st) { return launch_step("fwd pass", st, s); });
}

int run_inverse(ntt_plan *pl, const void *d_in, void *d_out, size_t batch, int layout, int scale,
                hipStream_t s, const std::vector<PassDesc> *forced = nullptr) {
    RoctxRange whole("ntt_inverse");
    return ntt::seq_inverse(*pl, forced ? *forced : passes_for(pl, batch), d_in, d_out, batch, layout, scale,
                            [&](const ntt::Step &st) { return launch_step("inv pass", st, s); });
}

// the four ntt_*_columns calls: validation here, the passes in sequence.h (seq_columns)
using ntt::COL_CINV;
using ntt::COL_LDE;
using ntt::COL_PLAIN;
using ntt::ColKind;
int run_columns(ntt_plan *pl, ColKind kind, const void *d_in, size_t in_pitch, void *d_out, size_t pitch, size_t width, size_t count, bool inverse,
                int scale, void *stream) {
    if (!pl) return NTT_E_ARG;
    if (pl->logn < MIN_COL_LOG_M) return NTT_E_LOGN;  // no column kernel shape below four stages
    if (width > pitch || width > in_pitch) return NTT_E_ARG;
    const bool empty = count == 0 || width == 0;
    if (!empty) {
        if (!d_in || !d_out) return NTT_E_ARG;
        if (((uintptr_t) d_in | (uintptr_t) d_out) & 15u) return NTT_E_ARG;
    }
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (inverse && !pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (kind == COL_LDE && pl->lde_beta == 0) return NTT_E_ARG;  // ntt_plan_set_coset first
    if (kind == COL_CINV && !pl->cinv_set) return NTT_E_ARG;     // ntt_plan_set_coset_inverse first
    if (empty) return NTT_OK;
    // size rule: N * pitch <= 2^NTT_MAX_LOGN words and logn + w <= NTT_MAX_LOGN -- what a size-2^28 transform obeys; the compact
    // source of the LDE obeys it with its own, smaller, row count
    const int beta = kind == COL_LDE ? pl->lde_beta : 0;
    const int w = ntt::mat_log_w(pl->word_bytes, width);
    if (pl->logn + w > NTT_MAX_LOGN || pitch > ((size_t) 1 << (NTT_MAX_LOGN - pl->logn)) || count > 0x7FFFFFFFull) return NTT_E_ARG;
    if (in_pitch > ((size_t) 1 << (NTT_MAX_LOGN - pl->logn + beta))) return NTT_E_ARG;
    const size_t N = (size_t) 1 << pl->logn, N_in = N >> beta;
    if (count > (SIZE_MAX / 16) / (N * pitch) || count > (SIZE_MAX / 16) / (N_in * in_pitch)) return NTT_E_ARG;
    // bytes from the first to the last live word of each buffer
    const size_t foot_in = ((count * N_in - 1) * in_pitch + width) * (size_t) pl->word_bytes;
    const size_t foot_out = ((count * N - 1) * pitch + width) * (size_t) pl->word_bytes;
    const uintptr_t in0 = (uintptr_t) d_in, out0 = (uintptr_t) d_out;
    if ((kind == COL_LDE || in0 != out0) && in0 < out0 + foot_out && out0 < in0 + foot_in) return NTT_E_ARG;  // in place (not the LDE), or apart
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    static const char *const names[3][2] = {{"ntt_forward_columns", "fwd columns pass"}, {"ntt_lde_columns", "lde columns pass"}, {"ntt_coset_inverse_columns", "coset inv columns pass"}};
    RoctxRange whole(kind == COL_PLAIN && inverse ? "ntt_inverse_columns" : names[kind][0]);
    const char *what = kind == COL_PLAIN && inverse ? "inv columns pass" : names[kind][1];
    return ntt::seq_columns(*pl, pl->col_passes, kind, d_in, in_pitch, d_out, pitch, width, count, inverse, scale,
                            [&](const ntt::Step &st) { return launch_step(what, st, s); });
}

// device-to-device, no host copy: over xGMI when the devices differ (hipMemcpyPeer), which is what the
// reference's on-chip table broadcast does below its host (src/aie2.py:96-104)
hipError_t copy_d2d(void *dst, int dst_dev, const void *from, int from_dev, size_t bytes) {
    if (bytes == 0 || !dst || !from) return hipSuccess;
    return dst_dev == from_dev ? hipMemcpy(dst, from, bytes, hipMemcpyDeviceToDevice) : hipMemcpyPeer(dst, dst_dev, from, from_dev, bytes);
}

}  // namespace

extern "C" {

int ntt_version(void) { return 500; /* 0.5.0 */ }

#if defined(NTT_PHASE_STAMPS)
// Diagnostic side build only (tools/ab_build.sh stamps -DNTT_PHASE_STAMPS -> ab/libntt_stamps.so; tools/phase_stamps.py): where
// the pass kernels of this process write their phase stamps (pass.h: stamp()).  [records][ntt::STAMP_RECORD] 64-bit slots, one
// record per wave of a launch; null = stamps go to a dummy record.  Never declared in include/ntt_hip.h.
int ntt_stamps_set(void *d_buf, size_t records) NTT_GUARD {
    ntt::stamp_buffer().buf = d_buf;
    ntt::stamp_buffer().records = (uint32_t) (records > 0xFFFFFFFFull ? 0xFFFFFFFFull : records);
    return NTT_OK;
} NTT_GUARD_END
#endif

#if defined(NTT_EXPERIMENT)
// libntt_hip_exp.so only (never declared in include/ntt_hip.h, never exported by the product): the timing switches of
// PassArgs::dbg for ONE plan, set explicitly instead of through the process environment (bench.py's VALU-floor leg).
// The symbol doubles as the build's identity: ntt_aie_amd/_lib.py refuses a library that exports it.
int ntt_plan_set_debug(ntt_plan_t pl, int flags) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    pl->dbg = flags;
    return NTT_OK;
} NTT_GUARD_END

// libntt_hip_exp.so only, never declared in include/ntt_hip.h: the accumulate launch of ntt_polymul_gadget_map_pre alone,
// d_out[i] = d_out[i] + d_addend[i] mod p over rows * N canonical words (tools/bench_negacyclic_map.py: the leg that maps and multiplies
// in separate calls adds through the same kernel as the fused call)
int ntt_add_rows_exp(ntt_plan_t pl, void *d_out, const void *d_addend, size_t rows, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_out, d_addend, rows);
    if (rc || rows == 0) return rc;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    return (int) ntt::launch_add_rows(pl->field, d_out, d_addend, rows << pl->logn, (hipStream_t) stream);
} NTT_GUARD_END
#endif

const char *ntt_error_string(int code) {
    switch (code) {
        case NTT_OK: return "ok";
        case NTT_E_ARG: return "invalid argument (null / misaligned pointer, size out of range)";
        case NTT_E_PRIME: return "unsupported modulus for this word size (must be odd, >= 3, and < 2^32 for 4-byte words)";
        case NTT_E_LOGN: return "logn out of range";
        case NTT_E_NOTABLE: return "twiddle table not set";
        case NTT_E_NOTINVERTIBLE: return "twiddle table has an entry that is not a unit mod p";
        case NTT_E_LAYOUT: return "AIE_BLOCK16 layout needs N >= 16";
        case NTT_E_RANGE: return "twiddle out of range [0, p)";
        case NTT_E_NODEVICE: return "no such HIP device";
        case NTT_E_NOMEM: return "out of host memory (a staging buffer of N words could not be allocated)";
        case NTT_E_INTERNAL: return "internal error (a C++ exception was caught at the C boundary)";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t) code);
    return "unknown error";
}

int ntt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ntt_plan_create(ntt_plan_t *out, int logn, uint64_t p, int word_bytes, int device) NTT_GUARD {
    if (!out) return NTT_E_ARG;
    *out = nullptr;
    if (word_bytes != 4 && word_bytes != 8) return NTT_E_ARG;
    if (logn < 1 || logn > NTT_MAX_LOGN) return NTT_E_LOGN;
    if ((p & 1) == 0 || p < 3) return NTT_E_PRIME;
    if (word_bytes == 4 && p > 0xFFFFFFFFull) return NTT_E_PRIME;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return NTT_E_NODEVICE;
    PlanHolder holder(new (std::nothrow) ntt_plan());
    ntt_plan *pl = holder.get();
    if (!pl) return NTT_E_NOMEM;
    pl->device = device;
    pl->logn = logn;
    pl->p = p;
    pl->word_bytes = word_bytes;
    pl->field = ntt::field_params(word_bytes, p);
    pl->ninv_plain = powmod(p / 2 + 1, (uint64_t) logn, p);  // (2^-1)^logn; 2^-1 = (p + 1) / 2 = p / 2 + 1 for odd p (no overflow at p near 2^64)
    pl->scale_tf = to_table_form(pl->ninv_plain, p, word_bytes);
    pl->alts = plan_alternatives(logn, word_bytes, p);
    pl->passes = pl->alts[0].passes;
    pl->col_passes = plan_column_passes(logn);
#if defined(NTT_EXPERIMENT)
    // Experiment knobs exist only in libntt_hip_exp.so (make exp; tools/): the product library reads NO environment
    // variable, so a stray NTT_DEBUG_FLAGS in a user's shell cannot redirect loads and stores.
    if (const char *e = getenv("NTT_TARGET_WGS")) {
        long v = atol(e);
        if (v > 0 && v < (1 << 24)) pl->target_wgs = (uint32_t) v, pl->target_wgs_col = 2 * pl->target_wgs;
    }
    if (const char *e = getenv("NTT_TARGET_WGS_COL")) {
        long v = atol(e);
        if (v > 0 && v < (1 << 24)) pl->target_wgs_col = (uint32_t) v;
    }
    if (const char *e = getenv("NTT_DEBUG_FLAGS")) pl->dbg = atoi(e);
    if (const char *e = getenv("NTT_ONLY_PASS")) pl->only_pass = atoi(e);
    if (const char *e = getenv("NTT_PASS_VARIANT")) pl->force_variant = atoi(e);
    if (const char *e = getenv("NTT_FUSED")) pl->fused = atoi(e);
    if (const char *e = getenv("NTT_LDE_UNFUSED")) pl->lde_unfused = atoi(e) != 0;  // tools/bench_lde.py: leg B
    if (const char *e = getenv("NTT_COSET_INV_UNFUSED")) pl->cinv_unfused = atoi(e) != 0;  // tools/bench_coset_inverse.py: leg B
    if (const char *e = getenv("NTT_MATVEC_SINGLE")) pl->mv_single = atoi(e) != 0;  // tools/bench_polymul_matvec.py: leg C
    if (const char *e = getenv("NTT_GADGET_UNFUSED")) pl->gadget_unfused = atoi(e) != 0;  // tools/bench_polymul_gadget.py: the decomposition kernel at every size
    if (const char *e = getenv("NTT_PLAN_SPLIT")) {  // "8,6,6" = CONTIG 8 stages + two 6-stage column passes
        std::vector<PassDesc> v;
        int s0 = 0;
        bool ok = true;
        for (const char *c = e; *c && ok;) {
            char *end = nullptr;
            const long m = strtol(c, &end, 10);
            if (end == c) break;
            if (v.empty()) ok = m >= 1 && m <= (word_bytes == 4 ? 14 : 13);
            else ok = m >= MIN_COL_LOG_M && m <= MAX_COL_LOG_M_WIDE;
            v.push_back({v.empty(), s0, (int) m, 0});
            s0 += (int) m;
            c = *end == ',' ? end + 1 : end;
        }
        if (v.size() > 1 && v[0].log_m < ntt::col_log_c(word_bytes)) ok = false;  // column tiles are 2^log_c words wide
        if (ok && s0 == logn && !v.empty()) {  // anything else: keep the planner's alternatives
            pl->passes = v;
            pl->alts.assign(1, PlanAlt{v, 0});
        }
    }
#endif
    DeviceGuard g(device);
    if (g.err != hipSuccess) return (int) g.err;
    hipError_t e = hipMalloc(&pl->tw_fwd, table_bytes(pl));
    if (e == hipSuccess) e = hipMalloc(&pl->tw_inv, table_bytes(pl));
    if (e == hipSuccess && sc_table_bytes(pl)) e = hipMalloc(&pl->tw_inv_sc, sc_table_bytes(pl));
    if (e == hipSuccess) e = hipMalloc(&pl->d_counter, sizeof(*pl->d_counter));
#if defined(NTT_EXPERIMENT)
    if (e == hipSuccess && pl->fused && logn == 16 && word_bytes == 8) {
        pl->fused_max_batch = (size_t) 1 << 20;
        e = hipMalloc(&pl->d_fused_ctl, ntt::fused_gl16_ctl_bytes(pl->fused_max_batch));
    }
#endif
    if (e != hipSuccess) return (int) e;  // the holder frees what was allocated
    *out = holder.release();
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_destroy(ntt_plan_t pl) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    DeviceGuard g(pl->device);
    free_plan(pl);
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_set_twiddles(ntt_plan_t pl, const void *host_T) NTT_GUARD {
    if (!pl || !host_T) return NTT_E_ARG;
    const size_t N = (size_t) 1 << pl->logn;
    const uint64_t p = pl->p;
    std::vector<uint64_t> T(N), Ti(N, 0);
    for (size_t i = 0; i < N; i++)
        T[i] = pl->word_bytes == 4 ? ((const uint32_t *) host_T)[i] : ((const uint64_t *) host_T)[i];
    for (size_t i = 1; i < N; i++)
        if (T[i] >= p) return NTT_E_RANGE;
    T[0] %= p;  // T[0] is never read by the network (src/test.cpp:45 uses h+i >= 1)
    const bool inv_ok = invert_table(T, p, Ti);
    std::vector<unsigned char> buf_f(table_bytes(pl)), buf_i(table_bytes(pl));
    if (pl->word_bytes == 4) {
        for (size_t i = 0; i < N; i++) {
            ((uint32_t *) buf_f.data())[i] = (uint32_t) to_table_form(T[i], p, 4);
            ((uint32_t *) buf_i.data())[i] = (uint32_t) to_table_form(Ti[i], p, 4);
        }
    } else {
        for (size_t i = 0; i < N; i++) {
            ((uint64_t *) buf_f.data())[i] = to_table_form(T[i], p, 8);
            ((uint64_t *) buf_i.data())[i] = to_table_form(Ti[i], p, 8);
        }
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipError_t e = hipMemcpy(pl->tw_fwd, buf_f.data(), buf_f.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->tw_inv, buf_i.data(), buf_i.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && pl->tw_inv_sc && inv_ok) {
        std::vector<uint64_t> sc(N / 2);
        for (size_t i = 0; i < N / 2; i++) sc[i] = to_table_form(mulmod(Ti[N / 2 + i], pl->ninv_plain, p), p, 8);
        e = hipMemcpy(pl->tw_inv_sc, sc.data(), sc.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return (int) e;
    pl->has_table = true;
    pl->has_inv = inv_ok;
    return NTT_OK;
} NTT_GUARD_END

int ntt_make_table(ntt_plan_t pl, int kind, uint64_t g, void *host_T) NTT_GUARD {
    if (!pl || !host_T) return NTT_E_ARG;
    const uint64_t N = 1ull << pl->logn;
    std::vector<uint64_t> T;
    if (kind < 0 || kind > 2 || !make_table(kind, pl->logn, pl->p, g, T)) return NTT_E_ARG;
    for (uint64_t i = 0; i < N; i++) {
        if (pl->word_bytes == 4) ((uint32_t *) host_T)[i] = (uint32_t) T[i];
        else ((uint64_t *) host_T)[i] = T[i];
    }
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_generate_twiddles(ntt_plan_t pl, int kind, uint64_t g) NTT_GUARD {
    if (!pl || kind < 0 || kind > 2) return NTT_E_ARG;
    const uint64_t N = 1ull << pl->logn, p = pl->p;
    uint64_t base;
    if (kind == 2) {
        if ((p - 1) % (2 * N)) return NTT_E_ARG;
        base = invmod(powmod(g, (p - 1) / (2 * N), p), p);  // psi^-1
    } else {
        if (kind == 1 && (p - 1) % N) return NTT_E_ARG;
        base = powmod(g, (p - 1) / N, p);                           // w (integer division, src/test.cpp:28)
    }
    if (base == 0) return NTT_E_NOTINVERTIBLE;
    const uint64_t base_inv = invmod(base, p);
    if (base_inv == 0) return NTT_E_NOTINVERTIBLE;
    const int wb = pl->word_bytes;
    const uint64_t one_m = to_table_form(1 % p, p, wb);
    DeviceGuard g_(pl->device);
    if (g_.err != hipSuccess) return (int) g_.err;
    hipError_t e = ntt::launch_gen_table(pl->field, pl->tw_fwd, pl->logn, kind, to_table_form(base, p, wb), one_m, nullptr);
    if (e == hipSuccess) e = ntt::launch_gen_table(pl->field, pl->tw_inv, pl->logn, kind, to_table_form(base_inv, p, wb), one_m, nullptr);
    if (e == hipSuccess && pl->tw_inv_sc)  // 8-byte words: stage-0 twiddles of the scaled inverse, T^-1[N/2 + i] * N^-1
        e = ntt::launch_scale_table(pl->field, (const uint64_t *) pl->tw_inv + N / 2, pl->tw_inv_sc, N / 2, pl->scale_tf, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return (int) e;
    pl->has_table = true;
    pl->has_inv = true;  // every entry is a power of a unit
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_get_twiddles(ntt_plan_t pl, int inverse, void *host_T) NTT_GUARD {
    if (!pl || !host_T) return NTT_E_ARG;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (inverse && !pl->has_inv) return NTT_E_NOTINVERTIBLE;
    DeviceGuard g_(pl->device);
    if (g_.err != hipSuccess) return (int) g_.err;
    hipError_t e = hipMemcpy(host_T, inverse ? pl->tw_inv : pl->tw_fwd, table_bytes(pl), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int) e;
    // table (Montgomery) form -> plain residues: x * R^-1
    const size_t N = (size_t) 1 << pl->logn;
    const uint64_t p = pl->p;
    const uint64_t rinv = invmod(to_table_form(1 % p, p, pl->word_bytes), p);  // R is a power of two, p odd: always a unit
    for (size_t i = 0; i < N; i++) {
        if (pl->word_bytes == 4) ((uint32_t *) host_T)[i] = (uint32_t) mulmod(((uint32_t *) host_T)[i], rinv, p);
        else ((uint64_t *) host_T)[i] = mulmod(((uint64_t *) host_T)[i], rinv, p);
    }
    return NTT_OK;
} NTT_GUARD_END

int ntt_make_roots(ntt_plan_t pl, uint64_t g, void *host_T) NTT_GUARD { return ntt_make_table(pl, 0, g, host_T); } NTT_GUARD_END

int64_t ntt_plan_info(ntt_plan_t pl, int what) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    switch (what) {
        case 0: return pl->logn;
        case 1: return pl->word_bytes;
        case 2: return pl->device;
        case 3: return (int64_t) pl->passes.size();
        case 4: return pl->has_inv ? 1 : 0;
        case 5: return pl->d_fused_ctl ? 1 : 0;
        case 6: return (int64_t) pl->alts.size();
        case 7: return pl->forced_alt;
        case 9: return pl->lde_beta;
        case 10: return ntt::lde_fused(*pl) ? 1 : 0;
        case 11: return pl->cinv_set ? 1 : 0;
        case 12: return cinv_fused(pl) ? 1 : 0;
        case 13: return (int64_t) pl->col_passes.size();
        case 14: {  // does ntt_polymul_matvec_pre run two-output middle launches (the pinned decomposition, or the one of a small batch)
            const std::vector<PassDesc> &passes = passes_for(pl, 1);
            return ntt::polymul_dot_fused(*pl, passes, 1) && ntt::polymul_matvec_paired(*pl, passes) ? 1 : 0;
        }
        case 15: {  // does ntt_polymul_gadget_pre decompose inside the middle launch (the pinned decomposition, or the one of a small batch)
            return ntt::polymul_gadget_fused(*pl, passes_for(pl, 1), 1) ? 1 : 0;
        }
        case 8: {  // capacity for ntt_forward_profile whatever the batch
            size_t k = 0;
            for (const PlanAlt &a : pl->alts) k = a.passes.size() > k ? a.passes.size() : k;
            return (int64_t) k;
        }
        default: break;
    }
    if (what >= 256 && what < 256 + 16 * (int) pl->alts.size()) {
        const PlanAlt &alt = pl->alts[(size_t) (what - 256) / 16];
        const int k = (what - 256) % 16;
        if (k == 0) return (int64_t) alt.passes.size();
        if (k >= 1 && k <= 7) return k - 1 < (int) alt.passes.size() ? alt.passes[(size_t) k - 1].log_m : NTT_E_ARG;
        if (k >= 8 && k <= 14) return k - 8 < (int) alt.passes.size() ? alt.passes[(size_t) k - 8].s0 : NTT_E_ARG;
        return (int64_t) alt.min_batch;  // k == 15
    }
    if (what >= 512 && what < 512 + 16 * (int) pl->alts.size()) {  // kernel variant of pass k of alternative a (PassDesc::variant)
        const PlanAlt &alt = pl->alts[(size_t) (what - 512) / 16];
        const int k = (what - 512) % 16;
        return k < (int) alt.passes.size() ? alt.passes[(size_t) k].variant : NTT_E_ARG;
    }
    if (what >= 96 && what < 96 + (int) pl->col_passes.size()) return pl->col_passes[what - 96].log_m;
    if (what >= 128 && what < 128 + (int) pl->col_passes.size()) return pl->col_passes[what - 128].s0;
    if (what >= 32 && what < 32 + (int) pl->passes.size()) return pl->passes[what - 32].log_m;
    if (what >= 64 && what < 64 + (int) pl->passes.size()) return pl->passes[what - 64].s0;
#if defined(NTT_EXPERIMENT)
    if (what >= 16 && what < 16 + 12 && pl->d_fused_ctl) {  // diagnostics: words of the last fused launch (blocking)
        uint32_t w[12];
        DeviceGuard g(pl->device);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(w, pl->d_fused_ctl, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
            return NTT_E_ARG;
        return w[what - 16];  // 0-7 slots per XCC, 8 status, 9 b_done, 10 ok
    }
#endif
    return NTT_E_ARG;
} NTT_GUARD_END

int ntt_plan_select(ntt_plan_t pl, size_t batch) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    return pl->forced_alt >= 0 ? pl->forced_alt : select_alternative(pl->alts, batch);
} NTT_GUARD_END

int ntt_plan_set_policy(ntt_plan_t pl, int alternative) NTT_GUARD {
    if (!pl || alternative < -1 || alternative >= (int) pl->alts.size()) return NTT_E_ARG;
    pl->forced_alt = alternative;
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_set_coset(ntt_plan_t pl, int log_blowup, uint64_t shift) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    const int max_beta = pl->logn - 1 < 4 ? pl->logn - 1 : 4;
    if (log_blowup < 1 || log_blowup > max_beta) return NTT_E_ARG;
    if (shift == 0 || shift >= pl->p) return NTT_E_ARG;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    const size_t words = lde_s_words(pl, log_blowup);
    void *d_s = nullptr;
    hipError_t e = hipMalloc(&d_s, words * (size_t) pl->word_bytes);
    if (e != hipSuccess) return (int) e;
    e = ntt::launch_gen_coset(pl->field, d_s, pl->logn - log_blowup, (uint32_t) words, to_table_form(shift, pl->p, pl->word_bytes),
                              to_table_form(1 % pl->p, pl->p, pl->word_bytes), nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void) hipFree(d_s);
        return (int) e;
    }
    if (pl->lde_s) (void) hipFree(pl->lde_s);  // a replaced setting (configuration call: nothing is in flight on this plan)
    pl->lde_s = d_s;
    pl->lde_beta = log_blowup;
    pl->lde_shift = shift;
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_set_coset_inverse(ntt_plan_t pl, uint64_t shift) NTT_GUARD {
    if (!pl) return NTT_E_ARG;
    if (shift == 0 || shift >= pl->p) return NTT_E_ARG;
    const uint64_t shift_inv = invmod(shift, pl->p);
    if (shift_inv == 0) return NTT_E_NOTINVERTIBLE;  // shares a factor with a composite modulus
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    const size_t words = cinv_u_words(pl);
    void *d_u = nullptr;
    hipError_t e = hipMalloc(&d_u, words * (size_t) pl->word_bytes);
    if (e != hipSuccess) return (int) e;
    // u[i] = (shift^-1)^bitrev(i) * N^-1: the coset generator, started from the table form of N^-1 instead of 1
    e = ntt::launch_gen_coset(pl->field, d_u, pl->logn, (uint32_t) words, to_table_form(shift_inv, pl->p, pl->word_bytes), pl->scale_tf, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void) hipFree(d_u);
        return (int) e;
    }
    if (pl->cinv_u) (void) hipFree(pl->cinv_u);  // a replaced setting (configuration call: nothing is in flight on this plan)
    pl->cinv_u = d_u;
    pl->cinv_set = true;
    pl->cinv_shift = shift;
    return NTT_OK;
} NTT_GUARD_END

int ntt_plan_clone(ntt_plan_t src, int device, ntt_plan_t *out) NTT_GUARD {
    if (!out) return NTT_E_ARG;
    *out = nullptr;
    if (!src) return NTT_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return NTT_E_NODEVICE;
    ntt_plan_t pl = nullptr;
    int rc = ntt_plan_create(&pl, src->logn, src->p, src->word_bytes, device);
    if (rc != NTT_OK) return rc;
    pl->alts = src->alts;  // an experiment split or a forced policy travels with the plan
    pl->passes = src->passes;
    pl->col_passes = src->col_passes;
    pl->forced_alt = src->forced_alt;
    pl->target_wgs = src->target_wgs;
    pl->target_wgs_col = src->target_wgs_col;
    if (src->has_table) {
        DeviceGuard g(device);
        hipError_t e = g.err;
        if (e == hipSuccess) e = copy_d2d(pl->tw_fwd, device, src->tw_fwd, src->device, table_bytes(src));
        if (e == hipSuccess) e = copy_d2d(pl->tw_inv, device, src->tw_inv, src->device, table_bytes(src));
        if (e == hipSuccess) e = copy_d2d(pl->tw_inv_sc, device, src->tw_inv_sc, src->device, sc_table_bytes(src));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void) ntt_plan_destroy(pl);
            return (int) e;
        }
        pl->has_table = true;
        pl->has_inv = src->has_inv;
    }
    pl->lde_unfused = src->lde_unfused;
    if (src->lde_beta > 0) {  // the coset setting and its vector, device to device like the tables
        const size_t bytes = lde_s_words(src, src->lde_beta) * (size_t) src->word_bytes;
        DeviceGuard g(device);
        hipError_t e = g.err;
        if (e == hipSuccess) e = hipMalloc(&pl->lde_s, bytes);
        if (e == hipSuccess) e = copy_d2d(pl->lde_s, device, src->lde_s, src->device, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void) ntt_plan_destroy(pl);
            return (int) e;
        }
        pl->lde_beta = src->lde_beta;
        pl->lde_shift = src->lde_shift;
    }
    pl->cinv_unfused = src->cinv_unfused;
    pl->mv_single = src->mv_single;
    pl->gadget_unfused = src->gadget_unfused;
    if (src->cinv_set) {  // ... and the coset-interpolation setting with its vector
        const size_t bytes = cinv_u_words(src) * (size_t) src->word_bytes;
        DeviceGuard g(device);
        hipError_t e = g.err;
        if (e == hipSuccess) e = hipMalloc(&pl->cinv_u, bytes);
        if (e == hipSuccess) e = copy_d2d(pl->cinv_u, device, src->cinv_u, src->device, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void) ntt_plan_destroy(pl);
            return (int) e;
        }
        pl->cinv_set = true;
        pl->cinv_shift = src->cinv_shift;
    }
    *out = pl;
    return NTT_OK;
} NTT_GUARD_END

int ntt_forward(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int out_layout, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if ((rc = check_layout(pl, out_layout)) != NTT_OK) return rc;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    return run_forward(pl, d_in, d_out, batch, out_layout, (hipStream_t) stream);
} NTT_GUARD_END

int ntt_lde(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int out_layout, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (pl->lde_beta == 0) return NTT_E_ARG;
    if ((rc = check_layout(pl, out_layout)) != NTT_OK) return rc;
    if (batch == 0) return NTT_OK;
    const int beta = pl->lde_beta;
    const uintptr_t in0 = (uintptr_t) d_in, in1 = in0 + ((batch << (pl->logn - beta)) * (size_t) pl->word_bytes);
    const uintptr_t out0 = (uintptr_t) d_out, out1 = out0 + ((batch << pl->logn) * (size_t) pl->word_bytes);
    if (in0 < out1 && out0 < in1) return NTT_E_ARG;  // the first pass writes rows of d_out while later workgroups still read d_in
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_lde");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);
    if (!ntt::lde_fused(*pl)) {
        // expansion as a launch of its own, then the ordinary transform in place
        hipError_t e = ntt::launch_lde_expand(pl->field, d_in, pl->lde_s, d_out, pl->logn, beta, batch, s);
        if (e != hipSuccess) return (int) e;
        return run_forward(pl, d_out, d_out, batch, out_layout, s, nullptr, 1, &passes);
    }
    return ntt::seq_lde(*pl, passes, d_in, d_out, batch, out_layout, [&](const ntt::Step &st) { return launch_step("lde pass", st, s); });
} NTT_GUARD_END

int ntt_forward_profile(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int out_layout,
                        void *stream, float *ms_per_pass, int max_passes, int *n_passes) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!ms_per_pass || !n_passes) return NTT_E_ARG;
    const std::vector<PassDesc> &passes = passes_for(pl, batch);
    *n_passes = (int) passes.size();
    if (max_passes < (int) passes.size()) return NTT_E_ARG;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    const size_t np = passes.size();
    std::vector<hipEvent_t> ev;
    ev.reserve(np + 1);
    for (size_t i = 0; i <= np; i++) {
        hipEvent_t x;
        const hipError_t ce = hipEventCreate(&x);
        if (ce != hipSuccess) {  // destroy the ones already made
            for (auto &y : ev) (void) hipEventDestroy(y);
            return (int) ce;
        }
        ev.push_back(x);
    }
    hipError_t e = hipEventRecord(ev[0], s);
    ntt::PlanFacts every_pass = *pl;  // (experiment build: NTT_ONLY_PASS does not apply here, every pass is timed)
    every_pass.only_pass = -1;
    if (e == hipSuccess)
        e = (hipError_t) ntt::seq_forward(every_pass, passes, d_in, d_out, batch, out_layout, nullptr, 1, nullptr, [&](const ntt::Step &st) {
            const int rc = launch_step("fwd pass", st, s);
            return rc ? rc : (int) hipEventRecord(ev[(size_t) st.pass + 1], s);
        });
    if (e == hipSuccess) e = hipEventSynchronize(ev[np]);
    for (size_t i = 0; i < np && e == hipSuccess; i++) e = hipEventElapsedTime(&ms_per_pass[i], ev[i], ev[i + 1]);
    for (auto &x : ev) (void) hipEventDestroy(x);
    return (int) e;
} NTT_GUARD_END

int ntt_inverse(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int in_layout, int scale,
                void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if ((rc = check_layout(pl, in_layout)) != NTT_OK) return rc;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    return run_inverse(pl, d_in, d_out, batch, in_layout, scale, (hipStream_t) stream);
} NTT_GUARD_END

int ntt_forward_columns(ntt_plan_t pl, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, void *stream) NTT_GUARD {
    return run_columns(pl, COL_PLAIN, d_in, pitch, d_out, pitch, width, count, false, 0, stream);
} NTT_GUARD_END

int ntt_inverse_columns(ntt_plan_t pl, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, int scale, void *stream) NTT_GUARD {
    return run_columns(pl, COL_PLAIN, d_in, pitch, d_out, pitch, width, count, true, scale, stream);
} NTT_GUARD_END

int ntt_lde_columns(ntt_plan_t pl, const void *d_in, size_t in_pitch, void *d_out, size_t out_pitch, size_t width, size_t count, void *stream) NTT_GUARD {
    return run_columns(pl, COL_LDE, d_in, in_pitch, d_out, out_pitch, width, count, false, 0, stream);
} NTT_GUARD_END

int ntt_coset_inverse_columns(ntt_plan_t pl, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, void *stream) NTT_GUARD {
    return run_columns(pl, COL_CINV, d_in, pitch, d_out, pitch, width, count, true, 0, stream);
} NTT_GUARD_END

int ntt_coset_inverse(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int in_layout, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (!pl->cinv_set) return NTT_E_ARG;
    if ((rc = check_layout(pl, in_layout)) != NTT_OK) return rc;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_coset_inverse");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);
    if (!ntt::cinv_pass_fused(*pl, passes)) {
        // the unscaled inverse, then the scaling as a launch of its own, in place on the output
        rc = run_inverse(pl, d_in, d_out, batch, in_layout, 0, s, &passes);
        if (rc) return rc;
        return (int) ntt::launch_row_scale(pl->field, d_out, pl->cinv_u, pl->logn, batch, s);
    }
    return ntt::seq_coset_inverse(*pl, passes, d_in, d_out, batch, in_layout, [&](const ntt::Step &st) { return launch_step("coset inv pass", st, s); });
} NTT_GUARD_END

int ntt_pointwise_mul(ntt_plan_t pl, const void *d_a, const void *d_b, void *d_out, size_t batch,
                      uint64_t scale, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_b, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u))) return NTT_E_ARG;
    if (scale >= pl->p) return NTT_E_RANGE;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    const size_t count = batch << pl->logn;
    const hipError_t e = ntt::launch_pointwise(pl->field, d_a, d_b, d_out, count, scale, (hipStream_t) stream);
    return (int) e;
} NTT_GUARD_END

int ntt_polymul_negacyclic(ntt_plan_t pl, void *d_a, void *d_b, void *d_out, size_t batch, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_b, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u))) return NTT_E_ARG;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    // With the Longa-Naehrig psi^-1 table the forward negacyclic NTT is the UNSCALED
    // inverse network and the inverse negacyclic NTT is N^-1 * forward network
    // (SURVEY F6-ii), so  c = Fwd( InvU(a) . InvU(b) . N^-1 ).
    const std::vector<PassDesc> &passes = passes_for(pl, batch);
    if (ntt::polymul_fused(*pl, passes, batch))  // inverse column passes, the fused middle, forward column passes (sequence.h)
        return ntt::seq_polymul_fused(*pl, passes, d_a, d_b, d_out, batch, [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT ? "product: fused middle" : st.inverse ? "product: inv pass" : "product: fwd pass", st, s);
        });
    if (ntt::operands_contiguous(*pl, d_a, d_b, batch)) {
        // the operands are one [2*batch][N] buffer: both unscaled inverse transforms as ONE launch per pass
        // (the decomposition is the one selected for `batch`, as ntt_plan_select documents -- not for the 2*batch rows of this launch)
        rc = run_inverse(pl, d_a, d_a, 2 * batch, NTT_LAYOUT_NATURAL, 0, s, &passes);
        if (rc) return rc;
    } else {
        rc = run_inverse(pl, d_a, d_a, batch, NTT_LAYOUT_NATURAL, 0, s, &passes);
        if (rc) return rc;
        rc = run_inverse(pl, d_b, d_b, batch, NTT_LAYOUT_NATURAL, 0, s, &passes);
        if (rc) return rc;
    }
    // pointwise product * N^-1 folded into the first pass of the final forward transform
    return run_forward(pl, d_a, d_out, batch, NTT_LAYOUT_NATURAL, s, d_b, pl->ninv_plain, &passes);
} NTT_GUARD_END

int ntt_polymul_prepare(ntt_plan_t pl, const void *d_b, void *d_bhat, size_t rows, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_b, d_bhat, rows);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (rows == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    // the prepared form IS the unscaled inverse in natural order: nothing else to it (include/ntt_hip.h)
    return run_inverse(pl, d_b, d_bhat, rows, NTT_LAYOUT_NATURAL, 0, (hipStream_t) stream);
} NTT_GUARD_END

int ntt_polymul_negacyclic_pre(ntt_plan_t pl, void *d_a, const void *d_bhat, size_t bhat_rows, void *d_out, size_t batch, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_bhat, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u))) return NTT_E_ARG;
    if (batch && bhat_rows != 1 && bhat_rows != batch) return NTT_E_ARG;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    {  // bhat is read while a and out are written: it lies apart from both (out may be a)
        const size_t row = table_bytes(pl);
        const uintptr_t h0 = (uintptr_t) d_bhat, h1 = h0 + bhat_rows * row;
        for (const void *buf : {(const void *) d_a, (const void *) d_out}) {
            const uintptr_t b0 = (uintptr_t) buf, b1 = b0 + batch * row;
            if (b0 < h1 && h0 < b1) return NTT_E_ARG;
        }
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_polymul_negacyclic_pre");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);
    return ntt::seq_polymul_pre(
        *pl, passes, d_a, d_bhat, bhat_rows, d_out, batch,
        [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT ? "product(pre): fused middle" : st.inverse ? "product(pre): inv pass" : "product(pre): fwd pass", st, s);
        },
        [&](void *buf, const void *row) { return (int) ntt::launch_pointwise_row(pl->field, buf, row, pl->logn, batch, pl->ninv_plain, s); });
} NTT_GUARD_END

int ntt_polymul_dot_pre(ntt_plan_t pl, void *d_a, const void *d_bhat, size_t bhat_rows, size_t terms, void *d_out, size_t batch, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_bhat, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u))) return NTT_E_ARG;
    if (batch && bhat_rows != 1 && bhat_rows != batch) return NTT_E_ARG;
    if (batch && (terms == 0 || terms > 0x7FFFFFFFull / batch)) return NTT_E_ARG;  // the inverse passes run over terms * batch rows
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    {
        const size_t row = table_bytes(pl);
        const uintptr_t a0 = (uintptr_t) d_a, a1 = a0 + terms * batch * row, o0 = (uintptr_t) d_out, o1 = o0 + batch * row;
        const uintptr_t h0 = (uintptr_t) d_bhat, h1 = h0 + terms * bhat_rows * row;
        // out is term 0's block of a or lies apart from all of a: every other overlap is overwritten while terms are still to be read
        if (o0 != a0 && o0 < a1 && a0 < o1) return NTT_E_ARG;
        // bhat is read while a and out are written: it lies apart from both
        if ((a0 < h1 && h0 < a1) || (o0 < h1 && h0 < o1)) return NTT_E_ARG;
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_polymul_dot_pre");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);  // by batch, not by terms * batch (include/ntt_hip.h)
    return ntt::seq_polymul_dot(
        *pl, passes, d_a, d_bhat, bhat_rows, terms, d_out, batch,
        [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT ? "product(dot): fused middle" : st.inverse ? "product(dot): inv pass" : "product(dot): fwd pass", st, s);
        },
        [&](void *buf, const void *hat) {
            RoctxRange sum("product(dot): row sum");
            return (int) ntt::launch_dot_rows(pl->field, buf, hat, pl->logn, batch, bhat_rows, terms, ntt::pw_scale_form(*pl, pl->ninv_plain), s);
        });
} NTT_GUARD_END

int ntt_polymul_matvec_pre(ntt_plan_t pl, void *d_a, const void *d_bhat, size_t bhat_rows, size_t terms, size_t outs, void *d_out, size_t batch,
                           void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_bhat, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u))) return NTT_E_ARG;
    if (batch && bhat_rows != 1 && bhat_rows != batch) return NTT_E_ARG;
    if (batch && (terms == 0 || terms > 0x7FFFFFFFull / batch)) return NTT_E_ARG;  // the inverse passes run over terms * batch rows
    if (batch && (outs == 0 || outs > 0x7FFFFFFFull / batch)) return NTT_E_ARG;    // the forward passes over outs * batch rows
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    {
        using u128 = unsigned __int128;
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;  // no buffer ends beyond that: three ranges that cannot wrap
        const u128 a0 = (uintptr_t) d_a, a1 = a0 + (u128) terms * batch * row, o0 = (uintptr_t) d_out, o1 = o0 + (u128) outs * batch * row;
        const u128 h0 = (uintptr_t) d_bhat, h1 = h0 + (u128) outs * terms * bhat_rows * row;
        if (a1 > top || o1 > top || h1 > top) return NTT_E_ARG;
        // out lies apart from all of a -- the middle launches of later outputs still read a -- and bhat, which is read while a and out
        // are written, apart from both
        if ((o0 < a1 && a0 < o1) || (a0 < h1 && h0 < a1) || (o0 < h1 && h0 < o1)) return NTT_E_ARG;
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_polymul_matvec_pre");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);  // by batch, as ntt_polymul_dot_pre selects it
    return ntt::seq_polymul_matvec(
        *pl, passes, d_a, d_bhat, bhat_rows, terms, outs, d_out, batch,
        [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT ? (st.args.mv_outs ? "product(matvec): fused middle, two outputs" : "product(matvec): fused middle")
                               : st.inverse                   ? "product(matvec): inv pass"
                                                              : "product(matvec): fwd pass",
                               st, s);
        },
        [&](void *buf, const void *hat, void *out) {
            RoctxRange sum("product(matvec): row sums");
            return (int) ntt::launch_matvec_rows(pl->field, buf, hat, out, pl->logn, batch, bhat_rows, terms, outs, ntt::pw_scale_form(*pl, pl->ninv_plain), s);
        });
} NTT_GUARD_END

int ntt_gadget_decompose(ntt_plan_t pl, const void *d_a, size_t polys, size_t batch, int log_base, int levels, int low_bits, void *d_digits,
                         void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_digits, batch);
    if (rc) return rc;
    if (batch == 0) return NTT_OK;
    if (!ntt::gadget_params_ok(pl->p, log_base, levels, low_bits)) return NTT_E_ARG;
    if (polys == 0 || polys > 0x7FFFFFFFull / batch / (size_t) levels) return NTT_E_ARG;  // the digits are polys * levels * batch rows of a product
    {
        using u128 = unsigned __int128;
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;
        const u128 a0 = (uintptr_t) d_a, a1 = a0 + (u128) polys * batch * row, g0 = (uintptr_t) d_digits, g1 = g0 + (u128) polys * (u128) levels * batch * row;
        if (a1 > top || g1 > top || (a0 < g1 && g0 < a1)) return NTT_E_ARG;
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    RoctxRange whole("ntt_gadget_decompose");
    return (int) ntt::launch_gadget_decompose(pl->field, d_a, d_digits, pl->logn, polys, batch, log_base, levels, low_bits, (hipStream_t) stream);
} NTT_GUARD_END

int ntt_polymul_gadget_pre(ntt_plan_t pl, const void *d_a, size_t polys, int log_base, int levels, int low_bits, void *d_work, const void *d_bhat, size_t bhat_rows,
                           size_t outs, void *d_out, size_t batch, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_bhat, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u) || !d_work || ((uintptr_t) d_work & 15u))) return NTT_E_ARG;
    if (batch && bhat_rows != 1 && bhat_rows != batch) return NTT_E_ARG;
    if (batch && !ntt::gadget_params_ok(pl->p, log_base, levels, low_bits)) return NTT_E_ARG;
    if (batch && (polys == 0 || polys > 0x7FFFFFFFull / batch / (size_t) levels)) return NTT_E_ARG;  // terms * batch rows, terms = polys * levels
    if (batch && (outs == 0 || outs > 0x7FFFFFFFull / batch)) return NTT_E_ARG;                      // the forward passes over outs * batch rows
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    const size_t terms = polys * (size_t) levels;
    {
        using u128 = unsigned __int128;
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;  // no buffer ends beyond that: four ranges that cannot wrap
        const u128 lo[4] = {(uintptr_t) d_a, (uintptr_t) d_work, (uintptr_t) d_bhat, (uintptr_t) d_out};
        const u128 hi[4] = {lo[0] + (u128) polys * batch * row, lo[1] + (u128) terms * batch * row, lo[2] + (u128) outs * terms * bhat_rows * row,
                            lo[3] + (u128) outs * batch * row};
        for (int i = 0; i < 4; ++i) {
            if (hi[i] > top) return NTT_E_ARG;
            for (int j = 0; j < i; ++j)
                if (lo[i] < hi[j] && lo[j] < hi[i]) return NTT_E_ARG;  // pairwise disjoint
        }
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_polymul_gadget_pre");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);  // by batch, as ntt_polymul_matvec_pre selects it
    return ntt::seq_polymul_gadget(
        *pl, passes, d_a, polys, log_base, levels, low_bits, d_work, d_bhat, bhat_rows, outs, d_out, batch,
        [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT
                                   ? (st.args.gad_levels ? (st.args.mv_outs ? "product(gadget): fused middle with digits, two outputs" : "product(gadget): fused middle with digits")
                                      : st.args.mv_outs  ? "product(gadget): fused middle, two outputs"
                                                         : "product(gadget): fused middle")
                               : st.inverse ? "product(gadget): inv pass"
                                            : "product(gadget): fwd pass",
                               st, s);
        },
        [&](void *buf, const void *hat, void *out) {
            RoctxRange sum("product(gadget): row sums");
            return (int) ntt::launch_matvec_rows(pl->field, buf, hat, out, pl->logn, batch, bhat_rows, terms, outs, ntt::pw_scale_form(*pl, pl->ninv_plain), s);
        },
        [&](const void *src, void *digits) {
            RoctxRange dec("product(gadget): decomposition");
            return (int) ntt::launch_gadget_decompose(pl->field, src, digits, pl->logn, polys, batch, log_base, levels, low_bits, s);
        });
} NTT_GUARD_END

int ntt_negacyclic_map(ntt_plan_t pl, const void *d_in, void *d_out, size_t polys, size_t batch, int kind, uint32_t param, const uint32_t *d_exp, int flags,
                       void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (batch == 0) return NTT_OK;
    uint32_t q;
    if ((rc = check_map(pl, kind, param, d_exp, flags, &q))) return rc;
    if (polys == 0 || polys > 0x7FFFFFFFull / batch) return NTT_E_ARG;
    {
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;
        const u128 a0 = (uintptr_t) d_in, a1 = a0 + (u128) polys * batch * row, o0 = (uintptr_t) d_out, o1 = o0 + (u128) polys * batch * row;
        // out of place only: the gather reads the whole row
        if (a1 > top || o1 > top || (a0 < o1 && o0 < a1) || exps_overlap(d_exp, batch, o0, o1)) return NTT_E_ARG;
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    RoctxRange whole("ntt_negacyclic_map");
    return (int) ntt::launch_negacyclic_map(pl->field, d_in, d_out, pl->logn, polys, batch, kind, q, d_exp, flags & NTT_MAP_MINUS_IDENTITY, 0, 0, 0, (hipStream_t) stream);
} NTT_GUARD_END

int ntt_gadget_decompose_map(ntt_plan_t pl, const void *d_a, size_t polys, size_t batch, int kind, uint32_t param, const uint32_t *d_exp, int flags, int log_base,
                             int levels, int low_bits, void *d_digits, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_digits, batch);
    if (rc) return rc;
    if (batch == 0) return NTT_OK;
    uint32_t q;
    if ((rc = check_map(pl, kind, param, d_exp, flags, &q))) return rc;
    if (!ntt::gadget_params_ok(pl->p, log_base, levels, low_bits)) return NTT_E_ARG;
    if (polys == 0 || polys > 0x7FFFFFFFull / batch / (size_t) levels) return NTT_E_ARG;  // the digits are polys * levels * batch rows of a product
    {
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;
        const u128 a0 = (uintptr_t) d_a, a1 = a0 + (u128) polys * batch * row, g0 = (uintptr_t) d_digits, g1 = g0 + (u128) polys * (u128) levels * batch * row;
        if (a1 > top || g1 > top || (a0 < g1 && g0 < a1) || exps_overlap(d_exp, batch, g0, g1)) return NTT_E_ARG;
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    RoctxRange whole("ntt_gadget_decompose_map");
    return (int) ntt::launch_negacyclic_map(pl->field, d_a, d_digits, pl->logn, polys, batch, kind, q, d_exp, flags & NTT_MAP_MINUS_IDENTITY, log_base, levels, low_bits,
                                            (hipStream_t) stream);
} NTT_GUARD_END

int ntt_polymul_gadget_map_pre(ntt_plan_t pl, const void *d_a, size_t polys, int kind, uint32_t param, const uint32_t *d_exp, int flags, int log_base, int levels,
                               int low_bits, void *d_work, const void *d_bhat, size_t bhat_rows, size_t outs, const void *d_addend, void *d_out, size_t batch,
                               void *stream) NTT_GUARD {
    int rc = check_io(pl, d_a, d_bhat, batch);
    if (rc) return rc;
    if (batch && (!d_out || ((uintptr_t) d_out & 15u) || !d_work || ((uintptr_t) d_work & 15u) || ((uintptr_t) d_addend & 15u))) return NTT_E_ARG;
    if (batch && bhat_rows != 1 && bhat_rows != batch) return NTT_E_ARG;
    uint32_t q = 0;
    if (batch && (rc = check_map(pl, kind, param, d_exp, flags, &q))) return rc;
    if (batch && !ntt::gadget_params_ok(pl->p, log_base, levels, low_bits)) return NTT_E_ARG;
    if (batch && (polys == 0 || polys > 0x7FFFFFFFull / batch / (size_t) levels)) return NTT_E_ARG;  // terms * batch rows, terms = polys * levels
    if (batch && (outs == 0 || outs > 0x7FFFFFFFull / batch)) return NTT_E_ARG;                      // the forward passes over outs * batch rows
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (!pl->has_inv) return NTT_E_NOTINVERTIBLE;
    if (batch == 0) return NTT_OK;
    const size_t terms = polys * (size_t) levels;
    {
        const u128 row = table_bytes(pl), top = (u128) 1 << 63;  // no buffer ends beyond that: ranges that cannot wrap
        const u128 lo[4] = {(uintptr_t) d_a, (uintptr_t) d_work, (uintptr_t) d_bhat, (uintptr_t) d_out};
        const u128 hi[4] = {lo[0] + (u128) polys * batch * row, lo[1] + (u128) terms * batch * row, lo[2] + (u128) outs * terms * bhat_rows * row,
                            lo[3] + (u128) outs * batch * row};
        for (int i = 0; i < 4; ++i) {
            if (hi[i] > top) return NTT_E_ARG;
            for (int j = 0; j < i; ++j)
                if (lo[i] < hi[j] && lo[j] < hi[i]) return NTT_E_ARG;  // pairwise disjoint
        }
        // what is only read -- the exponents and the addend -- lies apart from the two written ranges; the addend may be a itself (CMUX)
        if (exps_overlap(d_exp, batch, lo[1], hi[1]) || exps_overlap(d_exp, batch, lo[3], hi[3])) return NTT_E_ARG;
        if (d_addend) {
            const u128 d0 = (uintptr_t) d_addend, d1 = d0 + (u128) outs * batch * row;
            if (d1 > top || (d0 < hi[1] && lo[1] < d1) || (d0 < hi[3] && lo[3] < d1)) return NTT_E_ARG;
        }
    }
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    RoctxRange whole("ntt_polymul_gadget_map_pre");
    const std::vector<PassDesc> &passes = passes_for(pl, batch);  // by batch, as ntt_polymul_matvec_pre selects it
    {
        RoctxRange dec("product(gadget map): map and decomposition");
        rc = (int) ntt::launch_negacyclic_map(pl->field, d_a, d_work, pl->logn, polys, batch, kind, q, d_exp, flags & NTT_MAP_MINUS_IDENTITY, log_base, levels, low_bits, s);
        if (rc) return rc;
    }
    rc = ntt::seq_polymul_matvec(
        *pl, passes, d_work, d_bhat, bhat_rows, terms, outs, d_out, batch,
        [&](const ntt::Step &st) {
            return launch_step(st.family == ntt::STEP_PRODUCT ? (st.args.mv_outs ? "product(gadget map): fused middle, two outputs" : "product(gadget map): fused middle")
                               : st.inverse                   ? "product(gadget map): inv pass"
                                                              : "product(gadget map): fwd pass",
                               st, s);
        },
        [&](void *buf, const void *hat, void *out) {
            RoctxRange sum("product(gadget map): row sums");
            return (int) ntt::launch_matvec_rows(pl->field, buf, hat, out, pl->logn, batch, bhat_rows, terms, outs, ntt::pw_scale_form(*pl, pl->ninv_plain), s);
        });
    if (rc || !d_addend) return rc;
    RoctxRange add("product(gadget map): accumulate");
    return (int) ntt::launch_add_rows(pl->field, d_out, d_addend, (outs * batch) << pl->logn, s);
} NTT_GUARD_END

int ntt_count_noncanonical(ntt_plan_t pl, const void *d_buf, size_t batch, uint64_t *host_count) NTT_GUARD {
    if (!pl || !host_count) return NTT_E_ARG;
    *host_count = 0;
    if (batch == 0) return NTT_OK;
    if (!d_buf) return NTT_E_ARG;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    std::lock_guard<std::mutex> lock(pl->counter_mu);  // the plan's one counter word
    unsigned long long *d_cnt = pl->d_counter;
    hipError_t e = hipMemset(d_cnt, 0, sizeof(*d_cnt));
    if (e == hipSuccess) e = ntt::launch_count_noncanonical(d_buf, batch << pl->logn, pl->word_bytes, pl->p, d_cnt, nullptr);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d_cnt, sizeof(h), hipMemcpyDeviceToHost);
    *host_count = h;
    return (int) e;
} NTT_GUARD_END

int ntt_forward_stages(ntt_plan_t pl, const void *d_in, void *d_out, size_t batch, int stage, void *stream) NTT_GUARD {
    int rc = check_io(pl, d_in, d_out, batch);
    if (rc) return rc;
    if (!pl->has_table) return NTT_E_NOTABLE;
    if (stage < 0 || stage >= pl->logn) return NTT_E_ARG;
    if (batch == 0) return NTT_OK;
    DeviceGuard g(pl->device);
    if (g.err != hipSuccess) return (int) g.err;
    hipStream_t s = (hipStream_t) stream;
    if (d_in != d_out) {
        hipError_t e = hipMemcpyAsync(d_out, d_in, (batch << pl->logn) * pl->word_bytes,
                                      hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int) e;
    }
    for (int st = 0; st <= stage; st++) {
        hipError_t e = ntt::launch_stage(pl->field, d_out, pl->tw_fwd, pl->logn, st, batch, s);
        if (e != hipSuccess) return (int) e;
    }
    return NTT_OK;
} NTT_GUARD_END

}  // extern "C"
