// emu.cpp -- host index model of the pass kernels.
//
// TEST INFRASTRUCTURE.  Compiles the very same pass.h / field.h / plan.h the HIP
// kernels are built from with g++ and steps all 256 thread contexts of every
// workgroup phase by phase (the role __syncthreads() plays on the GPU), so the
// index rules, the LDS exchange pattern, the pass planner and the modular
// arithmetic can be checked against the oracle on a machine without a GPU.
// It is not a CPU fallback: nothing in the product loads this library.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// Which template families this translation unit instantiates (bit set = compiled in; a call into an absent family returns
// EMU_ABSENT).  The ordinary build has them all; tests/test_emu_asan.py compiles one family per sanitizer executable so that
// the instrumented builds run in parallel and finish in about a minute instead of six.
//   0 Goldilocks forward   1 Goldilocks inverse   2 general 64-bit forward   3 general 64-bit inverse
//   4 4-byte forward       5 4-byte inverse       6 / 7 / 8 fused product middle: Goldilocks / general 64-bit / 4-byte
#ifndef EMU_PARTS
#define EMU_PARTS 0x1FF
#endif
#define EMU_HAS(bit) (((EMU_PARTS) >> (bit)) & 1)
enum { EMU_ABSENT = -100 };
// non-zero: the LDS hazard tracker stays off (emu_set_tracking; the sanitizer sweep checks memory safety, test_emu.py hazards)
static int g_no_track = 0;

namespace {

// the kernel the GPU launcher runs for this pass (csrc/launch.h: pass_dispatch), stepped on the host; -1 = no such kernel
template <class F, bool INV>
int dispatch(bool contig, int log_m, const ErasedArgs &e) {
    int rc = -1;
    pass_dispatch<F, INV>(contig, log_m, e, [&](auto tag) { rc = emu::run_pass_launch<typename decltype(tag)::Cfg>(e, !g_no_track); });
    return rc;
}
template <class F>
int dispatch_product(int log_m, const ErasedArgs &e) {
    int rc = -1;
    product_dispatch<F>(log_m, [&](auto tag) { rc = emu::run_product_launch<typename decltype(tag)::Cfg>(e, !g_no_track); });
    return rc;
}

// the pass of one family (see EMU_PARTS)
int dispatch_family(bool inverse, bool contig, int log_m, const ErasedArgs &e) {
    (void) contig; (void) log_m;
    if (e.field.kind == FK_M64) {
#if EMU_HAS(2)
        if (!inverse) return dispatch<FieldM64, false>(contig, log_m, e);
#endif
#if EMU_HAS(3)
        if (inverse) return dispatch<FieldM64, true>(contig, log_m, e);
#endif
    } else if (e.field.kind == FK_GL) {
#if EMU_HAS(0)
        if (!inverse) return dispatch<FieldGL, false>(contig, log_m, e);
#endif
#if EMU_HAS(1)
        if (inverse) return dispatch<FieldGL, true>(contig, log_m, e);
#endif
    } else {
#if EMU_HAS(4)
        if (!inverse) return dispatch<FieldM32, false>(contig, log_m, e);
#endif
#if EMU_HAS(5)
        if (inverse) return dispatch<FieldM32, true>(contig, log_m, e);
#endif
    }
    return EMU_ABSENT;
}

// the fused product middle of one family
int dispatch_product_family(int log_m, const ErasedArgs &e) {
    (void) log_m;
#if EMU_HAS(7)
    if (e.field.kind == FK_M64) return dispatch_product<FieldM64>(log_m, e);
#endif
#if EMU_HAS(6)
    if (e.field.kind == FK_GL) return dispatch_product<FieldGL>(log_m, e);
#endif
#if EMU_HAS(8)
    if (e.field.kind == FK_M32) return dispatch_product<FieldM32>(log_m, e);
#endif
    return EMU_ABSENT;
}

}  // namespace

extern "C" {

void emu_set_tracking(int on) { g_no_track = !on; }

// Forward (inverse = 0) or exact inverse (inverse = 1, scaled by N^-1 when scale != 0)
// of `batch` polynomials, host buffers, table T in plain form (N words).
// passes_override: 0 = planner's split; otherwise a list "first,col,col,.." packed
// 4 bits each from the low nibble (used to exercise every tile shape); bits 60..63 = PassDesc::variant of the CONTIG pass.
int emu_transform(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, void *out,
                  uint32_t batch, int inverse, int layout, int scale, uint32_t target_wgs,
                  uint64_t passes_override) {
    const size_t N = (size_t) 1 << logn;
    std::vector<uint64_t> T(N), Ti;
    for (size_t i = 0; i < N; i++)
        T[i] = word_bytes == 4 ? ((const uint32_t *) T_plain)[i] : ((const uint64_t *) T_plain)[i];
    if (inverse && !invert_table(T, p, Ti)) return -5;
    const std::vector<uint64_t> &src = inverse ? Ti : T;
    std::vector<uint32_t> t32;
    std::vector<uint64_t> t64;
    const void *tw;
    if (word_bytes == 4) {
        t32.resize(N);
        for (size_t i = 0; i < N; i++) t32[i] = (uint32_t) to_table_form(src[i], p, 4);
        tw = t32.data();
    } else {
        t64.resize(N);
        for (size_t i = 0; i < N; i++) t64[i] = to_table_form(src[i], p, 8);
        tw = t64.data();
    }
    std::vector<uint64_t> tsc;  // stage-0 twiddles of the scaled Goldilocks inverse, as ntt_plan_set_twiddles makes them
    if (inverse && word_bytes == 8) {
        const uint64_t ninv = powmod(p / 2 + 1, (uint64_t) logn, p);
        tsc.resize(N / 2);
        for (size_t i = 0; i < N / 2; i++) tsc[i] = to_table_form(mulmod(Ti[N / 2 + i], ninv, p), p, 8);
    }
    std::vector<PassDesc> passes;
    const int contig_variant = (int) (passes_override >> 60);
    passes_override &= (1ull << 60) - 1;
    if (passes_override == 0) {
        passes = plan_passes(logn, word_bytes);
    } else {
        int s0 = 0;
        bool first = true;
        for (uint64_t v = passes_override; v; v >>= 4) {
            int m = (int) (v & 15);
            passes.push_back({first, s0, m});
            s0 += m;
            first = false;
        }
        if (s0 != logn) return -1;
    }
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(word_bytes, p);
    e.n = logn;
    e.batch = batch;
    e.layout = layout;
    e.target_wgs = target_wgs;
    e.tw = tw;
    e.tw_sc = tsc.empty() ? nullptr : tsc.data();
    e.scale = to_table_form(powmod(p / 2 + 1, (uint64_t) logn, p), p, word_bytes);
    const void *cur = in;
    const size_t np = passes.size();
    for (size_t k = 0; k < np; k++) {
        const size_t i = inverse ? np - 1 - k : k;
        e.in = cur;
        e.out = out;
        e.s0 = passes[i].s0;
        e.variant = passes[i].contig ? (contig_variant ? contig_variant : passes[i].variant) : 0;
        e.do_scale = (inverse && scale && i == 0) ? 1 : 0;
        const int rc = dispatch_family(inverse != 0, passes[i].contig, passes[i].log_m, e);
        if (rc) return rc;
        cur = out;
    }
    return 0;
}

// forward transform of (in * in2 * scale): the fused-product first pass (polymul's last leg)
int emu_forward_product(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, const void *in2,
                        void *out, uint32_t batch, uint64_t scale, uint32_t target_wgs) {
    const size_t N = (size_t) 1 << logn;
    std::vector<uint32_t> t32(N);
    std::vector<uint64_t> t64(N);
    for (size_t i = 0; i < N; i++) {
        const uint64_t t = word_bytes == 4 ? ((const uint32_t *) T_plain)[i] : ((const uint64_t *) T_plain)[i];
        t32[i] = (uint32_t) to_table_form(t, p, 4 == word_bytes ? 4 : 8);
        t64[i] = to_table_form(t, p, 8);
    }
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    // 8-byte words: this entry point has always driven the Goldilocks family whatever p is (its callers pass that prime only)
    e.field = word_bytes == 8 ? FieldParams{FK_GL, p, 0, 0} : field_params(word_bytes, p);
    e.n = logn;
    e.batch = batch;
    e.target_wgs = target_wgs;
    e.tw = word_bytes == 4 ? (const void *) t32.data() : (const void *) t64.data();
    const std::vector<PassDesc> passes = plan_passes(logn, word_bytes);
    const void *cur = in;
    for (size_t i = 0; i < passes.size(); i++) {
        e.in = cur;
        e.out = out;
        e.s0 = passes[i].s0;
        e.in2 = i == 0 ? in2 : nullptr;
        e.pw_scale = to_table_form(to_table_form(scale % p, p, word_bytes), p, word_bytes);
        const int rc = dispatch_family(false, passes[i].contig, passes[i].log_m, e);
        if (rc) return rc;
        cur = out;
    }
    return 0;
}

// The negacyclic product c = Fwd(InvU(a) . InvU(b) . N^-1) the way ntt_polymul_negacyclic runs it when the first pass
// has a product kernel: inverse column passes of both operands, the fused middle pass (pass.h: run_product_pass; the
// whole product for a single-pass size), forward column passes.  T_plain is the kind-2 table; a and b are overwritten
// (scratch), like on the device.
int emu_polymul_fused(int word_bytes, int logn, uint64_t p, const void *T_plain, void *a, void *b, void *out, uint32_t batch,
                      uint32_t target_wgs) {
    const size_t N = (size_t) 1 << logn;
    std::vector<uint64_t> T(N), Ti;
    for (size_t i = 0; i < N; i++) T[i] = word_bytes == 4 ? ((const uint32_t *) T_plain)[i] : ((const uint64_t *) T_plain)[i];
    if (!invert_table(T, p, Ti)) return -5;
    std::vector<uint64_t> tf64(N), ti64(N);
    std::vector<uint32_t> tf32(N), ti32(N);
    for (size_t i = 0; i < N; i++) {
        tf64[i] = to_table_form(T[i], p, word_bytes);
        ti64[i] = to_table_form(Ti[i], p, word_bytes);
        tf32[i] = (uint32_t) tf64[i];
        ti32[i] = (uint32_t) ti64[i];
    }
    const void *tf = word_bytes == 4 ? (const void *) tf32.data() : (const void *) tf64.data();
    const void *ti = word_bytes == 4 ? (const void *) ti32.data() : (const void *) ti64.data();
    const std::vector<PassDesc> passes = plan_passes(logn, word_bytes);
    const int m0 = passes[0].log_m;
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(word_bytes, p);
    // unit sizes the product kernels exist for (launch.h: product_dispatch), asked before a and b are touched
    if (!with_field(e.field, [&](auto f) { return product_dispatch<decltype(f)>(m0, [](auto) {}); })) return -1;
    e.n = logn;
    e.batch = batch;
    e.target_wgs = target_wgs;
    for (size_t i = passes.size(); i-- > 1;)
        for (void *buf : {a, b}) {
            e.in = buf;
            e.out = buf;
            e.tw = ti;
            e.s0 = passes[i].s0;
            const int rc = dispatch_family(true, passes[i].contig, passes[i].log_m, e);
            if (rc) return rc;
        }
    const uint64_t ninv = powmod(p / 2 + 1, (uint64_t) logn, p);
    e.in = a;
    e.in2 = b;
    e.out = out;
    e.tw = ti;
    e.tw2 = tf;
    e.s0 = 0;
    e.pw_scale = to_table_form(to_table_form(ninv, p, word_bytes), p, word_bytes);
    int rc = dispatch_product_family(m0, e);
    e.in2 = nullptr;
    e.pw_scale = 0;
    if (rc) return rc;
    for (size_t i = 1; i < passes.size(); i++) {
        e.in = out;
        e.out = out;
        e.tw = tf;
        e.s0 = passes[i].s0;
        rc = dispatch_family(false, passes[i].contig, passes[i].log_m, e);
        if (rc) return rc;
    }
    return 0;
}

// alternative `alt` of plan_alternatives(logn, word_bytes, p): writes up to 8 (contig, s0, log_m) triples, *min_batch;
// returns the number of passes, or -1 when there is no such alternative
int emu_plan_alt(int logn, int word_bytes, uint64_t p, int alt, int *out_triples, uint64_t *min_batch) {
    auto alts = plan_alternatives(logn, word_bytes, p);
    if (alt < 0 || alt >= (int) alts.size()) return -1;
    const auto &v = alts[(size_t) alt].passes;
    *min_batch = alts[(size_t) alt].min_batch;
    for (size_t i = 0; i < v.size() && i < 8; i++) {
        out_triples[3 * i] = v[i].contig;
        out_triples[3 * i + 1] = v[i].s0;
        out_triples[3 * i + 2] = v[i].log_m;
    }
    return (int) v.size();
}
// kernel variant (PassDesc::variant) of pass `pass` of alternative `alt`, or -1
int emu_plan_alt_variant(int logn, int word_bytes, uint64_t p, int alt, int pass) {
    auto alts = plan_alternatives(logn, word_bytes, p);
    if (alt < 0 || alt >= (int) alts.size() || pass < 0 || pass >= (int) alts[(size_t) alt].passes.size()) return -1;
    return alts[(size_t) alt].passes[(size_t) pass].variant;
}
int emu_select_alt(int logn, int word_bytes, uint64_t p, uint64_t batch) {
    return select_alternative(plan_alternatives(logn, word_bytes, p), batch);
}

// the planner's split, for tests: writes up to 8 (contig, s0, log_m) triples
int emu_plan(int logn, int word_bytes, int *out_triples) {
    auto v = plan_passes(logn, word_bytes);
    for (size_t i = 0; i < v.size() && i < 8; i++) {
        out_triples[3 * i] = v[i].contig;
        out_triples[3 * i + 1] = v[i].s0;
        out_triples[3 * i + 2] = v[i].log_m;
    }
    return (int) v.size();
}

// the launch geometry of one pass, for tests: out = {ppw, grid_x, grid_y, log_up, rows[0..3]}; returns the number of
// polynomial groups that the rule of phase_init() (the Ctx it fills for row by) covers other than exactly once
int emu_geometry(int n, int s0, int log_m, int log_c, int log_u, int contig, uint64_t batch, uint32_t target_wgs, int ppw_cap, uint32_t *out) {
    PassGeom g = pass_geometry(n, s0, log_m, log_c, log_u, contig != 0, batch, target_wgs, ppw_cap);
    out[0] = (uint32_t) g.ppw; out[1] = g.grid_x; out[2] = g.grid_y; out[3] = (uint32_t) g.log_up;
    for (int k = 0; k < 4; k++) out[4 + k] = g.tp.rows[k];
    using Cfg = ContigCfg<FieldM32, 1, false>;  // the row rule does not depend on the configuration
    PassArgs<Cfg> a;
    memset((void *) &a, 0, sizeof(a));
    a.ppw = g.ppw;
    a.tp = g.tp;
    a.n = n;
    const uint64_t groups = (batch + (1ull << g.log_up) - 1) >> g.log_up;
    std::vector<uint8_t> cov(groups, 0);
    for (uint32_t by = 0; by < g.grid_y; by++) {
        Ctx<Cfg> c;
        phase_init<Cfg, false>(c, a, 0, 0, by);
        if (c.ppw < 1) return -1;
        for (int it = 0; it < c.ppw; it++)
            if ((uint64_t) c.pg_base + it < groups && cov[(uint64_t) c.pg_base + it] < 255) cov[(uint64_t) c.pg_base + it]++;
    }
    int bad = 0;
    for (uint64_t i = 0; i < groups; i++) bad += cov[i] != 1;
    return bad;
}

// field arithmetic spot checks
uint64_t emu_gl_mul(uint64_t a, uint64_t b) { return FieldGL{}.mul_plain(a, b); }
uint64_t emu_gl_add(uint64_t a, uint64_t b) { return FieldGL{}.add(a, b); }
uint64_t emu_gl_sub(uint64_t a, uint64_t b) { return FieldGL{}.sub(a, b); }
uint64_t emu_m64_mul_plain(uint64_t a, uint64_t b, uint64_t p) {
    FieldM64 f{p, mont_pinv64(p), mont_r2_64(p)};
    return f.mul_plain(a, b);
}
uint64_t emu_m64_mul(uint64_t x, uint64_t tw, uint64_t p) { return FieldM64{p, mont_pinv64(p), mont_r2_64(p)}.mul(x, tw); }
uint64_t emu_m64_add(uint64_t a, uint64_t b, uint64_t p) { return FieldM64{p, 0, 0}.add(a, b); }
uint64_t emu_m64_sub(uint64_t a, uint64_t b, uint64_t p) { return FieldM64{p, 0, 0}.sub(a, b); }
uint32_t emu_m32_mul_plain(uint32_t a, uint32_t b, uint32_t p) {
    FieldM32 f{p, mont_pinv(p), mont_r2(p)};
    return f.mul_plain(a, b);
}
uint32_t emu_m32_add(uint32_t a, uint32_t b, uint32_t p) { return FieldM32{p, 0, 0}.add(a, b); }
uint32_t emu_m32_sub(uint32_t a, uint32_t b, uint32_t p) { return FieldM32{p, 0, 0}.sub(a, b); }

}  // extern "C"
