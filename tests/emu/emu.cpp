// emu.cpp -- host index model of the pass kernels.
//
// TEST INFRASTRUCTURE.  Compiles the very same pass.h / field.h / plan.h the HIP
// kernels are built from with g++ and steps all 256 thread contexts of every
// workgroup phase by phase (the role __syncthreads() plays on the GPU), so the
// index rules, the LDS exchange pattern, the pass planner and the modular
// arithmetic can be checked against the oracle on a machine without a GPU.
// Which passes run, in which order and with which arguments is the library's own
// sequence (csrc/sequence.h), each step through the launchers' dispatchers (emu_exec.h: run_step).
// It is not a CPU fallback: nothing in the product loads this library.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// Which template families this translation unit instantiates (bit set = compiled in; a call into an absent family returns
// EMU_ABSENT).  The ordinary build has them all; tests/test_emu_asan.py compiles one family per sanitizer executable so that
// the instrumented builds run in parallel and finish in about a minute instead of six.
//   0 Goldilocks forward   1 Goldilocks inverse   2 general 64-bit forward   3 general 64-bit inverse
//   4 4-byte forward       5 4-byte inverse       6 / 7 / 8 fused product middle: Goldilocks / general 64-bit / 4-byte
// (emu_exec.h: run_step has the same numbering; no matrix pass runs here)
#ifndef EMU_PARTS
#define EMU_PARTS 0x1FF
#endif
using emu::EMU_ABSENT;
// non-zero: the LDS hazard tracker stays off (emu_set_tracking; the sanitizer sweep checks memory safety, test_emu.py hazards)
static int g_no_track = 0;

namespace {

// every step of a sequence (csrc/sequence.h) goes to the kernel the GPU launcher runs for it, stepped on the host; -1 = no such kernel
int step(const Step &st) { return emu::run_step<(EMU_PARTS) & 0x1FF>(st, !g_no_track, -1); }

}  // namespace

extern "C" {

void emu_set_tracking(int on) { g_no_track = !on; }

// Forward (inverse = 0) or exact inverse (inverse = 1, scaled by N^-1 when scale != 0) of `batch` polynomials as ntt_forward /
// ntt_inverse sequence them (seq_forward / seq_inverse), host buffers, table T in plain form (N words).
// passes_override: 0 = planner's split; otherwise a list "first,col,col,.." packed 4 bits each from the low nibble (used to
// exercise every tile shape); bits 60..63 = PassDesc::variant of the CONTIG pass.  Either is a decomposition of its own
// handed to the same sequence.
int emu_transform(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, void *out,
                  uint32_t batch, int inverse, int layout, int scale, uint32_t target_wgs,
                  uint64_t passes_override) {
    const emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, inverse != 0);
    if (inverse && !pl.invertible) return -5;
    std::vector<PassDesc> passes;
    const int contig_variant = (int) (passes_override >> 60);
    passes_override &= (1ull << 60) - 1;
    if (passes_override == 0) {
        passes = plan_passes(logn, word_bytes);
    } else {
        int s0 = 0;
        for (uint64_t v = passes_override; v; v >>= 4) {
            const int m = (int) (v & 15);
            passes.push_back({passes.empty(), s0, m});
            s0 += m;
        }
        if (s0 != logn) return -1;
    }
    if (contig_variant && passes[0].contig) passes[0].variant = contig_variant;
    if (inverse) return seq_inverse(pl, passes, in, out, batch, layout, scale, step);
    return seq_forward(pl, passes, in, out, batch, layout, nullptr, 1, nullptr, step);
}

// forward transform of (in * in2 * scale): the fused-product first pass (polymul's last leg)
int emu_forward_product(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, const void *in2,
                        void *out, uint32_t batch, uint64_t scale, uint32_t target_wgs) {
    const emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, false);
    return seq_forward(pl, plan_passes(logn, word_bytes), in, out, batch, LAYOUT_NATURAL, in2, scale, nullptr, step);
}

// The negacyclic product c = Fwd(InvU(a) . InvU(b) . N^-1) the way ntt_polymul_negacyclic runs it when the first pass
// has a product kernel (seq_polymul_fused): inverse column passes of both operands, the fused middle pass (pass.h:
// run_product_pass; the whole product for a single-pass size), forward column passes.  T_plain is the kind-2 table; a and b are
// overwritten (scratch), like on the device.
int emu_polymul_fused(int word_bytes, int logn, uint64_t p, const void *T_plain, void *a, void *b, void *out, uint32_t batch,
                      uint32_t target_wgs) {
    const emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, true);
    if (!pl.invertible) return -5;
    const std::vector<PassDesc> passes = plan_passes(logn, word_bytes);
    // unit sizes the product kernels exist for (launch.h: product_dispatch; one more than the library takes, launch.h:
    // product_mid_used), asked before a and b are touched
    if (!with_field(pl.field, [&](auto f) { return product_dispatch<decltype(f)>(passes[0].log_m, [](auto) {}); })) return -1;
    return seq_polymul_fused(pl, passes, a, b, out, batch, step);
}

// The launch list of one call, for tests/test_sequence_cpu.py: nothing runs, no pointer is followed.  call: 0 ntt_forward, 1 ntt_inverse,
// 2 ntt_lde, 3 ntt_coset_inverse, 4 ntt_forward_columns, 5 ntt_inverse_columns, 6 ntt_lde_columns, 7 ntt_coset_inverse_columns,
// 8 / 9 ntt_polymul_negacyclic with separate / contiguous operands.  alt: plan alternative, -1 = by batch.  Per step 16 ints: family,
// inverse, contig, log_m, n, s0, variant, do_scale, batch, then what each pointer IS -- in, out, tw, tw2, tw_sc, in2 (0 null, 1 the
// caller's input / operand a, 2 the output, 3 operand b, 4 forward table, 5 inverse table, 6 scaled stage-0 table, 7 coset vector,
// 8 interpolation vector, -1 anything else) -- and a mask of the coset operands: 1 lde_in = input, 2 lde_s = coset vector (then bits
// 8.. hold lde_beta), 4 cinv_u, 16 / 32 / 64 the same for mat_lde_in, mat_lde_s (bits 8..: mat_lde_beta), mat_cinv_u.  Returns the
// number of steps, or -1 when they do not fit `cap`.
int emu_sequence(int call, int word_bytes, int logn, uint64_t p, uint32_t batch, int alt, int scale, int beta, uint32_t width, int *steps, int cap) {
    const size_t operand_bytes = ((size_t) batch << logn) * (size_t) word_bytes;
    void *ptr[9];  // tokens, far apart; never followed
    for (uintptr_t k = 0; k < 9; k++) ptr[k] = (void *) (k << 44);
    if (call == 9) ptr[3] = (void *) ((uintptr_t) ptr[1] + operand_bytes);
    PlanFacts pl;
    pl.logn = logn;
    pl.p = p;
    pl.word_bytes = word_bytes;
    pl.field = field_params(word_bytes, p);
    pl.tw_fwd = ptr[4];
    pl.tw_inv = ptr[5];
    pl.tw_inv_sc = word_bytes == 8 ? ptr[6] : nullptr;
    pl.lde_s = ptr[7];
    pl.lde_beta = beta;
    pl.cinv_u = ptr[8];
    pl.cinv_set = true;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -1;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    const std::vector<PassDesc> cols = plan_column_passes(logn);
    int count = 0;
    auto id = [&](const void *x) {
        for (int k = 0; k < 9; k++)
            if (x == ptr[k]) return k;
        return -1;
    };
    auto dump = [&](const Step &st) {
        if (count >= cap) return -1;
        const ErasedArgs &a = st.args;
        const int v[16] = {st.family, st.inverse, st.contig, st.log_m, a.n, a.s0, a.variant, a.do_scale, (int) a.batch, id(a.in), id(a.out), id(a.tw), id(a.tw2),
                           id(a.tw_sc), id(a.in2),
                           (a.lde_in == ptr[1]) | (a.lde_s == ptr[7]) << 1 | (a.cinv_u == ptr[8]) << 2 | (a.mat_lde_in == ptr[1]) << 4 | (a.mat_lde_s == ptr[7]) << 5 |
                               (a.mat_cinv_u == ptr[8]) << 6 | (a.lde_beta + a.mat_lde_beta) << 8};
        memcpy(steps + 16 * count++, v, sizeof(v));
        return 0;
    };
    int rc = -1;
    if (call == 0) rc = seq_forward(pl, passes, ptr[1], ptr[2], batch, LAYOUT_NATURAL, nullptr, 1, nullptr, dump);
    if (call == 1) rc = seq_inverse(pl, passes, ptr[1], ptr[2], batch, LAYOUT_NATURAL, scale, dump);
    if (call == 2 && lde_fused(pl)) rc = seq_lde(pl, passes, ptr[1], ptr[2], batch, LAYOUT_NATURAL, dump);
    if (call == 3 && cinv_pass_fused(pl, passes)) rc = seq_coset_inverse(pl, passes, ptr[1], ptr[2], batch, LAYOUT_NATURAL, dump);
    if (call == 4) rc = seq_columns(pl, cols, COL_PLAIN, ptr[1], width, ptr[2], width, width, batch, false, 0, dump);
    if (call == 5) rc = seq_columns(pl, cols, COL_PLAIN, ptr[1], width, ptr[2], width, width, batch, true, scale, dump);
    if (call == 6) rc = seq_columns(pl, cols, COL_LDE, ptr[1], width, ptr[2], width, width, batch, false, 0, dump);
    if (call == 7) rc = seq_columns(pl, cols, COL_CINV, ptr[1], width, ptr[2], width, width, batch, true, 0, dump);
    if ((call == 8 || call == 9) && polymul_fused(pl, passes, batch)) rc = seq_polymul_fused(pl, passes, ptr[1], ptr[3], ptr[2], batch, dump);
    return rc ? -1 : count;
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
