// emu_coset_inverse.cpp -- host index model of ntt_coset_inverse's last pass (pass.h: PassCfg::CINV, phase_cinv_scale).
//
// TEST INFRASTRUCTURE, a sibling of emu_lde.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++, every
// thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  Every pass is the configuration the
// launcher's own rule names (csrc/launch.h: pass_dispatch) with the launcher's argument block (fill_pass_args): the column passes
// of the unscaled inverse, then the CONTIG pass with the vector operand, exactly as ntt_coset_inverse sequences them.
//   * as a library (tests/emu_coset_inverse_lib.py): emu_coset_inverse() on the caller's buffers;
//   * with -DEMU_CINV_MAIN (tests/test_coset_inverse_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c): a
//     sweep over word classes x every fused logM x ragged batches x both layouts x every plan alternative on malloc() buffers of
//     EXACTLY batch * M input words, batch * M output words and M vector words, each case compared with the oracle's scaled
//     inverse times shift^-bitrev(i).
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words): the sanitizer test compiles
// one executable per field so that the instrumented builds run in parallel; a call into an absent field returns -100
#ifndef EMU_CINV_FIELDS
#define EMU_CINV_FIELDS 7
#endif

namespace {

// the passes of one plan alternative in the inverse's execution order (descending): the first one launched reads `in`, the others
// run in place on e.out; pass 0 (CONTIG, launched last) carries the vector
template <class F>
int run_cinv(ErasedArgs e, const void *in, const void *u, const std::vector<PassDesc> &passes) {
    if (passes.empty() || !passes[0].contig || passes[0].s0 != 0) return -1;
    const void *cur = in;
    for (size_t k = passes.size(); k-- > 0;) {
        const PassDesc &pd = passes[k];
        e.s0 = pd.s0;
        e.in = cur;
        e.variant = pd.contig ? pd.variant : 0;
        e.cinv_u = k == 0 ? u : nullptr;
        int rc = k == 0 ? -2 : -3;  // no such kernel
        pass_dispatch<F, true>(pd.contig, pd.log_m, e, [&](auto tag) { rc = emu::run_pass_launch<typename decltype(tag)::Cfg>(e, true); });
        if (rc) return rc;
        cur = e.out;
    }
    return 0;
}

}  // namespace

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_cinv_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// does the CONTIG pass of alternative `alt` have a twin with the vector sweep: the launcher's rule, asked without running anything
int emu_cinv_fused(int word_bytes, int logn, uint64_t p, int alt) {
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt < 0 || alt >= (int) alts.size()) return -1;
    const PassDesc &pd = alts[(size_t) alt].passes[0];
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.n = logn;
    e.variant = pd.variant;
    e.cinv_u = &e;  // non-null: only the selection is asked for
    return with_field(field_params(word_bytes, p), [&](auto f) { return pass_dispatch<decltype(f), true>(true, pd.log_m, e, [](auto) {}); }) ? 1 : 0;
}

// One coset interpolation as ntt_coset_inverse runs it where it is fused.  T_plain: the size-2^logn table, plain residues; in, out:
// [batch][2^logn] words (out may be in); alt: plan alternative, -1 = by batch.
int emu_coset_inverse(int word_bytes, int logn, uint64_t p, const void *T_plain, uint64_t shift, const void *in, void *out, uint32_t batch,
                      int layout, uint32_t target_wgs, int alt) {
    if (shift == 0 || shift >= p) return -1;
    const uint64_t shift_inv = invmod(shift, p);
    if (shift_inv == 0) return -5;
    const size_t M = (size_t) 1 << logn;
    std::vector<uint64_t> T(M), Ti;
    for (size_t i = 0; i < M; i++) T[i] = word_bytes == 4 ? ((const uint32_t *) T_plain)[i] : ((const uint64_t *) T_plain)[i];
    if (!invert_table(T, p, Ti)) return -5;
    // exact-size heap buffers: the inverse table and the vector of ntt_plan_set_coset_inverse, u[i] = shift^-bitrev(i) * M^-1, M words
    void *tw = malloc(M * (size_t) word_bytes), *u = malloc(M * (size_t) word_bytes);
    if (!tw || !u) abort();
    const uint64_t minv = powmod(p / 2 + 1, (uint64_t) logn, p);
    for (size_t i = 0; i < M; i++) {
        const uint64_t t = to_table_form(Ti[i], p, word_bytes);
        const uint64_t v = to_table_form(mulmod(powmod(shift_inv, bitrev(i, logn), p), minv, p), p, word_bytes);
        if (word_bytes == 4) ((uint32_t *) tw)[i] = (uint32_t) t, ((uint32_t *) u)[i] = (uint32_t) v;
        else ((uint64_t *) tw)[i] = t, ((uint64_t *) u)[i] = v;
    }
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    const int k = alt >= 0 ? alt : select_alternative(alts, batch);
    int rc = -4;
    if (k < (int) alts.size()) {
        ErasedArgs e;
        memset(&e, 0, sizeof(e));
        e.field = field_params(word_bytes, p);
        e.out = out;
        e.tw = tw;
        e.n = logn;
        e.batch = batch;
        e.layout = layout;
        e.target_wgs = target_wgs;
        const std::vector<PassDesc> &passes = alts[(size_t) k].passes;
        rc = -100;
#if EMU_CINV_FIELDS & 1
        if (e.field.kind == FK_GL) rc = run_cinv<FieldGL>(e, in, u, passes);
#endif
#if EMU_CINV_FIELDS & 2
        if (e.field.kind == FK_M64) rc = run_cinv<FieldM64>(e, in, u, passes);
#endif
#if EMU_CINV_FIELDS & 4
        if (e.field.kind == FK_M32) rc = run_cinv<FieldM32>(e, in, u, passes);
#endif
    }
    free(tw);
    free(u);
    return rc;
}

// the launcher's refusals (launch.h: fill_pass_args), asked on one shape: bit 0 a twin without its vector, bit 1 the vector on the
// plain kernel of that shape, bit 2 a twin on a scaled launch; bit 3 is set when the matching pair is NOT accepted.  7 = as it should be
int emu_cinv_refusals(void) {
    using Twin = ContigCfg<FieldM32, 8, true, true>;
    using Plain = ContigCfg<FieldM32, 8, true>;
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(4, 998244353ull);
    e.n = 8;
    e.batch = 1;
    e.target_wgs = 8192;
    uint32_t dummy[4] = {0, 0, 0, 0};
    int got = 0;
    PassArgs<Twin> at;
    PassArgs<Plain> ap;
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at)) got |= 1;
    e.cinv_u = dummy;
    if (!fill_pass_args<Plain>(e, pass_geometry_of<Plain>(e), ap)) got |= 2;
    e.do_scale = 1;
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at)) got |= 4;
    e.do_scale = 0;
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at) || at.cinv_u != dummy) got |= 8;  // the matching pair is accepted
    return got;
}

}  // extern "C"

#if defined(EMU_CINV_MAIN)
#include "../../oracle/ntt_oracle.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct Class {
    const char *name;
    int wb;
    uint64_t p, g;
};

// one case on exact-size buffers; returns 0 when every word equals the oracle's
int one_case(const Class &c, int logn, uint32_t batch, int layout, int alt, uint64_t shift, bool in_place, uint32_t target_wgs) {
    const size_t M = (size_t) 1 << logn;
    const size_t wb = (size_t) c.wb, bytes = (size_t) batch * M * wb;
    std::vector<uint64_t> T64(M);
    if (oracle_make_table_u64(1, M, T64.data(), c.p, c.g) != 0) return 0;  // 2^logn does not divide p - 1: no such case
    void *T = malloc(M * wb), *in = malloc(bytes), *out = in_place ? in : malloc(bytes), *want = malloc(bytes);
    if (!T || !in || !out || !want) abort();
    for (size_t i = 0; i < M; i++) {
        if (c.wb == 4) ((uint32_t *) T)[i] = (uint32_t) T64[i];
        else ((uint64_t *) T)[i] = T64[i];
    }
    if (!in_place) memset(out, 0xEE, bytes);
    for (size_t i = 0; i < (size_t) batch * M; i++) {
        const uint64_t r = rnd();
        const uint64_t x = (r & 15) == 0 ? 0 : (r & 15) == 1 ? c.p - 1 : (r >> 4) % c.p;  // 0 and p - 1 among the inputs
        if (c.wb == 4) ((uint32_t *) want)[i] = (uint32_t) x;
        else ((uint64_t *) want)[i] = x;
    }
    // the input is the natural-order words in `layout`; the expectation is the oracle's scaled inverse of the natural-order words ...
    for (size_t b = 0; b < batch; b++) {
        if (layout) {
            if (c.wb == 4) oracle_block16_u32((uint32_t *) in + b * M, (const uint32_t *) want + b * M, (uint32_t) M);
            else oracle_block16_u64((uint64_t *) in + b * M, (const uint64_t *) want + b * M, M);
        } else {
            memcpy((char *) in + b * M * wb, (const char *) want + b * M * wb, M * wb);
        }
    }
    int orc;
    if (c.wb == 4) orc = oracle_intt_batch_u32((uint32_t *) want, (uint32_t) M, batch, (const uint32_t *) T, (uint32_t) c.p, 1);
    else orc = oracle_intt_batch_u64((uint64_t *) want, M, batch, (const uint64_t *) T, c.p, 1);
    // ... times shift^-bitrev(i)
    const uint64_t shift_inv = invmod(shift, c.p);
    for (size_t i = 0; i < M; i++) {
        const uint64_t f = powmod(shift_inv, bitrev(i, logn), c.p);
        for (size_t b = 0; b < batch; b++) {
            if (c.wb == 4) ((uint32_t *) want)[b * M + i] = (uint32_t) mulmod(((uint32_t *) want)[b * M + i], f, c.p);
            else ((uint64_t *) want)[b * M + i] = mulmod(((uint64_t *) want)[b * M + i], f, c.p);
        }
    }
    const int rc = emu_coset_inverse(c.wb, logn, c.p, T, shift, in, out, batch, layout, target_wgs, alt);
    const int bad = orc != 0 || rc != 0 || memcmp(out, want, bytes) != 0;
    if (bad) fprintf(stderr, "MISMATCH %s logM=%d batch=%u layout=%d alt=%d shift=%llu in_place=%d target_wgs=%u rc=%d\n", c.name, logn, batch, layout, alt, (unsigned long long) shift, (int) in_place, target_wgs, rc);
    free(T);
    free(in);
    if (!in_place) free(out);
    free(want);
    return bad;
}

}  // namespace

// usage: emu_cinv_sweep <class: gl | m64 | m32> [quick]
int main(int argc, char **argv) {
    const Class classes[] = {
        {"gl", 8, GOLDILOCKS, 7},
        {"m64", 8, 0xFFFFFFFC00000001ull, 10},  // general 64-bit class: an NTT prime above 2^63 (sums wrap: the carry paths)
        {"m32", 4, 998244353ull, 3},
    };
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    for (const Class &c : classes) {
        if (strcmp(c.name, argv[1]) != 0) continue;
        // every size whose plan has a fused last pass, every alternative (so every CONTIG shape: radix-16 5..12, 13, 14 of 4-byte
        // words, radix-8 7..12 as the first pass of a two-pass plan and as variant 1).  target_wgs alternates between the plan's
        // value (ppw = 1 at these batches) and 2 (a workgroup streams several polynomial groups: ppw > 1, ragged last row)
        const int max_logn = quick ? 11 : 17;
        for (int logn = 5; logn <= max_logn; logn++) {
            const int nalt = emu_cinv_alternatives(c.wb, logn, c.p);
            for (int alt = 0; alt < nalt; alt++) {
                if (emu_cinv_fused(c.wb, logn, c.p, alt) != 1) {
                    fprintf(stderr, "%s logM=%d alt=%d: no fused kernel\n", c.name, logn, alt);
                    bad++;
                    continue;
                }
                for (int layout = 0; layout < 2; layout++) {
                    const uint32_t batches[] = {1, 3, 5, 9};
                    const int nb = logn <= 14 ? 4 : 1;  // every CONTIG shape (5..14 stages) at all four batches; the two-pass sizes above at batch 1
                    for (int bi = 0; bi < nb; bi++) {
                        const uint64_t shifts[] = {1, c.g, c.p - 1};
                        bad += one_case(c, logn, batches[bi], layout, alt, shifts[cases % 3], (cases & 1) != 0, (cases & 2) ? 2 : 8192);
                        cases++;
                    }
                }
            }
        }
        // ppw > 1 where a workgroup holds many polynomials (2^(12 - logM) of them): three full groups and one with a single row
        for (int logn = 5; logn <= 11; logn++) {
            bad += one_case(c, logn, (3u << (12 - logn)) + 1, logn & 1, 0, c.g, false, 2);
            cases++;
        }
    }
    printf("%s: %ld cases, %ld bad\n", argv[1], cases, bad);
    if (bad == 0 && cases > 0) printf("%s: %ld cases clean\n", argv[1], cases);
    return bad ? 1 : (cases ? 0 : 3);
}
#endif
