// emu_lde.cpp -- host index model of ntt_lde's fused first pass (pass.h: PassCfg::LDE, phase_lde_*).
//
// TEST INFRASTRUCTURE, a sibling of emu.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++, every
// thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  The first pass is the configuration
// the launcher's own rule names (csrc/launch.h: pass_dispatch, lde_dispatch behind it), with the launcher's argument block, and the
// column passes behind it are the plain ones, so a whole low-degree extension runs here exactly as ntt_lde sequences it.
//   * as a library (tests/emu_lde_lib.py): emu_lde() on the caller's buffers;
//   * with -DEMU_LDE_MAIN (tests/test_lde_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c): a sweep over
//     word classes x logM 5..17 x blow-up 1..4 x ragged batches x both layouts x every plan alternative on malloc() buffers of
//     EXACTLY batch * N input words, batch * M output words and max(N, 4) coset words, each case compared with the oracle's
//     network applied to the expanded input.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words): the sanitizer test compiles
// one executable per field so that the instrumented builds run in parallel; a call into an absent field returns -100
#ifndef EMU_LDE_FIELDS
#define EMU_LDE_FIELDS 7
#endif

namespace {

// the passes of one plan alternative, as ntt_lde sequences them: the first one with the coset operand, the others in place on e.out;
// every kernel is the one the GPU launcher's rule names (csrc/launch.h: pass_dispatch)
template <class F>
int run_lde(ErasedArgs e, const void *in, const void *sv, int beta, const std::vector<PassDesc> &passes) {
    for (const PassDesc &pd : passes) {
        const bool first = &pd == &passes.front();
        if (first && (!pd.contig || pd.s0 != 0)) return -1;
        e.s0 = pd.s0;
        e.in = first ? nullptr : e.out;  // the fused pass must not read `in` at all
        e.lde_in = first ? in : nullptr;
        e.lde_s = first ? sv : nullptr;
        e.lde_beta = first ? beta : 0;
        int rc = first ? -2 : -3;  // no such kernel
        pass_dispatch<F, false>(pd.contig, pd.log_m, e, [&](auto tag) { rc = emu::run_pass_launch<typename decltype(tag)::Cfg>(e, true); });
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_lde_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// One low-degree extension as ntt_lde runs it from logn = 5 on: fused first pass, then the plain column passes, in place on `out`.
// T_plain: the size-2^logn table, plain residues; in: [batch][2^(logn - beta)]; out: [batch][2^logn]; alt: plan alternative, -1 = by batch.
int emu_lde(int word_bytes, int logn, uint64_t p, const void *T_plain, int beta, uint64_t shift, const void *in, void *out,
            uint32_t batch, int layout, uint32_t target_wgs, int alt) {
    if (logn < LDE_MIN_LOG_M || beta < 1 || beta > 4 || beta >= logn || shift == 0 || shift >= p) return -1;
    const size_t M = (size_t) 1 << logn, N = M >> beta;
    const int logN = logn - beta;
    void *tw = malloc(M * (size_t) word_bytes);
    const size_t s_words = N < 4 ? 4 : N;
    void *sv = malloc(s_words * (size_t) word_bytes);
    if (!tw || !sv) abort();
    for (size_t i = 0; i < M; i++) {
        if (word_bytes == 4) ((uint32_t *) tw)[i] = (uint32_t) to_table_form(((const uint32_t *) T_plain)[i], p, 4);
        else ((uint64_t *) tw)[i] = to_table_form(((const uint64_t *) T_plain)[i], p, 8);
    }
    for (size_t i = 0; i < s_words; i++) {  // ntt_plan_set_coset's vector: shift^bitrev_logN(i mod N), periodic up to 4 words
        const uint64_t v = to_table_form(powmod(shift, bitrev(i & (N - 1), logN), p), p, word_bytes);
        if (word_bytes == 4) ((uint32_t *) sv)[i] = (uint32_t) v;
        else ((uint64_t *) sv)[i] = v;
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
#if EMU_LDE_FIELDS & 1
        if (e.field.kind == FK_GL) rc = run_lde<FieldGL>(e, in, sv, beta, passes);
#endif
#if EMU_LDE_FIELDS & 2
        if (e.field.kind == FK_M64) rc = run_lde<FieldM64>(e, in, sv, beta, passes);
#endif
#if EMU_LDE_FIELDS & 4
        if (e.field.kind == FK_M32) rc = run_lde<FieldM32>(e, in, sv, beta, passes);
#endif
    }
    free(tw);
    free(sv);
    return rc;
}

}  // extern "C"

#if defined(EMU_LDE_MAIN)
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
int one_case(const Class &c, int logn, int beta, uint32_t batch, int layout, int alt, uint64_t shift) {
    const size_t M = (size_t) 1 << logn, N = M >> beta;
    const size_t wb = (size_t) c.wb;
    std::vector<uint64_t> T64(M);
    if (oracle_make_table_u64(1, M, T64.data(), c.p, c.g) != 0) return 0;  // 2^logn does not divide p - 1: no such case
    void *T = malloc(M * wb), *in = malloc((size_t) batch * N * wb), *out = malloc((size_t) batch * M * wb), *want = malloc((size_t) batch * M * wb);
    if (!T || !in || !out || !want) abort();
    for (size_t i = 0; i < M; i++) {
        if (c.wb == 4) ((uint32_t *) T)[i] = (uint32_t) T64[i];
        else ((uint64_t *) T)[i] = T64[i];
    }
    memset(want, 0, (size_t) batch * M * wb);
    memset(out, 0xEE, (size_t) batch * M * wb);
    for (size_t b = 0; b < batch; b++)
        for (size_t i = 0; i < N; i++) {
            const uint64_t r = rnd();
            const uint64_t x = (r & 15) == 0 ? 0 : (r & 15) == 1 ? c.p - 1 : (r >> 4) % c.p;  // 0 and p - 1 among the inputs
            const uint64_t sx = mulmod(x, powmod(shift, bitrev(i, logn - beta), c.p), c.p);
            if (c.wb == 4) {
                ((uint32_t *) in)[b * N + i] = (uint32_t) x;
                ((uint32_t *) want)[b * M + (i << beta)] = (uint32_t) sx;
            } else {
                ((uint64_t *) in)[b * N + i] = x;
                ((uint64_t *) want)[b * M + (i << beta)] = sx;
            }
        }
    if (c.wb == 4) oracle_ntt_batch_u32((uint32_t *) want, (uint32_t) M, batch, (const uint32_t *) T, (uint32_t) c.p, 1);
    else oracle_ntt_batch_u64((uint64_t *) want, M, batch, (const uint64_t *) T, c.p, 1);
    if (layout) {
        void *tmp = malloc((size_t) batch * M * wb);
        if (!tmp) abort();
        for (size_t b = 0; b < batch; b++) {
            if (c.wb == 4) oracle_block16_u32((uint32_t *) tmp + b * M, (const uint32_t *) want + b * M, (uint32_t) M);
            else oracle_block16_u64((uint64_t *) tmp + b * M, (const uint64_t *) want + b * M, M);
        }
        free(want);
        want = tmp;
    }
    const int rc = emu_lde(c.wb, logn, c.p, T, beta, shift, in, out, batch, layout, 8192, alt);
    int bad = rc != 0 || memcmp(out, want, (size_t) batch * M * wb) != 0;
    if (bad) fprintf(stderr, "MISMATCH %s logM=%d beta=%d batch=%u layout=%d alt=%d shift=%llu rc=%d\n", c.name, logn, beta, batch, layout, alt, (unsigned long long) shift, rc);
    free(T);
    free(in);
    free(out);
    free(want);
    return bad;
}

}  // namespace

// usage: emu_lde_sweep <class: gl | m64 | m32> [quick]
int main(int argc, char **argv) {
    const Class classes[] = {
        {"gl", 8, GOLDILOCKS, 7},
        {"m64", 8, 0xFFFFFFFC00000001ull, 10},  // general 64-bit class: an NTT prime above 2^63 (sums wrap: the carry paths)
        {"m32", 4, 998244353ull, 3},
    };
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    for (const Class &c0 : classes) {
        if (strcmp(c0.name, argv[1]) != 0) continue;
        const Class &c = c0;
        const int max_logn = quick ? 11 : 17;
        for (int logn = 5; logn <= max_logn; logn++) {
            const int nalt = emu_lde_alternatives(c.wb, logn, c.p);
            for (int beta = 1; beta <= 4 && beta < logn; beta++)
                for (int alt = 0; alt < nalt; alt++)
                    for (int layout = 0; layout < 2; layout++) {
                        // ragged batches: 1, an odd count that leaves the last polynomial group of a many-polynomial workgroup part
                        // empty, and one past a power of two; fewer at the large sizes (the host model steps every lane)
                        const uint32_t batches_small[] = {1, 3, 5, 33, 67}, batches_big[] = {1, 3};
                        const uint32_t *bs = logn <= 11 ? batches_small : batches_big;
                        const int nb = logn <= 11 ? 5 : (logn <= 14 ? 2 : 1);
                        for (int bi = 0; bi < nb; bi++) {
                            const uint64_t shifts[] = {1, c.g, c.p - 1};
                            const uint64_t shift = shifts[(cases + bi) % 3];
                            bad += one_case(c, logn, beta, bs[bi], layout, alt, shift);
                            cases++;
                        }
                    }
        }
    }
    printf("%s: %ld cases, %ld bad\n", argv[1], cases, bad);
    if (bad == 0 && cases > 0) printf("%s: %ld cases clean\n", argv[1], cases);
    return bad ? 1 : (cases ? 0 : 3);
}
#endif
