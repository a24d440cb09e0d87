// emu_lde.cpp -- host index model of ntt_lde's fused first pass (pass.h: PassCfg::LDE, phase_lde_*).
//
// TEST INFRASTRUCTURE, a sibling of emu.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++, every
// thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  The launches are the library's own
// sequence (csrc/sequence.h: seq_lde), every kernel the one the launcher's rule names (csrc/launch.h: pass_dispatch, lde_dispatch
// behind it) with the launcher's argument block.  The fused pass gets `out` as its ordinary input, which it must not read: callers
// fill `out` with words >= p first, so that a read of it cannot produce the oracle's words.
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

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_lde_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// One low-degree extension as ntt_lde runs it from logn = 5 on: fused first pass, then the plain column passes, in place on `out`.
// T_plain: the size-2^logn table, plain residues; in: [batch][2^(logn - beta)]; out: [batch][2^logn]; alt: plan alternative, -1 = by batch.
// -2 / -3: no kernel for the first / a later pass (or the launcher refuses its arguments: -2), -4: no such alternative
int emu_lde(int word_bytes, int logn, uint64_t p, const void *T_plain, int beta, uint64_t shift, const void *in, void *out,
            uint32_t batch, int layout, uint32_t target_wgs, int alt) {
    if (logn < LDE_MIN_LOG_M || beta < 1 || beta > 4 || beta >= logn || shift == 0 || shift >= p) return -1;
    emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, false);
    pl.set_coset(beta, shift);
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -4;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    if (!passes[0].contig || passes[0].s0 != 0) return -1;
    return seq_lde(pl, passes, in, out, batch, layout, [](const Step &st) {
        return emu::run_step<emu::field_parts(EMU_LDE_FIELDS, emu::PARTS_PASS, 1)>(st, true, st.args.s0 == 0 ? -2 : -3);
    });
}

}  // extern "C"

#if defined(EMU_LDE_MAIN)
#include "emu_sweep.h"

namespace {

using namespace sweep;

// one case on exact-size buffers; returns 0 when every word equals the oracle's
int one_case(const Class &c, int logn, int beta, uint32_t batch, int layout, int alt, uint64_t shift) {
    const size_t M = (size_t) 1 << logn, N = M >> beta;
    const size_t wb = (size_t) c.wb;
    void *T = oracle_table(c, M);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *in = malloc((size_t) batch * N * wb), *out = malloc((size_t) batch * M * wb), *want = malloc((size_t) batch * M * wb);
    if (!in || !out || !want) abort();
    memset(want, 0, (size_t) batch * M * wb);
    memset(out, 0xFF, (size_t) batch * M * wb);  // words >= p: the fused pass is handed `out` as its input and must not read it
    for (size_t b = 0; b < batch; b++)
        for (size_t i = 0; i < N; i++) {
            const uint64_t x = rnd_residue(c.p);
            put(in, c.wb, b * N + i, x);
            put(want, c.wb, b * M + (i << beta), mulmod(x, powmod(shift, bitrev(i, logn - beta), c.p), c.p));
        }
    oracle_transform(c, want, M, batch, T, false);
    if (layout) {
        void *tmp = malloc((size_t) batch * M * wb);
        if (!tmp) abort();
        for (size_t b = 0; b < batch; b++) oracle_block16(c, (char *) tmp + b * M * wb, (const char *) want + b * M * wb, M);
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
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
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
    return report(argv[1], cases, bad);
}
#endif
