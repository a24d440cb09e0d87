// emu_coset_inverse.cpp -- host index model of ntt_coset_inverse's last pass (pass.h: PassCfg::CINV, phase_cinv_scale).
//
// TEST INFRASTRUCTURE, a sibling of emu_lde.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++, every
// thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  Every pass is the configuration the
// launcher's own rule names (csrc/launch.h: pass_dispatch) with the launcher's argument block (fill_pass_args), and the launches are
// the library's own sequence (csrc/sequence.h: seq_coset_inverse): the column passes of the unscaled inverse, then the CONTIG pass
// with the vector operand.
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

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_cinv_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// does the CONTIG pass of alternative `alt` have a twin with the vector sweep: the library's own question (sequence.h: cinv_pass_fused)
int emu_cinv_fused(int word_bytes, int logn, uint64_t p, int alt) {
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt < 0 || alt >= (int) alts.size()) return -1;
    PlanFacts pl;
    pl.logn = logn;
    pl.field = field_params(word_bytes, p);
    return cinv_pass_fused(pl, alts[(size_t) alt].passes) ? 1 : 0;
}

// One coset interpolation as ntt_coset_inverse runs it where it is fused.  T_plain: the size-2^logn table, plain residues; in, out:
// [batch][2^logn] words (out may be in); alt: plan alternative, -1 = by batch.
// -2 / -3: no kernel for the last / an earlier pass (or the launcher refuses its arguments: -2), -4: no such alternative
int emu_coset_inverse(int word_bytes, int logn, uint64_t p, const void *T_plain, uint64_t shift, const void *in, void *out, uint32_t batch,
                      int layout, uint32_t target_wgs, int alt) {
    if (shift == 0 || shift >= p) return -1;
    emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, true);
    if (!pl.invertible || !pl.set_coset_inverse(shift)) return -5;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -4;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    if (!passes[0].contig || passes[0].s0 != 0) return -1;
    return seq_coset_inverse(pl, passes, in, out, batch, layout, [](const Step &st) {
        return emu::run_step<emu::field_parts(EMU_CINV_FIELDS, emu::PARTS_PASS, 2)>(st, true, st.args.s0 == 0 ? -2 : -3);
    });
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
#include "emu_sweep.h"

namespace {

using namespace sweep;

// one case on exact-size buffers; returns 0 when every word equals the oracle's
int one_case(const Class &c, int logn, uint32_t batch, int layout, int alt, uint64_t shift, bool in_place, uint32_t target_wgs) {
    const size_t M = (size_t) 1 << logn;
    const size_t wb = (size_t) c.wb, bytes = (size_t) batch * M * wb;
    void *T = oracle_table(c, M);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *in = malloc(bytes), *out = in_place ? in : malloc(bytes), *want = malloc(bytes);
    if (!in || !out || !want) abort();
    if (!in_place) memset(out, 0xEE, bytes);
    for (size_t i = 0; i < (size_t) batch * M; i++) put(want, c.wb, i, rnd_residue(c.p));
    // the input is the natural-order words in `layout`; the expectation is the oracle's scaled inverse of the natural-order words ...
    for (size_t b = 0; b < batch; b++) {
        if (layout) oracle_block16(c, (char *) in + b * M * wb, (const char *) want + b * M * wb, M);
        else memcpy((char *) in + b * M * wb, (const char *) want + b * M * wb, M * wb);
    }
    const int orc = oracle_transform(c, want, M, batch, T, true);
    // ... times shift^-bitrev(i)
    const uint64_t shift_inv = invmod(shift, c.p);
    for (size_t i = 0; i < M; i++) {
        const uint64_t f = powmod(shift_inv, bitrev(i, logn), c.p);
        for (size_t b = 0; b < batch; b++) put(want, c.wb, b * M + i, mulmod(get(want, c.wb, b * M + i), f, c.p));
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
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
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
    return report(argv[1], cases, bad);
}
#endif
