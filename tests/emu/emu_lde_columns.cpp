// emu_lde_columns.cpp -- host index model of ntt_lde_columns / ntt_coset_inverse_columns (pass.h: PassCfg::MLDE / MCINV, the coset
// twins of the matrix column pass).
//
// TEST INFRASTRUCTURE, a sibling of emu_columns.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++,
// every thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  Every pass is the configuration the
// launcher's own rule names (csrc/launch.h: mat_twin_dispatch) with the launcher's geometry and argument block (pass_geometry_of /
// fill_pass_args), and the launches are the library's own sequence (csrc/sequence.h: seq_columns over plan.h's plan_column_passes).
//   * as a library (tests/emu_lde_columns_lib.py): emu_lde_columns() / emu_coset_inverse_columns() on the caller's buffers;
//   * with -DEMU_LDE_COLUMNS_MAIN (tests/test_lde_columns_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c):
//     the sweep word classes x {lde, coset inverse} x logn x beta x width x pitch x count on malloc() buffers of EXACTLY
//     (count * rows - 1) * pitch + width words, padding columns pre-filled with a sentinel >= p and asserted unchanged, each live
//     word compared with the oracle's network on the expanded / scaled column.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words); a call into an absent
// field returns -100
#ifndef EMU_LDE_COLUMNS_FIELDS
#define EMU_LDE_COLUMNS_FIELDS 7
#endif

namespace {

// kind COL_LDE: ntt_lde_columns (forward, the twin in the pass with stage 0 reads the compact source); COL_CINV: ntt_coset_inverse_columns
int run_any(int word_bytes, int logn, uint64_t p, const void *T_plain, ColKind kind, const void *in, uint32_t in_pitch, void *out, uint32_t pitch,
            uint32_t width, uint32_t count, int beta, uint64_t shift, uint32_t target_wgs) {
    if (width == 0 || count == 0) return 0;
    if (width > pitch || width > in_pitch) return -1;
    emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, kind == COL_CINV);
    if (kind == COL_CINV && (!pl.invertible || !pl.set_coset_inverse(shift))) return -5;
    if (kind == COL_LDE) pl.set_coset(beta, shift);
    const std::vector<PassDesc> passes = plan_column_passes(logn);
    if (passes.empty()) return -3;
    return seq_columns(pl, passes, kind, in, in_pitch, out, pitch, width, count, kind == COL_CINV, 0, [](const Step &st) {
        return emu::run_step<emu::field_parts(EMU_LDE_COLUMNS_FIELDS, emu::PARTS_MAT, 3)>(st, true, -2);
    });
}

}  // namespace

extern "C" {

// ntt_lde_columns as the library runs it.  T_plain: the size-2^logn (= M) table, plain residues; in: (count * (M >> beta) - 1) *
// in_pitch + width words; out: (count * M - 1) * out_pitch + width words
int emu_lde_columns(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, uint32_t in_pitch, void *out, uint32_t out_pitch,
                    uint32_t width, uint32_t count, int beta, uint64_t shift, uint32_t target_wgs) {
    if (beta < 1 || beta > 4 || beta >= logn) return -1;
    return run_any(word_bytes, logn, p, T_plain, COL_LDE, in, in_pitch, out, out_pitch, width, count, beta, shift, target_wgs);
}

// ntt_coset_inverse_columns; in, out: (count * M - 1) * pitch + width words (out may be in)
int emu_coset_inverse_columns(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, void *out, uint32_t width, uint32_t pitch,
                              uint32_t count, uint64_t shift, uint32_t target_wgs) {
    return run_any(word_bytes, logn, p, T_plain, COL_CINV, in, pitch, out, pitch, width, count, 0, shift, target_wgs);
}

// The launcher's refusals (launch.h: fill_pass_args), asked on one shape (logn 12, w 5, passes 6 + 6).  A set bit = refused as it
// should be.  bit 0: the LDE twin without its operands; 1: the scaling twin without its vector; 2: the LDE operands on the plain
// matrix twin; 3: the vector on the plain matrix twin; 4: the source pitch alone on the plain matrix twin; 5: the matrix LDE operands on a
// CONTIG LDE kernel (beside its own); 6: the LDE twin on a pass with s0 != mat_w; 7: the scaling twin on such a pass;
// 8: do_scale together with the scaling twin; 9: beta out of range (0 rows left / 5); 10: a source pitch below the width;
// 11: mat_twin_dispatch with both operands; 12: the LDE operands in an inverse launch / the vector in a forward one.
// Bit 13 is set when a matching launch is NOT accepted, bit 14 when mat_dispatch or pass_dispatch can be made to name a twin, or
// mat_twin_dispatch names one without operands.  0x1FFF = as it should be
int emu_lde_columns_refusals(void) {
    using Plain = ColMatCfg<FieldGL, 6, false>;
    using PlainI = ColMatCfg<FieldGL, 6, true>;
    using Lde = ColMatLdeCfg<FieldGL, 6>;
    using Cinv = ColMatCinvCfg<FieldGL, 6>;
    uint64_t dummy[4] = {0, 0, 0, 0};
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(8, GOLDILOCKS);
    e.n = 12 + 5;
    e.s0 = 5;
    e.batch = 1;
    e.target_wgs = 8192;
    e.mat_w = 5;
    e.mat_pitch = 40;
    e.mat_width = 20;
    ErasedArgs l = e, c = e;
    l.mat_lde_in = dummy;
    l.mat_lde_s = dummy;
    l.mat_lde_beta = 2;
    l.mat_src_pitch = 24;
    c.mat_cinv_u = dummy;
    int got = 0;
    PassArgs<Plain> ap;
    PassArgs<PlainI> api;
    PassArgs<Lde> al;
    PassArgs<Cinv> ac;
    if (!fill_pass_args<Lde>(e, pass_geometry_of<Lde>(e), al)) got |= 1;
    if (!fill_pass_args<Cinv>(e, pass_geometry_of<Cinv>(e), ac)) got |= 2;
    if (!fill_pass_args<Plain>(l, pass_geometry_of<Plain>(l), ap)) got |= 4;
    if (!fill_pass_args<PlainI>(c, pass_geometry_of<PlainI>(c), api)) got |= 8;
    {
        ErasedArgs x = e;
        x.mat_src_pitch = 24;
        if (!fill_pass_args<Plain>(x, pass_geometry_of<Plain>(x), ap)) got |= 16;
    }
    {
        ErasedArgs x;
        memset(&x, 0, sizeof(x));
        x.field = e.field;
        x.n = 12;
        x.batch = 1;
        x.target_wgs = 8192;
        x.lde_in = dummy;
        x.lde_s = dummy;
        x.lde_beta = 2;
        x.mat_lde_in = dummy;
        x.mat_lde_s = dummy;
        x.mat_lde_beta = 2;
        x.mat_src_pitch = 24;
        bool refused = true;
        lde_dispatch<FieldGL>(6, false, [&](auto tag) {
            using Cfg = typename decltype(tag)::Cfg;
            PassArgs<Cfg> a;
            refused = !fill_pass_args<Cfg>(x, pass_geometry_of<Cfg>(x), a);
        });
        if (refused) got |= 32;
    }
    {
        ErasedArgs x = l, y = c;
        x.s0 = y.s0 = 6 + 5;  // stages 6..11
        if (!fill_pass_args<Lde>(x, pass_geometry_of<Lde>(x), al)) got |= 64;
        if (!fill_pass_args<Cinv>(y, pass_geometry_of<Cinv>(y), ac)) got |= 128;
    }
    {
        ErasedArgs y = c;
        y.do_scale = 1;
        if (!fill_pass_args<Cinv>(y, pass_geometry_of<Cinv>(y), ac)) got |= 256;
    }
    {
        ErasedArgs x = l, y = l;
        x.mat_lde_beta = 12;
        y.mat_lde_beta = 5;
        if (!fill_pass_args<Lde>(x, pass_geometry_of<Lde>(x), al) && !fill_pass_args<Lde>(y, pass_geometry_of<Lde>(y), al)) got |= 512;
    }
    {
        ErasedArgs x = l;
        x.mat_src_pitch = 19;
        if (!fill_pass_args<Lde>(x, pass_geometry_of<Lde>(x), al)) got |= 1024;
    }
    {
        ErasedArgs x = l;
        x.mat_cinv_u = dummy;
        bool named = false;
        if (!mat_twin_dispatch<FieldGL, false>(6, x, [&](auto) { named = true; }) && !mat_twin_dispatch<FieldGL, true>(6, x, [&](auto) { named = true; }) && !named) got |= 2048;
    }
    {
        bool named = false;
        if (!mat_twin_dispatch<FieldGL, true>(6, l, [&](auto) { named = true; }) && !mat_twin_dispatch<FieldGL, false>(6, c, [&](auto) { named = true; }) && !named) got |= 4096;
    }
    // the matching launches
    if (!fill_pass_args<Lde>(l, pass_geometry_of<Lde>(l), al) || al.lde_in != dummy || al.lde_s != dummy || al.lde_beta != 2 || al.mat_src_pitch != 24u) got |= 8192;
    if (!fill_pass_args<Cinv>(c, pass_geometry_of<Cinv>(c), ac) || ac.cinv_u != dummy) got |= 8192;
    {
        bool is_lde = false, is_cinv = false;
        mat_twin_dispatch<FieldGL, false>(6, l, [&](auto tag) { is_lde = decltype(tag)::Cfg::MLDE; });
        mat_twin_dispatch<FieldGL, true>(6, c, [&](auto tag) { is_cinv = decltype(tag)::Cfg::MCINV; });
        if (!is_lde || !is_cinv) got |= 8192;
    }
    // ordinary launches and the plain columns calls never select a twin
    bool twin_named = false;
    for (int log_m = 1; log_m <= 14; log_m++) {
        mat_dispatch<FieldGL, false>(log_m, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
        mat_dispatch<FieldGL, true>(log_m, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
        mat_twin_dispatch<FieldGL, false>(log_m, e, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
        mat_twin_dispatch<FieldGL, true>(log_m, e, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
        for (int contig = 0; contig < 2; contig++)
            for (const ErasedArgs *x : {&e, &l, &c}) {
                pass_dispatch<FieldGL, false>(contig != 0, log_m, *x, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
                pass_dispatch<FieldGL, true>(contig != 0, log_m, *x, [&](auto tag) { twin_named |= decltype(tag)::Cfg::MLDE || decltype(tag)::Cfg::MCINV; });
            }
    }
    if (twin_named) got |= 16384;
    return got;
}

}  // extern "C"

#if defined(EMU_LDE_COLUMNS_MAIN)
#include "emu_sweep.h"

namespace {

using namespace sweep;

// one case on exact-size buffers; kind 1 lde (beta >= 1, out of place), 2 coset inverse (beta ignored); returns 0 when every live
// word equals the oracle's and every padding word is untouched
int one_case(const Class &c, int logn, int beta, uint32_t width, uint32_t in_pitch, uint32_t pitch, uint32_t count, int kind, bool in_place,
             uint32_t target_wgs, uint64_t shift) {
    const size_t M = (size_t) 1 << logn, wb = (size_t) c.wb, rows_in = kind == 1 ? M >> beta : M;
    const size_t in_words = ((size_t) count * rows_in - 1) * in_pitch + width, out_words = ((size_t) count * M - 1) * pitch + width;
    const uint64_t sentinel = c.wb == 4 ? 0xFFFFFFF5ull : 0xFFFFFFFFFFFFFFF5ull;  // >= p for every class
    void *T = oracle_table(c, M);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *in = malloc(in_words * wb), *out = in_place ? in : malloc(out_words * wb), *cols = malloc((size_t) count * width * M * wb);
    if (!in || !out || !cols) abort();
    for (size_t i = 0; i < in_words; i++) put(in, c.wb, i, sentinel ^ (i & 3));  // padding: non-canonical junk
    if (!in_place)
        for (size_t i = 0; i < out_words; i++) put(out, c.wb, i, sentinel);
    // columns laid out contiguously for the oracle: [count][width][M]; the LDE's are the expanded, scaled ones
    memset(cols, 0, (size_t) count * width * M * wb);
    const int ls = logn - beta;
    for (size_t m = 0; m < count; m++)
        for (size_t r = 0; r < rows_in; r++)
            for (size_t k = 0; k < width; k++) {
                const uint64_t x = rnd_residue(c.p);
                put(in, c.wb, (m * rows_in + r) * in_pitch + k, x);
                if (kind == 1) put(cols, c.wb, (m * width + k) * M + (r << beta), mulmod(x, powmod(shift, bitrev(r, ls), c.p), c.p));
                else put(cols, c.wb, (m * width + k) * M + r, x);
            }
    void *in0 = malloc(in_words * wb);
    if (!in0) abort();
    memcpy(in0, in, in_words * wb);
    const size_t nb = (size_t) count * width;
    const int orc = oracle_transform(c, cols, M, nb, T, kind == 2);
    if (kind == 2) {
        const uint64_t si = powmod(shift, c.p - 2, c.p);
        for (size_t b = 0; b < nb; b++)
            for (size_t r = 0; r < M; r++) put(cols, c.wb, b * M + r, mulmod(get(cols, c.wb, b * M + r), powmod(si, bitrev(r, logn), c.p), c.p));
    }
    const int rc = kind == 1 ? emu_lde_columns(c.wb, logn, c.p, T, in, in_pitch, out, pitch, width, count, beta, shift, target_wgs)
                             : emu_coset_inverse_columns(c.wb, logn, c.p, T, in, out, width, pitch, count, shift, target_wgs);
    int bad = orc != 0 || rc != 0;
    for (size_t m = 0; m < count && !bad; m++)
        for (size_t r = 0; r < M && !bad; r++)
            for (size_t k = 0; k < pitch && !bad; k++) {
                const size_t i = (m * M + r) * pitch + k;
                if (i >= out_words) break;
                if (k < width) bad = get(out, c.wb, i) != get(cols, c.wb, (m * width + k) * M + r);
                else bad = get(out, c.wb, i) != (in_place ? (sentinel ^ (i & 3)) : sentinel);
            }
    if (!in_place && memcmp(in, in0, in_words * wb) != 0) bad = 1;  // the input is read only
    if (bad) fprintf(stderr, "MISMATCH %s kind=%d logn=%d beta=%d width=%u in_pitch=%u pitch=%u count=%u in_place=%d target_wgs=%u rc=%d orc=%d\n", c.name, kind, logn, beta, width, in_pitch, pitch, count, (int) in_place, target_wgs, rc, orc);
    free(T);
    free(in);
    free(in0);
    if (!in_place) free(out);
    free(cols);
    return bad;
}

}  // namespace

// usage: emu_lde_columns_sweep <class: gl | m64 | m32>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    long cases = 0, bad = 0;
    if (emu_lde_columns_refusals() != 0x1FFF) {
        fprintf(stderr, "refusals: %#x\n", emu_lde_columns_refusals());
        bad++;
    }
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
        const uint64_t shifts[] = {1, c.g, c.p - 1};
        const int logns[] = {4, 5, 8, 9, 12};
        const uint32_t widths[] = {1, 3, 16, 17, 33};
        for (int logn : logns)
            for (uint32_t width : widths) {
                uint32_t p2 = 1;
                while (p2 < width) p2 *= 2;
                const uint32_t pitches[] = {width, width + 1, p2 + 16};
                for (int pi = 0; pi < 3; pi++)
                    for (uint32_t count : {1u, 3u}) {
                        // lde: every legal beta, the input pitch is the NEXT choice of the list (always != the output pitch)
                        for (int beta = 1; beta <= 4 && beta < logn; beta++) {
                            bad += one_case(c, logn, beta, width, pitches[(pi + 1) % 3], pitches[pi], count, 1, false, (cases & 2) ? 2 : 16384, shifts[cases % 3]);
                            cases++;
                        }
                        // coset inverse: in place / out of place alternate at the large sizes, both at the small ones
                        const int reps = logn <= 8 ? 2 : 1;
                        for (int rep = 0; rep < reps; rep++) {
                            const bool in_place = reps == 2 ? rep != 0 : (cases & 1) != 0;
                            bad += one_case(c, logn, 0, width, pitches[pi], pitches[pi], count, 2, in_place, (cases & 2) ? 2 : 16384, shifts[cases % 3]);
                            cases++;
                        }
                    }
            }
        // many matrices per workgroup and several groups per workgroup (ppw > 1) with a ragged last group: 49 matrices of 16 rows
        for (int beta = 1; beta <= 3; beta++) {
            bad += one_case(c, 4, beta, 5, 6, 7, 3 * 16 + 1, 1, false, 2, c.g);
            cases++;
        }
        for (int rep = 0; rep < 2; rep++) {
            bad += one_case(c, 4, 0, 5, 7, 7, 3 * 16 + 1, 2, rep != 0, 2, c.g);
            cases++;
        }
        // three passes (logn 17 = 6 + 6 + 5): a plain in-place matrix pass between the fused twin and the other end
        bad += one_case(c, 17, 1, 17, 17, 18, 1, 1, false, 16384, c.p - 1);
        bad += one_case(c, 17, 4, 17, 18, 17, 1, 1, false, 2, c.g);
        bad += one_case(c, 17, 0, 17, 18, 18, 1, 2, true, 16384, c.g);
        cases += 3;
    }
    return report(argv[1], cases, bad);
}
#endif
