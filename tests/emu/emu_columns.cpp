// emu_columns.cpp -- host index model of ntt_forward_columns / ntt_inverse_columns (pass.h: PassCfg::MAT, the matrix twin of the
// column pass).
//
// TEST INFRASTRUCTURE, a sibling of emu_lde.cpp / emu_coset_inverse.cpp: the same pass.h / plan.h / field.h the HIP kernels are built
// from, under g++, every thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  Every pass is the
// configuration the launcher's own rule names (csrc/launch.h: mat_twin_dispatch) with the launcher's geometry and argument block
// (pass_geometry_of / fill_pass_args), and the launches are the library's own sequence (csrc/sequence.h: seq_columns over plan.h's
// plan_column_passes).
//   * as a library (tests/emu_columns_lib.py): emu_columns() on the caller's buffers;
//   * with -DEMU_COLUMNS_MAIN (tests/test_columns_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c): the sweep
//     word classes x forward / scaled / unscaled inverse x logn x width x pitch x count x in place / out of place on malloc() buffers of
//     EXACTLY (count * N - 1) * pitch + width words, padding columns pre-filled with a sentinel >= p and asserted unchanged, each
//     live word compared with the oracle's transform of its column.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words); a call into an absent
// field returns -100
#ifndef EMU_COLUMNS_FIELDS
#define EMU_COLUMNS_FIELDS 7
#endif

extern "C" {

// plan.h: plan_column_passes; writes (first stage, stages) pairs, returns the number of passes
int emu_column_passes(int logn, int *s0, int *log_m, int cap) {
    const std::vector<PassDesc> v = plan_column_passes(logn);
    for (size_t i = 0; i < v.size() && (int) i < cap; i++) {
        if (v[i].contig) return -1;
        s0[i] = v[i].s0;
        log_m[i] = v[i].log_m;
    }
    return (int) v.size();
}

// The launch geometry of pass `pass` (an index into plan_column_passes(logn)) of a columns call on this shape, as the launchers form
// it: mat_dispatch names the kernel, pass_geometry_of sizes its grid -- the launch.h code itself, no restatement.  geom: grid_x,
// grid_y, ppw, log_up and the four taper rows.  0, -1 for a bad shape, -2 when there is no such pass or kernel
int emu_columns_geometry(int word_bytes, uint64_t p, int logn, uint32_t width, uint32_t pitch, uint32_t count, uint32_t target_wgs, int pass,
                         int inverse, uint32_t *geom) {
    if (width == 0 || count == 0 || width > pitch) return -1;
    const std::vector<PassDesc> passes = plan_column_passes(logn);
    if (pass < 0 || (size_t) pass >= passes.size()) return -2;
    const int w = mat_log_w(word_bytes, width);
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(word_bytes, p);
    e.n = logn + w;
    e.s0 = passes[pass].s0 + w;
    e.batch = count;
    e.layout = LAYOUT_NATURAL;
    e.target_wgs = target_wgs;
    e.mat_w = w;
    e.mat_pitch = pitch;
    e.mat_width = width;
    int rc = -2;
    auto report = [&](auto tag) {
        const PassGeom g = pass_geometry_of<typename decltype(tag)::Cfg>(e);
        const uint32_t v[8] = {g.grid_x, g.grid_y, (uint32_t) g.ppw, (uint32_t) g.log_up, g.tp.rows[0], g.tp.rows[1], g.tp.rows[2], g.tp.rows[3]};
        memcpy(geom, v, sizeof(v));
        rc = 0;
    };
    with_field(e.field, [&](auto f) {
        using F = decltype(f);
        if (inverse) mat_dispatch<F, true>(passes[pass].log_m, report);
        else mat_dispatch<F, false>(passes[pass].log_m, report);
        return 0;
    });
    return rc;
}

// One matrix transform as ntt_forward_columns / ntt_inverse_columns run it.  T_plain: the size-2^logn table, plain residues; in, out:
// (count * 2^logn - 1) * pitch + width words (out may be in).
int emu_columns(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *in, void *out, uint32_t width, uint32_t pitch,
                uint32_t count, int inverse, int scale, uint32_t target_wgs) {
    if (width == 0 || count == 0) return 0;
    if (width > pitch) return -1;
    const emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, inverse != 0);
    if (inverse && !pl.invertible) return -5;
    const std::vector<PassDesc> passes = plan_column_passes(logn);
    if (passes.empty()) return -3;
    return seq_columns(pl, passes, COL_PLAIN, in, pitch, out, pitch, width, count, inverse != 0, scale, [](const Step &st) {
        return emu::run_step<emu::field_parts(EMU_COLUMNS_FIELDS, emu::PARTS_MAT, 3)>(st, true, -2);
    });
}

// the launcher's refusals (launch.h: fill_pass_args), asked on one shape.  bit 0: a MAT twin without its three arguments; bit 1: the
// arguments on the plain column kernel of that shape; bit 2: the arguments on a CONTIG kernel; bit 3: width > pitch; bit 4: a
// scaled launch on a pass that does not hold stage 0; bit 5: a matrix of more than 2^28 words.  Bit 6 is set when the matching
// pair is NOT accepted, bit 7 when pass_dispatch (an ordinary launch's rule) can be made to name a MAT kernel.  63 = as it should be
int emu_columns_refusals(void) {
    using Twin = ColMatCfg<FieldGL, 6, true>;
    using Plain = ColPassCfg<FieldGL, 6, true>;
    using Contig = ContigCfg<FieldGL, 6, true>;
    ErasedArgs e;
    memset(&e, 0, sizeof(e));
    e.field = field_params(8, GOLDILOCKS);
    e.n = 6 + 5;  // logn 6, w 5
    e.s0 = 5;
    e.batch = 1;
    e.target_wgs = 8192;
    int got = 0;
    PassArgs<Twin> at;
    PassArgs<Plain> ap;
    PassArgs<Contig> ac;
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Plain>(e), at)) got |= 1;
    e.mat_w = 5;
    e.mat_pitch = 40;
    e.mat_width = 20;
    if (!fill_pass_args<Plain>(e, pass_geometry_of<Plain>(e), ap)) got |= 2;
    {
        ErasedArgs c = e;
        c.n = 6;
        c.s0 = 0;
        if (!fill_pass_args<Contig>(c, pass_geometry_of<Contig>(c), ac)) got |= 4;
    }
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at) || at.mat_w != 5 || at.mat_pitch != 40u || at.mat_width != 20u) got |= 64;
    e.do_scale = 1;  // s0 == mat_w: this pass holds stage 0, the sweep is allowed
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at)) got |= 64;
    e.do_scale = 0;
    e.mat_width = 41;
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at)) got |= 8;
    e.mat_width = 20;
    {
        ErasedArgs c = e;
        c.n = 12 + 5;  // stages 6..11 of a 2^12-row matrix
        c.s0 = 6 + 5;
        if (!fill_pass_args<Twin>(c, pass_geometry_of<Twin>(c), at)) got |= 64;
        c.do_scale = 1;
        if (!fill_pass_args<Twin>(c, pass_geometry_of<Twin>(c), at)) got |= 16;
    }
    e.mat_pitch = (1u << 22) + 1u;  // 2^6 rows x (2^22 + 1) words
    if (!fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at)) got |= 32;
    e.mat_pitch = 40;
    bool mat_named = false;
    for (int contig = 0; contig < 2; contig++)
        for (int log_m = 1; log_m <= 14; log_m++)
            pass_dispatch<FieldGL, true>(contig != 0, log_m, e, [&](auto tag) { mat_named |= decltype(tag)::Cfg::MAT; });
    if (mat_named) got |= 128;
    return got;
}

// the size limit from both sides (launch.h: fill_pass_args, MAT_MAX_LOG_WORDS), asked on the first pass of a 2^20-row matrix.  bit 0:
// N * pitch == 2^28 words (pitch 256) is accepted; bit 1: pitch 257 is refused; bit 2: logn + w == 28 (129 columns: w = 8) is accepted;
// bit 3: logn + w == 29 (257 columns in a pitch of 512) is refused.  15 = as it should be
int emu_columns_limit(void) {
    using Twin = ColMatCfg<FieldGL, 7, false>;
    PassArgs<Twin> at;
    auto accepted = [&](int w, uint32_t width, uint32_t pitch) {
        ErasedArgs e;
        memset(&e, 0, sizeof(e));
        e.field = field_params(8, GOLDILOCKS);
        e.n = 20 + w;
        e.s0 = w;
        e.batch = 1;
        e.target_wgs = 16384;
        e.mat_w = w;
        e.mat_pitch = pitch;
        e.mat_width = width;
        return fill_pass_args<Twin>(e, pass_geometry_of<Twin>(e), at);
    };
    int got = 0;
    if (accepted(4, 2, 256)) got |= 1;
    if (!accepted(4, 2, 257)) got |= 2;
    if (accepted(8, 129, 256)) got |= 4;
    if (!accepted(9, 257, 512)) got |= 8;
    return got;
}

}  // extern "C"

#if defined(EMU_COLUMNS_MAIN)
#include "emu_sweep.h"

namespace {

using namespace sweep;

// one case on exact-size buffers; mode 0 forward, 1 scaled inverse, 2 unscaled inverse; returns 0 when every live word equals the
// oracle's and every padding word is untouched
int one_case(const Class &c, int logn, uint32_t width, uint32_t pitch, uint32_t count, int mode, bool in_place, uint32_t target_wgs) {
    const size_t N = (size_t) 1 << logn, wb = (size_t) c.wb;
    const size_t words = ((size_t) count * N - 1) * pitch + width, bytes = words * wb;
    const uint64_t sentinel = c.wb == 4 ? 0xFFFFFFF5ull : 0xFFFFFFFFFFFFFFF5ull;  // >= p for every class
    void *T = oracle_table(c, N);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *in = malloc(bytes), *out = in_place ? in : malloc(bytes), *cols = malloc((size_t) count * width * N * wb);
    if (!in || !out || !cols) abort();
    for (size_t i = 0; i < words; i++) {
        put(in, c.wb, i, sentinel ^ (i & 3));  // padding: non-canonical junk
        if (!in_place) put(out, c.wb, i, sentinel);
    }
    // columns laid out contiguously for the oracle: [count][width][N]
    for (size_t m = 0; m < count; m++)
        for (size_t r = 0; r < N; r++)
            for (size_t k = 0; k < width; k++) {
                const uint64_t x = rnd_residue(c.p);
                put(in, c.wb, (m * N + r) * pitch + k, x);
                put(cols, c.wb, (m * width + k) * N + r, x);
            }
    const size_t nb = (size_t) count * width;
    const int orc = oracle_transform(c, cols, N, nb, T, mode != 0);
    if (mode == 2)  // the oracle's inverse is the scaled one: the unscaled words are N times it
        for (size_t i = 0; i < nb * N; i++) put(cols, c.wb, i, mulmod(get(cols, c.wb, i), (uint64_t) N % c.p, c.p));
    const int rc = emu_columns(c.wb, logn, c.p, T, in, out, width, pitch, count, mode != 0, mode == 1, target_wgs);
    int bad = orc != 0 || rc != 0;
    for (size_t m = 0; m < count && !bad; m++)
        for (size_t r = 0; r < N && !bad; r++)
            for (size_t k = 0; k < pitch && !bad; k++) {
                const size_t i = (m * N + r) * pitch + k;
                if (i >= words) break;
                if (k < width) bad = get(out, c.wb, i) != get(cols, c.wb, (m * width + k) * N + r);
                else bad = get(out, c.wb, i) != (in_place ? (sentinel ^ (i & 3)) : sentinel);
            }
    if (bad) fprintf(stderr, "MISMATCH %s logn=%d width=%u pitch=%u count=%u mode=%d in_place=%d target_wgs=%u rc=%d orc=%d\n", c.name, logn, width, pitch, count, mode, (int) in_place, target_wgs, rc, orc);
    free(T);
    free(in);
    if (!in_place) free(out);
    free(cols);
    return bad;
}

}  // namespace

// usage: emu_columns_sweep <class: gl | m64 | m32> [quick]
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    if (emu_columns_refusals() != 63) {
        fprintf(stderr, "refusals: %d\n", emu_columns_refusals());
        bad++;
    }
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
        const int logns[] = {4, 5, 8, 9, 10, 12};
        const uint32_t widths[] = {1, 3, 16, 17, 33};
        for (int logn : logns) {
            if (quick && logn > 9) continue;
            for (uint32_t width : widths) {
                uint32_t p2 = 1;
                while (p2 < width) p2 *= 2;
                const uint32_t pitches[] = {width, width + 1, p2 + 16};
                for (uint32_t pitch : pitches)
                    for (uint32_t count : {1u, 3u})
                        for (int mode = 0; mode < 3; mode++) {
                            // in place / out of place and ppw 1 / > 1 alternate over the cases; the small sizes run both placements
                            const int reps = logn <= 8 ? 2 : 1;
                            for (int rep = 0; rep < reps; rep++) {
                                const bool in_place = reps == 2 ? rep != 0 : (cases & 1) != 0;
                                bad += one_case(c, logn, width, pitch, count, mode, in_place, (cases & 2) ? 2 : 16384);
                                cases++;
                            }
                        }
            }
        }
        // many matrices per workgroup and several groups per workgroup (ppw > 1) with a ragged last group
        for (int mode = 0; mode < 3; mode++) {
            bad += one_case(c, 4, 5, 7, 3 * 16 + 1, mode, mode == 1, 2);
            cases++;
        }
        // three passes (logn 17 = 6 + 6 + 5): the middle one has several hi blocks, a first stage above mat_w and a row stride above 1
        // at once, and is the only launch that neither reads the caller's input nor holds stage 0
        for (int mode = 0; mode < 3 && !quick; mode++) {
            bad += one_case(c, 17, 17, 18, 1, mode, mode != 1, mode == 2 ? 2 : 16384);
            cases++;
        }
    }
    return report(argv[1], cases, bad);
}
#endif
