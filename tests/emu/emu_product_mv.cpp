// emu_product_mv.cpp -- host index model of ntt_polymul_matvec_pre: several inner products of ONE operand a with prepared operands -- the
// two-output summed middle pass (pass.h: run_product_mv_pass, phase_pre_mac on pre_addr for both outputs) and the launches around it.
//
// TEST INFRASTRUCTURE, a sibling of emu_product_dot.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++,
// every thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  The launches are the library's own
// sequence (csrc/sequence.h: seq_polymul_matvec): every ordinary pass through the launchers' dispatchers (emu_exec.h: run_step), a
// two-output middle step through the same product_mv_dispatch / product_mv_args_ok / fill_product_args the GPU launcher uses
// (product_kernel.inc: launch_product_mv), a summed middle step (the last output of an odd count, or a unit without a two-output
// kernel) through product_dot_dispatch / product_dot_args_ok as launch_product_dot does, and the row sums of the fallback as a plain
// loop (a grid-stride kernel without an index model of its own: misc_kernels.hip, matvec_rows_kernel).
// The model steps phases thread by thread: it checks every index and every word, and its hazard tracker sees the barrier between the
// two forward units, but a barrier the schedule lacks altogether shows only where waves really run side by side, on the GPU.
//   * as a library (tests/emu_product_mv_lib.py): emu_polymul_matvec() on the caller's buffers, emu_polymul_matvec_sequence() the launch list;
//   * with -DEMU_PRODUCT_MV_MAIN (tests/test_product_mv_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c): a
//     sweep over word classes x every fused unit size, a two-pass and a three-pass size x ragged batches x output counts x term counts x
//     both bhat_rows x every plan alternative on malloc() buffers of EXACTLY terms * batch * N words of a, outs * terms * bhat_rows * N
//     words of b^ and outs * batch * N words of out, each case compared with the oracle pipeline.  The SECOND output's last term of a
//     broadcast with a ragged last polynomial group is the point: it must not reach past that term's single row, where the
//     allocation of b^ ends.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words): the sanitizer test compiles
// one executable per field so that the instrumented builds run in parallel; a call into an absent field returns -100
#ifndef EMU_PRODUCT_MV_FIELDS
#define EMU_PRODUCT_MV_FIELDS 7
#endif

namespace {

// host twin of launch_product_mv<PC> (two == true) and of launch_product_dot<PC> (product_kernel.inc): every workgroup of the
// launcher's grid, the launcher's argument blocks
template <class PC>
int run_product_mv_launch(const ErasedArgs &e, bool two, bool track) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    using W = typename CI::W;
    if (two ? !product_mv_args_ok(e) : !product_dot_args_ok(e)) return -2;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y > 65535u) return -2;
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    emu::EmuProductExec<CI, CF> ex;
    for (uint32_t by = 0; by < g.grid_y; by++)
        for (uint32_t bx = 0; bx < g.grid_x; bx++) {
            ex.bx = bx;
            ex.by = by;
            memset(ex.tile.data(), 0xA5, ex.tile.size() * sizeof(W));
            ex.tr.reset(ex.tile.data(), ex.tile.size(), sizeof(W));
            ex.tr.what = two ? "product pass (two inner products)" : "product pass (inner product)";
            ntt::lds_track() = track ? &ex.tr : nullptr;
            if (two) run_product_mv_pass<CI, CF>(ex, aa, (const W *) e.in2, af, e.in2_broadcast != 0, e.dot_terms, (size_t) e.mv_in2_stride, (size_t) e.mv_out_stride);
            else run_product_dot_pass<CI, CF>(ex, aa, (const W *) e.in2, af, e.in2_broadcast != 0, e.dot_terms);
            ntt::lds_track() = nullptr;
        }
    return 0;
}

template <class F, int K>
int mv_step_of(const Step &st, bool track) {
    int rc = -1;
    if constexpr ((EMU_PRODUCT_MV_FIELDS >> K) & 1) {
        if (st.args.mv_outs != 0) product_mv_dispatch<F>(st.log_m, [&](auto tag) { rc = run_product_mv_launch<typename decltype(tag)::Cfg>(st.args, true, track); });
        else product_dot_dispatch<F>(st.log_m, [&](auto tag) { rc = run_product_mv_launch<typename decltype(tag)::Cfg>(st.args, false, track); });
    } else {
        rc = emu::EMU_ABSENT;
    }
    return rc;
}

// every step of the sequence: the middle steps here, everything else where the other models run it
int step(const Step &st) {
    if (st.family == STEP_PRODUCT && (st.args.dot_terms != 0 || st.args.mv_outs != 0)) {
        if (st.args.field.kind == FK_GL) return mv_step_of<FieldGL, 0>(st, true);
        if (st.args.field.kind == FK_M64) return mv_step_of<FieldM64, 1>(st, true);
        return mv_step_of<FieldM32, 2>(st, true);
    }
    return emu::run_step<emu::field_parts(EMU_PRODUCT_MV_FIELDS, emu::PARTS_PASS, 3)>(st, true, -3);
}

uint64_t get_word(const void *b, int wb, size_t i) { return wb == 4 ? ((const uint32_t *) b)[i] : ((const uint64_t *) b)[i]; }
void put_word(void *b, int wb, size_t i, uint64_t v) {
    if (wb == 4) ((uint32_t *) b)[i] = (uint32_t) v;
    else ((uint64_t *) b)[i] = v;
}
uint64_t addmod(uint64_t x, uint64_t y, uint64_t p) {
    const uint64_t s = x + y;
    return (s < x || s >= p) ? s - p : s;
}

}  // namespace

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_polymul_matvec_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// 0: the call takes the fallback; 1: fused with one summed launch per output; 2: fused with the two-output kernel -- the library's own
// questions (sequence.h: polymul_dot_fused, polymul_matvec_paired); -1 = no such alternative
int emu_polymul_matvec_fused(int word_bytes, int logn, uint64_t p, uint32_t batch, uint32_t target_wgs, int alt) {
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -1;
    PlanFacts pl;
    pl.logn = logn;
    pl.field = field_params(word_bytes, p);
    pl.target_wgs = target_wgs;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    return !polymul_dot_fused(pl, passes, batch) ? 0 : polymul_matvec_paired(pl, passes) ? 2 : 1;
}

// ntt_polymul_matvec_pre as the library sequences it.  T_plain: the size-2^logn table, plain residues; a: [terms][batch][N], overwritten;
// bhat: [outs][terms][bhat_rows][N] (bhat_rows: 1 or batch), never written; out: [outs][batch][N], apart from a.  alt: plan alternative,
// -1 = by batch.  single != 0: one summed launch per output (the experiment build's NTT_MATVEC_SINGLE).
// -1 bad arguments, -3 no kernel for a pass (-2: the launcher refuses its arguments), -4 no such alternative, -5 table not invertible
int emu_polymul_matvec(int word_bytes, int logn, uint64_t p, const void *T_plain, void *a, const void *bhat, uint32_t bhat_rows, uint32_t terms, uint32_t outs, void *out,
                       uint32_t batch, uint32_t target_wgs, int alt, int single) {
    if ((bhat_rows != 1 && bhat_rows != batch) || terms == 0 || outs == 0 || (uint64_t) terms * batch > 0x7FFFFFFFull || (uint64_t) outs * batch > 0x7FFFFFFFull) return -1;
    {
        const size_t row = ((size_t) 1 << logn) * (size_t) word_bytes;
        const uintptr_t a0 = (uintptr_t) a, a1 = a0 + (size_t) terms * batch * row, o0 = (uintptr_t) out, o1 = o0 + (size_t) outs * batch * row;
        if (o0 < a1 && a0 < o1) return -1;  // out overlaps a
    }
    emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, true);
    if (!pl.invertible) return -5;
    pl.mv_single = single;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -4;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    const size_t N = (size_t) 1 << logn;
    return seq_polymul_matvec(pl, passes, a, bhat, bhat_rows, terms, outs, out, batch, step, [&](void *buf, const void *hat, void *dst) {
        for (size_t j = 0; j < outs; j++)
            for (size_t r = 0; r < batch; r++)
                for (size_t i = 0; i < N; i++) {
                    uint64_t acc = 0;
                    for (size_t k = 0; k < terms; k++)
                        acc = addmod(acc, mulmod(get_word(buf, word_bytes, (k * batch + r) * N + i),
                                                 get_word(hat, word_bytes, ((j * terms + k) * bhat_rows + (bhat_rows == 1 ? 0 : r)) * N + i), p), p);
                    put_word(dst, word_bytes, (j * batch + r) * N + i, mulmod(acc, pl.ninv_plain, p));
                }
        return 0;
    });
}

// The launch list of one call: nothing runs, no pointer is followed.  Per step 24 ints: family (0 pass, 2 product middle, 3 = the row sums
// of the fallback), inverse, contig, log_m, n, s0, variant, do_scale, batch, then what each pointer IS -- in, out, tw, tw2, tw_sc, in2
// (0 null, 1 operand a, 2 the output, 3 b^, 4 forward table, 5 inverse table, 6 scaled stage-0 table, -1 anything else; for out and in2
// a pointer INSIDE the output / b^ counts as that buffer) -- a mask (1 in2_prepared, 2 in2_broadcast, 4 pw_scale != 0), dot_terms, the
// two term strides in units of N words, mv_outs, the two output strides in units of N words, and how far out and in2 lie inside
// their buffers, in units of N words.  Returns the number of steps, or -1 when they do not fit `cap` (or there is no such alternative).
int emu_polymul_matvec_sequence(int word_bytes, int logn, uint64_t p, uint32_t batch, uint32_t bhat_rows, uint32_t terms, uint32_t outs, int alt, uint32_t target_wgs,
                                int single, int *steps, int cap) {
    char *ptr[7];  // tokens, far apart; never followed
    for (uintptr_t k = 0; k < 7; k++) ptr[k] = (char *) (k << 44);
    PlanFacts pl;
    pl.logn = logn;
    pl.p = p;
    pl.word_bytes = word_bytes;
    pl.field = field_params(word_bytes, p);
    pl.ninv_plain = powmod(p / 2 + 1, (uint64_t) logn, p);
    pl.tw_fwd = ptr[4];
    pl.tw_inv = ptr[5];
    pl.tw_inv_sc = word_bytes == 8 ? ptr[6] : nullptr;
    pl.target_wgs = pl.target_wgs_col = target_wgs;
    pl.mv_single = single;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -1;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    const uintptr_t row = ((uintptr_t) 1 << logn) * (uintptr_t) word_bytes;
    int count = 0;
    auto id = [&](const void *x) {
        if (x == nullptr) return 0;
        for (int k = 1; k < 7; k++)
            if ((uintptr_t) x >= (uintptr_t) ptr[k] && (uintptr_t) x < (uintptr_t) ptr[k] + ((uintptr_t) 1 << 43)) return (k == 2 || k == 3 || x == ptr[k]) ? k : -1;
        return -1;
    };
    auto off = [&](const void *x, int k) { return (int) (((uintptr_t) x - (uintptr_t) ptr[k]) / row); };
    auto put = [&](const int (&v)[24]) {
        if (count >= cap) return -1;
        memcpy(steps + 24 * count++, v, sizeof(v));
        return 0;
    };
    const int rc = seq_polymul_matvec(
        pl, passes, ptr[1], ptr[3], bhat_rows, terms, outs, ptr[2], batch,
        [&](const Step &st) {
            const ErasedArgs &a = st.args;
            const int v[24] = {st.family, st.inverse, st.contig, st.log_m, a.n, a.s0, a.variant, a.do_scale, (int) a.batch, id(a.in), id(a.out), id(a.tw), id(a.tw2),
                               id(a.tw_sc), id(a.in2), (a.in2_prepared ? 1 : 0) | (a.in2_broadcast ? 2 : 0) | (a.pw_scale ? 4 : 0), a.dot_terms,
                               (int) (a.dot_in_stride >> logn), (int) (a.dot_in2_stride >> logn), a.mv_outs, (int) (a.mv_in2_stride >> logn), (int) (a.mv_out_stride >> logn),
                               id(a.out) == 2 ? off(a.out, 2) : 0, id(a.in2) == 3 ? off(a.in2, 3) : 0};
            return put(v);
        },
        [&](void *buf, const void *hat, void *dst) {
            const int v[24] = {3, 0, 0, 0, logn, 0, 0, 0, (int) batch, id(buf), id(dst), 0, 0, 0, id(hat), bhat_rows != batch ? 2 : 0, (int) terms, (int) batch, (int) bhat_rows,
                               (int) outs, (int) (terms * bhat_rows), (int) batch, 0, 0};
            return put(v);
        });
    return rc ? -1 : count;
}

}  // extern "C"

#if defined(EMU_PRODUCT_MV_MAIN)
#include "emu_sweep.h"

namespace {

using namespace sweep;

// one case on exact-size buffers; returns 0 when every word equals the oracle's and b^ is untouched.  The table is the class's kind-1
// table: the identity Fwd(N^-1 . sum InvU(a_k) . b^_k) holds for any invertible table, and 2N need not divide p - 1
int one_case(const Class &c, int logn, uint32_t batch, uint32_t bhat_rows, uint32_t terms, uint32_t outs, int alt) {
    const size_t N = (size_t) 1 << logn, wb = (size_t) c.wb, rowsA = (size_t) terms * batch, rowsB = (size_t) outs * terms * bhat_rows, rowsO = (size_t) outs * batch;
    void *T = oracle_table(c, N);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *a = malloc(rowsA * N * wb), *bhat = malloc(rowsB * N * wb), *keep = malloc(rowsB * N * wb);
    void *out = malloc(rowsO * N * wb), *want = malloc(rowsO * N * wb), *inv = malloc(rowsA * N * wb);
    if (!a || !bhat || !keep || !out || !want || !inv) abort();
    for (size_t i = 0; i < rowsA * N; i++) put(a, c.wb, i, rnd_residue(c.p));
    for (size_t i = 0; i < rowsB * N; i++) put(bhat, c.wb, i, rnd_residue(c.p));
    memcpy(keep, bhat, rowsB * N * wb);
    // want[j] = Fwd( sum_k Inv(a_k) . b^_jk ): the scaled inverse carries the N^-1
    memcpy(inv, a, rowsA * N * wb);
    int bad = oracle_transform(c, inv, N, rowsA, T, true) != 0;
    for (size_t j = 0; j < outs; j++)
        for (size_t r = 0; r < batch; r++)
            for (size_t i = 0; i < N; i++) {
                uint64_t acc = 0;
                for (size_t k = 0; k < terms; k++)
                    acc = addmod(acc, ntt::host::mulmod(get(inv, c.wb, (k * batch + r) * N + i),
                                                        get(bhat, c.wb, ((j * terms + k) * bhat_rows + (bhat_rows == 1 ? 0 : r)) * N + i), c.p), c.p);
                put(want, c.wb, (j * batch + r) * N + i, acc);
            }
    oracle_transform(c, want, N, rowsO, T, false);
    memset(out, 0xFF, rowsO * N * wb);
    const int rc = emu_polymul_matvec(c.wb, logn, c.p, T, a, bhat, bhat_rows, terms, outs, out, batch, 8, alt, 0);
    bad |= rc != 0 || memcmp(out, want, rowsO * N * wb) != 0 || memcmp(bhat, keep, rowsB * N * wb) != 0;
    if (bad) fprintf(stderr, "MISMATCH %s logn=%d batch=%u bhat_rows=%u terms=%u outs=%u alt=%d rc=%d\n", c.name, logn, batch, bhat_rows, terms, outs, alt, rc);
    free(T);
    free(a);
    free(bhat);
    free(keep);
    free(out);
    free(want);
    free(inv);
    return bad;
}

}  // namespace

// usage: emu_product_mv_sweep <class: gl | m64 | m32> [quick]
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0, point = 0;
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
        // every fused unit size as a single-pass size (launch.h: product_mid_used), the fallback size below it, then one two-pass and
        // one three-pass size (8 + 8 + 7 stages)
        const int lo = c.wb == 4 ? 5 : 6, single_hi = c.wb == 4 ? 13 : 12, two_pass = c.wb == 4 ? 14 : 13, three_pass = 23;
        for (int logn = lo; logn <= three_pass; logn++) {
            if (logn > two_pass && logn < three_pass) continue;
            if (quick && logn > 9) break;
            const int nalt = emu_polymul_matvec_alternatives(c.wb, logn, c.p);
            // ragged batches: odd counts leave the last polynomial group of a many-polynomial workgroup part empty; fewer at the
            // large sizes (the host model steps every lane).  The term count (1, 2, 3, 5) and the output count (2, 3, 2, 4: a pair, a
            // pair and a summed launch, two pairs) are drawn from the sweep's fixed random stream, so every combination with a batch
            // and a bhat_rows turns up; a broadcast ALWAYS has a second output (no 1 among the counts): its last term ends b^.
            const uint32_t all[] = {1, 3, 5, 9, 17, 33}, big[] = {1}, ks[] = {1, 2, 3, 5}, js[] = {2, 3, 2, 4};
            const uint32_t *bs = logn == three_pass ? big : all;
            const int nb = logn == three_pass ? 1 : (logn <= 9 ? 6 : logn <= single_hi ? 4 : 3);
            // THE case of this sweep, counted per size: a broadcast on a ragged batch (odd, > 1) whose middle is the two-output kernel,
            // so that the second output's last term ends the allocation of b^.  Every size at which some alternative pairs must have one.
            long pairing_alts = 0, point_here = 0;
            for (int alt = 0; alt < nalt; alt++)
                for (int bi = 0; bi < nb; bi++)
                    for (int bc = 0; bc < 2; bc++) {
                        if (bc && bs[bi] == 1u) continue;  // the same call
                        const uint32_t terms = logn == three_pass ? 2u : ks[(rnd() >> 8) & 3], outs = logn == three_pass ? 2u : js[(rnd() >> 8) & 3];
                        bad += one_case(c, logn, bs[bi], bc ? 1u : bs[bi], terms, outs, alt);
                        cases++;
                        const bool paired = emu_polymul_matvec_fused(c.wb, logn, c.p, bs[bi], 8, alt) == 2;
                        if (paired && bi == 0 && bc == 0) pairing_alts++;
                        if (paired && bc && (bs[bi] & 1u) && outs >= 2) point_here++;
                    }
            if (pairing_alts > 0 && point_here == 0 && logn != three_pass) {  // (the three-pass size runs one polynomial: nothing ragged)
                fprintf(stderr, "NO paired ragged broadcast case at %s logn=%d\n", c.name, logn);
                bad++;
            }
            point += point_here;
        }
    }
    printf("%s: %ld paired ragged broadcast cases\n", argv[1], point);
    return report(argv[1], cases, bad);
}
#endif
