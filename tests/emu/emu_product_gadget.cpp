// emu_product_gadget.cpp -- host index model of ntt_polymul_gadget_pre: the prepared products of the balanced gadget digits of a, with
// the decomposition inside the summed middle passes (pass.h: run_product_dot_pass / run_product_mv_pass with GAD = true, gadget_digit
// between the load and the first inverse round) and the launches around them.
//
// TEST INFRASTRUCTURE, a sibling of emu_product_mv.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++,
// every thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  The launches are the library's own
// sequence (csrc/sequence.h: seq_polymul_gadget): a digit step through the same product_gadget_dispatch / product_gadget_args_ok /
// fill_product_args the GPU launcher uses (product_kernel.inc: launch_product_gad), the summed and two-output steps of the unfused path
// as emu_product_mv.cpp runs them, every ordinary pass through the launchers' dispatchers (emu_exec.h: run_step), and the two
// grid-stride kernels without an index model of their own as plain loops: the row sums (misc_kernels.hip: matvec_rows_kernel) and the
// decomposition kernel (gadget_decompose_kernel; the loop calls the kernel's own gadget_digit).
//   * as a library (tests/emu_product_gadget_lib.py): emu_polymul_gadget() on the caller's buffers, emu_polymul_gadget_sequence() the
//     launch list, emu_gadget_digits() the decomposition alone, emu_gadget_params_ok() the argument rule;
//   * with -DEMU_PRODUCT_GADGET_MAIN (tests/test_product_gadget_emu_asan.py, built with ASan + UBSan and linked with
//     oracle/ntt_oracle.c): a sweep over word classes x the size below the smallest unit, every fused unit size and a two-pass size x
//     ragged batches x polynomial counts x digit parameter sets x output counts x both bhat_rows x every plan alternative on malloc()
//     buffers of EXACTLY polys * batch * N words of a, polys * levels * batch * N words of work, outs * polys * levels * bhat_rows * N
//     words of b^ and outs * batch * N words of out; each case compared with the oracle pipeline on digits computed from the
//     definition in 128-bit integers, and a compared with its copy.  The last polynomial's last unit of a ends exactly where the
//     allocation ends; a broadcast on a ragged batch through the two-output digit kernel ends the allocation of b^.
#include "emu_exec.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words): the sanitizer test compiles
// one executable per field so that the instrumented builds run in parallel; a call into an absent field returns -100
#ifndef EMU_PRODUCT_GADGET_FIELDS
#define EMU_PRODUCT_GADGET_FIELDS 7
#endif

namespace {

// host twin of launch_product_gad<PC> (kind 2), launch_product_mv<PC> (1) and launch_product_dot<PC> (0) (product_kernel.inc): every
// workgroup of the launcher's grid, the launcher's argument blocks
template <class PC>
int run_gadget_launch(const ErasedArgs &e, int kind, bool track) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    using F = typename CI::F;
    using W = typename CI::W;
    if (kind == 2 ? !product_gadget_args_ok(e) : kind == 1 ? !product_mv_args_ok(e) : !product_dot_args_ok(e)) return -2;
    const bool two = e.mv_outs != 0;
    if (two && !product_mv_unit<F>(CI::LOG_M)) return -2;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y > 65535u) return -2;
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    const GadgetParams gp{e.gad_log_base, e.gad_levels, e.gad_low_bits};
    emu::EmuProductExec<CI, CF> ex;
    for (uint32_t by = 0; by < g.grid_y; by++)
        for (uint32_t bx = 0; bx < g.grid_x; bx++) {
            ex.bx = bx;
            ex.by = by;
            memset(ex.tile.data(), 0xA5, ex.tile.size() * sizeof(W));
            ex.tr.reset(ex.tile.data(), ex.tile.size(), sizeof(W));
            ex.tr.what = kind == 2 ? "product pass (gadget digits)" : "product pass (inner products)";
            ntt::lds_track() = track ? &ex.tr : nullptr;
            const W *bhat = (const W *) e.in2;
            const bool bc = e.in2_broadcast != 0;
            if (kind == 2 && two)
                run_product_mv_pass<CI, CF, emu::EmuProductExec<CI, CF>, -1, true>(ex, aa, bhat, af, bc, e.dot_terms, (size_t) e.mv_in2_stride, (size_t) e.mv_out_stride, gp);
            else if (kind == 2) run_product_dot_pass<CI, CF, emu::EmuProductExec<CI, CF>, -1, true>(ex, aa, bhat, af, bc, e.dot_terms, gp);
            else if (two) run_product_mv_pass<CI, CF>(ex, aa, bhat, af, bc, e.dot_terms, (size_t) e.mv_in2_stride, (size_t) e.mv_out_stride);
            else run_product_dot_pass<CI, CF>(ex, aa, bhat, af, bc, e.dot_terms);
            ntt::lds_track() = nullptr;
        }
    return 0;
}

template <class F, int K>
int gadget_step_of(const Step &st, bool track) {
    int rc = -1;
    if constexpr ((EMU_PRODUCT_GADGET_FIELDS >> K) & 1) {
        if (!product_no_digits(st.args)) product_gadget_dispatch<F>(st.log_m, [&](auto tag) { rc = run_gadget_launch<typename decltype(tag)::Cfg>(st.args, 2, track); });
        else if (st.args.mv_outs != 0) product_mv_dispatch<F>(st.log_m, [&](auto tag) { rc = run_gadget_launch<typename decltype(tag)::Cfg>(st.args, 1, track); });
        else product_dot_dispatch<F>(st.log_m, [&](auto tag) { rc = run_gadget_launch<typename decltype(tag)::Cfg>(st.args, 0, track); });
    } else {
        rc = emu::EMU_ABSENT;
    }
    return rc;
}

// every step of the sequence: the middle steps here, everything else where the other models run it
int step(const Step &st) {
    if (st.family == STEP_PRODUCT && (st.args.dot_terms != 0 || st.args.mv_outs != 0 || !product_no_digits(st.args))) {
        if (st.args.field.kind == FK_GL) return gadget_step_of<FieldGL, 0>(st, true);
        if (st.args.field.kind == FK_M64) return gadget_step_of<FieldM64, 1>(st, true);
        return gadget_step_of<FieldM32, 2>(st, true);
    }
    return emu::run_step<emu::field_parts(EMU_PRODUCT_GADGET_FIELDS, emu::PARTS_PASS, 3)>(st, true, -3);
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

// gadget_decompose_kernel as a loop: digits[q][k][i] = digit_k(a[q][i]), i < block = batch * N
void decompose(int wb, uint64_t p, const void *a, size_t polys, size_t block, int w, int K, int l, void *digits) {
    const GadgetConsts g = gadget_consts(p, GadgetParams{w, K, l});
    for (size_t q = 0; q < polys; q++)
        for (size_t i = 0; i < block; i++)
            for (int k = 0; k < K; k++) put_word(digits, wb, (q * (size_t) K + (size_t) k) * block + i, gadget_digit(g, get_word(a, wb, q * block + i), k * w, k == K - 1));
}

PlanFacts token_plan(int word_bytes, int logn, uint64_t p, uint32_t target_wgs) {
    PlanFacts pl;
    pl.logn = logn;
    pl.p = p;
    pl.word_bytes = word_bytes;
    pl.field = field_params(word_bytes, p);
    pl.target_wgs = pl.target_wgs_col = target_wgs;
    return pl;
}

}  // namespace

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_polymul_gadget_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// the argument rule of the decomposition (pass.h: gadget_params_ok), as the C-ABI asks it
int emu_gadget_params_ok(uint64_t p, int log_base, int levels, int low_bits) { return gadget_params_ok(p, log_base, levels, low_bits) ? 1 : 0; }

// ntt_gadget_decompose: a [polys][block] words -> digits [polys][levels][block] words, block = batch * N.  -1: the argument rule
int emu_gadget_digits(int word_bytes, uint64_t p, const void *a, uint64_t polys, uint64_t block, int log_base, int levels, int low_bits, void *digits) {
    if (!gadget_params_ok(p, log_base, levels, low_bits)) return -1;
    decompose(word_bytes, p, a, polys, block, log_base, levels, low_bits, digits);
    return 0;
}

// 0: the call runs the decomposition kernel and the unfused digits' product; 1: digit launches, one summed launch per output; 2: digit
// launches through the two-output kernel -- the library's own questions (sequence.h: polymul_gadget_fused, polymul_matvec_paired);
// -1 = no such alternative
int emu_polymul_gadget_fused(int word_bytes, int logn, uint64_t p, uint32_t batch, uint32_t target_wgs, int alt, int unfused) {
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -1;
    PlanFacts pl = token_plan(word_bytes, logn, p, target_wgs);
    pl.gadget_unfused = unfused;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    return !polymul_gadget_fused(pl, passes, batch) ? 0 : polymul_matvec_paired(pl, passes) ? 2 : 1;
}

// ntt_polymul_gadget_pre as the library sequences it.  T_plain: the size-2^logn table, plain residues; a: [polys][batch][N], const;
// work: polys * levels * batch * N words; bhat: [outs][polys * levels][bhat_rows][N] (bhat_rows: 1 or batch), never written; out:
// [outs][batch][N].  alt: plan alternative, -1 = by batch.  unfused != 0: the experiment build's NTT_GADGET_UNFUSED; single != 0: its
// NTT_MATVEC_SINGLE.
// -1 bad arguments, -3 no kernel for a pass (-2: the launcher refuses its arguments), -4 no such alternative, -5 table not invertible
int emu_polymul_gadget(int word_bytes, int logn, uint64_t p, const void *T_plain, const void *a, uint32_t polys, int log_base, int levels, int low_bits, void *work,
                       const void *bhat, uint32_t bhat_rows, uint32_t outs, void *out, uint32_t batch, uint32_t target_wgs, int alt, int unfused, int single) {
    if (!a || !work || !bhat || !out || !gadget_params_ok(p, log_base, levels, low_bits)) return -1;
    if ((bhat_rows != 1 && bhat_rows != batch) || polys == 0 || outs == 0 || (uint64_t) polys * (uint64_t) levels * batch > 0x7FFFFFFFull ||
        (uint64_t) outs * batch > 0x7FFFFFFFull)
        return -1;
    const size_t N = (size_t) 1 << logn, terms = (size_t) polys * (size_t) levels;
    {
        const size_t row = N * (size_t) word_bytes;
        const uintptr_t lo[4] = {(uintptr_t) a, (uintptr_t) work, (uintptr_t) bhat, (uintptr_t) out};
        const uintptr_t hi[4] = {lo[0] + (size_t) polys * batch * row, lo[1] + terms * batch * row, lo[2] + (size_t) outs * terms * bhat_rows * row, lo[3] + (size_t) outs * batch * row};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < i; j++)
                if (lo[i] < hi[j] && lo[j] < hi[i]) return -1;  // pairwise disjoint
    }
    emu::HostPlan pl(word_bytes, logn, p, T_plain, target_wgs, true);
    if (!pl.invertible) return -5;
    pl.gadget_unfused = unfused;
    pl.mv_single = single;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -4;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    return seq_polymul_gadget(
        pl, passes, a, polys, log_base, levels, low_bits, work, bhat, bhat_rows, outs, out, batch, step,
        [&](void *buf, const void *hat, void *dst) {
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
        },
        [&](const void *src, void *digits) {
            decompose(word_bytes, p, src, polys, (size_t) batch * N, log_base, levels, low_bits, digits);
            return 0;
        });
}

// The launch list of one call: nothing runs, no pointer is followed.  Per step 28 ints: the 24 of emu_polymul_matvec_sequence -- family
// (0 pass, 2 product middle, 3 = the row sums of the fallback, 4 = the decomposition kernel), inverse, contig, log_m, n, s0, variant,
// do_scale, batch, then what each pointer IS -- in, out, tw, tw2, tw_sc, in2 (0 null, 1 operand a, 2 the output, 3 b^, 4 forward table,
// 5 inverse table, 6 scaled stage-0 table, 7 work, -1 anything else; for out and in2 a pointer INSIDE the output / b^ counts as that
// buffer) -- a mask (1 in2_prepared, 2 in2_broadcast, 4 pw_scale != 0), dot_terms, the two term strides in units of N words, mv_outs, the
// two output strides in units of N words, how far out and in2 lie inside their buffers in units of N words -- then gad_log_base,
// gad_levels, gad_low_bits and 0.  Returns the number of steps, or -1 when they do not fit `cap` (or there is no such alternative).
int emu_polymul_gadget_sequence(int word_bytes, int logn, uint64_t p, uint32_t batch, uint32_t bhat_rows, uint32_t polys, int log_base, int levels, int low_bits,
                                uint32_t outs, int alt, uint32_t target_wgs, int unfused, int single, int *steps, int cap) {
    char *ptr[8];  // tokens, far apart; never followed
    for (uintptr_t k = 0; k < 8; k++) ptr[k] = (char *) (k << 44);
    PlanFacts pl = token_plan(word_bytes, logn, p, target_wgs);
    pl.ninv_plain = powmod(p / 2 + 1, (uint64_t) logn, p);
    pl.tw_fwd = ptr[4];
    pl.tw_inv = ptr[5];
    pl.tw_inv_sc = word_bytes == 8 ? ptr[6] : nullptr;
    pl.gadget_unfused = unfused;
    pl.mv_single = single;
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    if (alt >= (int) alts.size()) return -1;
    const std::vector<PassDesc> &passes = passes_for(alts, alt, batch);
    const uintptr_t row = ((uintptr_t) 1 << logn) * (uintptr_t) word_bytes;
    const size_t terms = (size_t) polys * (size_t) levels;
    int count = 0;
    auto id = [&](const void *x) {
        if (x == nullptr) return 0;
        for (int k = 1; k < 8; k++)
            if ((uintptr_t) x >= (uintptr_t) ptr[k] && (uintptr_t) x < (uintptr_t) ptr[k] + ((uintptr_t) 1 << 43)) return (k == 2 || k == 3 || x == ptr[k]) ? k : -1;
        return -1;
    };
    auto off = [&](const void *x, int k) { return (int) (((uintptr_t) x - (uintptr_t) ptr[k]) / row); };
    auto put = [&](const int (&v)[28]) {
        if (count >= cap) return -1;
        memcpy(steps + 28 * count++, v, sizeof(v));
        return 0;
    };
    const int rc = seq_polymul_gadget(
        pl, passes, ptr[1], polys, log_base, levels, low_bits, ptr[7], ptr[3], bhat_rows, outs, ptr[2], batch,
        [&](const Step &st) {
            const ErasedArgs &a = st.args;
            const int v[28] = {st.family, st.inverse, st.contig, st.log_m, a.n, a.s0, a.variant, a.do_scale, (int) a.batch, id(a.in), id(a.out), id(a.tw), id(a.tw2),
                               id(a.tw_sc), id(a.in2), (a.in2_prepared ? 1 : 0) | (a.in2_broadcast ? 2 : 0) | (a.pw_scale ? 4 : 0), a.dot_terms,
                               (int) (a.dot_in_stride >> logn), (int) (a.dot_in2_stride >> logn), a.mv_outs, (int) (a.mv_in2_stride >> logn), (int) (a.mv_out_stride >> logn),
                               id(a.out) == 2 ? off(a.out, 2) : 0, id(a.in2) == 3 ? off(a.in2, 3) : 0, a.gad_log_base, a.gad_levels, a.gad_low_bits, 0};
            return put(v);
        },
        [&](void *buf, const void *hat, void *dst) {
            const int v[28] = {3, 0, 0, 0, logn, 0, 0, 0, (int) batch, id(buf), id(dst), 0, 0, 0, id(hat), bhat_rows != batch ? 2 : 0, (int) terms, (int) batch, (int) bhat_rows,
                               (int) outs, (int) (terms * bhat_rows), (int) batch, 0, 0, 0, 0, 0, 0};
            return put(v);
        },
        [&](const void *src, void *digits) {
            const int v[28] = {4, 0, 0, 0, logn, 0, 0, 0, (int) batch, id(src), id(digits), 0, 0, 0, 0, 0, (int) terms, (int) batch, 0, 0, 0, 0, 0, 0, log_base, levels, low_bits, 0};
            return put(v);
        });
    return rc ? -1 : count;
}

}  // extern "C"

#if defined(EMU_PRODUCT_GADGET_MAIN)
#include "emu_sweep.h"

namespace {

using namespace sweep;

// digit_k(a) from the definition of include/ntt_hip.h in 128-bit signed integers: nothing here can wrap, and nothing is shared with
// pass.h's gadget_digit
uint64_t ref_digit(uint64_t a, uint64_t p, int w, int K, int l, int k) {
    using i128 = __int128;
    const bool neg = a > (p - 1) / 2;
    const i128 m = neg ? (i128) p - (i128) a : (i128) a;
    const i128 h = l > 0 ? (i128) 1 << (l - 1) : 0;
    const i128 u = (m + h) >> l;
    i128 v = u;
    for (int j = 0; j + 1 < K; j++) v += (i128) 1 << (j * w + w - 1);
    const i128 B = (i128) 1 << w;
    i128 e = k < K - 1 ? ((v >> (k * w)) & (B - 1)) - B / 2 : v >> ((K - 1) * w);
    if (neg) e = -e;
    e %= (i128) p;
    if (e < 0) e += (i128) p;
    return (uint64_t) e;
}

struct Digits {
    int w, K, l;
};

// one case on exact-size buffers; returns 0 when every word equals the oracle's and neither a nor b^ is written.  The table is the
// class's kind-1 table: the identity Fwd(N^-1 . sum InvU(d_t) . b^_t) holds for any invertible table, and 2N need not divide p - 1
int one_case(const Class &c, int logn, uint32_t batch, uint32_t bhat_rows, uint32_t polys, const Digits &d, uint32_t outs, int alt) {
    const size_t N = (size_t) 1 << logn, wb = (size_t) c.wb, terms = (size_t) polys * (size_t) d.K;
    const size_t rowsA = (size_t) polys * batch, rowsD = terms * batch, rowsB = (size_t) outs * terms * bhat_rows, rowsO = (size_t) outs * batch;
    void *T = oracle_table(c, N);
    if (!T) return 0;  // 2^logn does not divide p - 1: no such case
    void *a = malloc(rowsA * N * wb), *keep_a = malloc(rowsA * N * wb), *work = malloc(rowsD * N * wb), *bhat = malloc(rowsB * N * wb), *keep = malloc(rowsB * N * wb);
    void *out = malloc(rowsO * N * wb), *want = malloc(rowsO * N * wb), *inv = malloc(rowsD * N * wb);
    if (!a || !keep_a || !work || !bhat || !keep || !out || !want || !inv) abort();
    for (size_t i = 0; i < rowsA * N; i++) put(a, c.wb, i, rnd_residue(c.p));
    // words around p / 2 and around the rounding point in the first row
    const uint64_t edge[] = {(c.p - 1) / 2, (c.p - 1) / 2 + 1, d.l > 0 ? ((uint64_t) 1 << (d.l - 1)) % c.p : 1, d.l > 0 ? (((uint64_t) 1 << (d.l - 1)) - 1) % c.p : 2};
    for (size_t i = 0; i < 4 && i < N; i++) put(a, c.wb, i, edge[i]);
    for (size_t i = 0; i < rowsB * N; i++) put(bhat, c.wb, i, rnd_residue(c.p));
    memcpy(keep_a, a, rowsA * N * wb);
    memcpy(keep, bhat, rowsB * N * wb);
    memset(work, 0xEE, rowsD * N * wb);
    // want[j] = Fwd( sum_t Inv(digit_t) . b^_jt ): the scaled inverse carries the N^-1
    for (size_t q = 0; q < polys; q++)
        for (int k = 0; k < d.K; k++)
            for (size_t i = 0; i < (size_t) batch * N; i++)
                put(inv, c.wb, (q * (size_t) d.K + (size_t) k) * batch * N + i, ref_digit(get(a, c.wb, q * batch * N + i), c.p, d.w, d.K, d.l, k));
    int bad = oracle_transform(c, inv, N, rowsD, T, true) != 0;
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
    const int rc = emu_polymul_gadget(c.wb, logn, c.p, T, a, polys, d.w, d.K, d.l, work, bhat, bhat_rows, outs, out, batch, 8, alt, 0, 0);
    bad |= rc != 0 || memcmp(out, want, rowsO * N * wb) != 0 || memcmp(bhat, keep, rowsB * N * wb) != 0 || memcmp(a, keep_a, rowsA * N * wb) != 0;
    if (bad)
        fprintf(stderr, "MISMATCH %s logn=%d batch=%u bhat_rows=%u polys=%u w=%d K=%d l=%d outs=%u alt=%d rc=%d\n", c.name, logn, batch, bhat_rows, polys, d.w, d.K, d.l, outs, alt, rc);
    for (void *b : {T, a, keep_a, work, bhat, keep, out, want, inv}) free(b);
    return bad;
}

}  // namespace

// usage: emu_product_gadget_sweep <class: gl | m64 | m32>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    long cases = 0, bad = 0, fused = 0, point = 0;
    if (const Class *cp = find_class(argv[1])) {
        const Class &c = *cp;
        // digit parameter sets of the class: exact, approximate (low bits dropped), one level
        const Digits gl[] = {{16, 4, 0}, {8, 3, 40}, {22, 3, 0}, {8, 1, 56}}, m64[] = {{16, 4, 0}, {10, 3, 32}, {1, 5, 0}, {8, 1, 56}}, m32[] = {{10, 3, 0}, {7, 2, 16}, {8, 4, 0}, {4, 1, 26}};
        const Digits *ds = c.wb == 4 ? m32 : c.p == 0xFFFFFFFF00000001ull ? gl : m64;
        // the size below the smallest unit, every fused unit size as a single-pass size (launch.h: product_mid_used), one two-pass size
        const int lo = c.wb == 4 ? 5 : 6, two_pass = c.wb == 4 ? 14 : 13;
        for (int logn = lo; logn <= two_pass; logn++) {
            const int nalt = emu_polymul_gadget_alternatives(c.wb, logn, c.p);
            // ragged batches: odd counts leave the last polynomial group of a many-polynomial workgroup part empty; fewer at the large
            // sizes (the host model steps every lane).  The polynomial count (1, 2), the digit set and the output count (2, 3, 1, 2) are
            // drawn from the sweep's fixed random stream; a broadcast always has a second output
            const uint32_t all[] = {1, 5, 33}, js[] = {2, 3, 1, 2};
            const int nb = logn <= 9 ? 3 : logn < two_pass ? 2 : 1;
            long pairing_alts = 0, point_here = 0;
            for (int alt = 0; alt < nalt; alt++)
                for (int bi = 0; bi < nb; bi++)
                    for (int bc = 0; bc < 2; bc++) {
                        const uint32_t batch = logn == two_pass ? 3u : all[bi];
                        if (bc && batch == 1u) continue;  // the same call
                        const uint32_t polys = 1u + (uint32_t) ((rnd() >> 8) & 1);
                        const Digits &d = ds[(rnd() >> 8) & 3];
                        uint32_t outs = js[(rnd() >> 8) & 3];
                        if (bc && outs < 2) outs = 2;
                        bad += one_case(c, logn, batch, bc ? 1u : batch, polys, d, outs, alt);
                        cases++;
                        const int f = emu_polymul_gadget_fused(c.wb, logn, c.p, batch, 8, alt, 0);
                        fused += f != 0;
                        if (f == 2 && bi == 0 && bc == 0) pairing_alts++;
                        if (f == 2 && bc && (batch & 1u) && outs >= 2) point_here++;
                    }
            if (pairing_alts > 0 && point_here == 0) {
                fprintf(stderr, "NO ragged broadcast case through the two-output digit kernel at %s logn=%d\n", c.name, logn);
                bad++;
            }
            point += point_here;
        }
    }
    printf("%s: %ld cases with digit launches\n", argv[1], fused);
    printf("%s: %ld paired ragged broadcast cases\n", argv[1], point);
    return report(argv[1], cases, bad);
}
#endif
