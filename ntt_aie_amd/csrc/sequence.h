// sequence.h -- which launches an entry point makes, in which order and with which arguments: the third shared layer beside
// launch.h's kernel selection and argument fill.  Host code only (no hip_runtime.h, included by no kernel translation unit): the C-ABI
// (ntt_api.hip) hands every Step to a GPU launcher, the host index model (tests/emu) steps the same list on the CPU, so the pass order,
// the buffer each pass reads and the pass that carries an operand are written once.
//
// Contract of every sequence below:
//   * forward passes run in ascending, inverse passes in descending stage order; the first step emitted reads the caller's input,
//     every later one runs in place on the output (which may alias the input);
//   * an operand rides on ONE step: in2 / pw_scale and lde_* on the pass that holds stage 0 of a forward sequence (the first
//     one emitted), do_scale / tw_sc and cinv_u on the pass that holds stage 0 of an inverse sequence (the last one emitted);
//   * emit(step) returns 0 to go on; anything else ends the sequence and is returned.  Nothing is allocated, nothing dereferenced.
#pragma once
#include <stddef.h>
#include <string.h>

#include "launch.h"

namespace ntt {

// What a sequence needs to know of a plan (ntt_plan is one; the host model fills one from host tables).
struct PlanFacts {
    int logn = 0;
    uint64_t p = 0;
    int word_bytes = 0;
    FieldParams field = {};  // arithmetic (launch.h: FieldKind) and its Montgomery constants
    // tables, table form
    void *tw_fwd = nullptr;
    void *tw_inv = nullptr;
    void *tw_inv_sc = nullptr;  // 8-byte words (both fields): T^-1[N/2 + i] * N^-1, i < N/2 (stage-0 twiddles of the scaled inverse, pass.h: fold_scale)
    uint64_t scale_tf = 0;      // N^-1 in table form
    uint64_t ninv_plain = 0;    // N^-1 plain
    uint32_t target_wgs = 8192;  // workgroups per launch the batch loop of a CONTIG pass is sized for (sweep: profiles/)
    // ... of a column pass: 16384 (their tile streams 8 polynomials per workgroup at N = 2^16, batch 4096, instead of 16): -4 %
    uint32_t target_wgs_col = 2 * 8192;
    // ntt_plan_set_coset: low-degree extension onto shift * <w_N> from N >> lde_beta coefficients (0 = not set)
    int lde_beta = 0;
    void *lde_s = nullptr;  // s[i] = shift^bitrev(i), table form, max(N >> lde_beta, 4) words (misc_kernels.hip: gen_coset_kernel)
    // ntt_plan_set_coset_inverse: interpolation from shift * <w_N> (independent of the setting above)
    bool cinv_set = false;
    void *cinv_u = nullptr;  // u[i] = shift^-bitrev(i) * N^-1, table form, max(N, 4) words (gen_coset_kernel with shift^-1 and the constant N^-1)
    // experiment build only (-DNTT_EXPERIMENT); the product never changes them
    int dbg = 0;             // NTT_DEBUG_FLAGS
    int force_variant = -1;  // NTT_PASS_VARIANT=k: every CONTIG pass runs kernel variant k
    int only_pass = -1;      // NTT_ONLY_PASS=k: a forward run of passes launches pass k alone (power / clock of one kernel)
    int lde_unfused = 0;     // NTT_LDE_UNFUSED=1: ntt_lde takes the separate expansion kernel at every size
    int cinv_unfused = 0;    // NTT_COSET_INV_UNFUSED=1: ntt_coset_inverse takes the separate row-scaling kernel at every size
    int mv_single = 0;       // NTT_MATVEC_SINGLE=1: ntt_polymul_matvec_pre runs one summed middle launch per output, no two-output kernel
    int gadget_unfused = 0;  // NTT_GADGET_UNFUSED=1: ntt_polymul_gadget_pre runs the decomposition kernel and the digits' product at every size
};

#if defined(NTT_PHASE_STAMPS)
// diagnostic build: where the pass kernels of this process write their phase stamps (ntt_stamps_set)
struct StampBuffer {
    void *buf = nullptr;
    uint32_t records = 0;
};
inline StampBuffer &stamp_buffer() {
    static StampBuffer b;
    return b;
}
#endif

// which launcher takes a step: launch_pass / launch_mat_pass / launch_product_mid (kernels.h), or their host twins (tests/emu/emu_exec.h)
enum StepFamily { STEP_PASS = 0, STEP_MAT = 1, STEP_PRODUCT = 2 };
struct Step {
    StepFamily family;
    bool inverse;  // (false for the product middle, which runs both directions)
    bool contig;
    int log_m;
    int pass;  // index into the decomposition the step belongs to
    ErasedArgs args;
};

// ---- the decisions that pick a branch -----------------------------------------------------------------------------------------

// the decomposition the launchers run for this batch
inline const std::vector<host::PassDesc> &passes_for(const std::vector<host::PlanAlt> &alts, int forced_alt, size_t batch) {
    const int k = forced_alt >= 0 ? forced_alt : host::select_alternative(alts, batch);
    return alts[(size_t) k].passes;
}

// does ntt_lde expand inside the first pass of this plan (every alternative's first pass has >= 5 stages from logn = 5 on)
inline bool lde_fused(const PlanFacts &pf) { return pf.lde_beta > 0 && pf.logn >= LDE_MIN_LOG_M && !pf.lde_unfused; }

// the kernel variant a pass of this plan runs with
inline int variant_of(const PlanFacts &pf, const host::PassDesc &pd) {
#if defined(NTT_EXPERIMENT)
    if (pf.force_variant >= 0 && pd.contig) return pf.force_variant;  // NTT_PASS_VARIANT=k: A/B of a kernel variant
#endif
    (void) pf;
    return pd.variant;
}

// does the inverse CONTIG pass of this decomposition have a twin with the vector sweep: launch.h's pass_dispatch asked for its
// selection alone -- nothing is launched
inline bool cinv_pass_fused(const PlanFacts &pf, const std::vector<host::PassDesc> &passes) {
    if (pf.cinv_unfused || passes.empty() || !passes[0].contig || passes[0].s0 != 0) return false;
    ErasedArgs a;
    memset(&a, 0, sizeof(a));
    a.n = pf.logn;
    a.variant = variant_of(pf, passes[0]);
    static const char selection_only = 0;  // stands for "a vector is present"
    a.cinv_u = &selection_only;
    return with_field(pf.field, [&](auto f) { return pass_dispatch<decltype(f), true>(true, passes[0].log_m, a, [](auto) {}); });
}
// ntt_plan_info 12: ntt_coset_inverse scales inside its last pass whatever the batch (every alternative, or the pinned one)
inline bool cinv_fused(const PlanFacts &pf, const std::vector<host::PlanAlt> &alts, int forced_alt) {
    if (!pf.cinv_set) return false;
    if (forced_alt >= 0) return cinv_pass_fused(pf, alts[(size_t) forced_alt].passes);
    for (const host::PlanAlt &alt : alts)
        if (!cinv_pass_fused(pf, alt.passes)) return false;
    return true;
}

// PassArgs::pw_scale of a fused pointwise product * scale (plain): scale * R^2, i.e. the table form of the table form
inline uint64_t pw_scale_form(const PlanFacts &pf, uint64_t scale_plain) {
    return host::to_table_form(host::to_table_form(scale_plain % pf.p, pf.p, pf.word_bytes), pf.p, pf.word_bytes);
}

// Does ntt_polymul_negacyclic take the fused middle pass?  Goldilocks, first (or only) pass of 7..12 stages: the radix-8 product
// kernel exists for that unit size; 4-byte words: radix-16 product kernel, unit sizes 2^6 .. 2^13 (any odd p).  The product launch
// is not sliced: beyond blockIdx.y's range (tens of millions of tiny polynomials) the separate passes run, whose launcher slices
// the batch.  The check IS the launcher's geometry call (launch.h: product_mid_fits).
inline bool polymul_fused(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, size_t batch) {
    const host::PassDesc &first = passes.front();
    return first.contig && product_mid_used(pf.field, first.log_m) && product_mid_fits(pf.field, first.log_m, pf.logn, (uint32_t) batch, pf.target_wgs);
}
// are the operands of a product one [2 * batch][N] buffer (then a pass over both is ONE launch)
inline bool operands_contiguous(const PlanFacts &pf, const void *a, const void *b, size_t batch) {
    const size_t operand_bytes = (batch << pf.logn) * (size_t) pf.word_bytes;
    return (const char *) b == (const char *) a + operand_bytes && 2 * batch <= 0x7FFFFFFFull;
}

// log2 of the virtual row length of a matrix call: the column tile's width at least, then the next power of two >= width
inline int mat_log_w(int word_bytes, size_t width) {
    int w = col_log_c(word_bytes);
    while (((size_t) 1 << w) < width && w < MAT_MAX_LOG_WORDS) ++w;
    return w;
}

// ---- the steps ------------------------------------------------------------------------------------------------------------------

// the arguments every launch of a plan shares
inline ErasedArgs step_args(const PlanFacts &pf, const host::PassDesc &pd, const void *in, void *out, size_t batch) {
    ErasedArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.out = out;
    a.field = pf.field;
    a.n = pf.logn;
    a.s0 = pd.s0;
    a.batch = (uint32_t) batch;
    a.target_wgs = pd.contig ? pf.target_wgs : pf.target_wgs_col;
    a.dbg = pf.dbg;
    a.variant = variant_of(pf, pd);
#if defined(NTT_PHASE_STAMPS)
    // one region per pass kind, so that the passes of one transform do not overwrite each other's records: the CONTIG pass
    // takes the first half of the buffer, a column pass the second (tools/phase_stamps.py stamps two-pass transforms)
    a.stamp_records = stamp_buffer().records / 2;
    a.stamps = stamp_buffer().buf ? (char *) stamp_buffer().buf + (pd.contig ? 0 : (size_t) a.stamp_records * STAMP_RECORD * 8) : nullptr;
#endif
    return a;
}
// ... and the table of the direction: one ordinary pass
inline Step pass_step(const PlanFacts &pf, const host::PassDesc &pd, int pass, bool inverse, const void *in, void *out, size_t batch, int layout) {
    Step st{STEP_PASS, inverse, pd.contig, pd.log_m, pass, step_args(pf, pd, in, out, batch)};
    st.args.tw = inverse ? pf.tw_inv : pf.tw_fwd;
    st.args.layout = layout;
    return st;
}

// Passes [lo, hi) of a decomposition in execution order; tweak(args, i) adds what only pass i has.
// (experiment build, NTT_ONLY_PASS=k: a forward run emits pass k alone -- a timing experiment, outputs meaningless)
template <class Tweak, class Emit>
int seq_passes(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, size_t lo, size_t hi, bool inverse, const void *in, void *out,
               size_t batch, int layout, Tweak &&tweak, Emit &&emit) {
    const void *src = in;
    for (size_t k = lo; k < hi; k++) {
        const size_t i = inverse ? lo + (hi - 1 - k) : k;
#if defined(NTT_EXPERIMENT)
        if (!inverse && pf.only_pass >= 0 && (int) i != pf.only_pass) continue;
#endif
        Step st = pass_step(pf, passes[i], (int) i, inverse, src, out, batch, layout);
        tweak(st.args, i);
        if (const int rc = emit(st)) return rc;
        src = out;
    }
    return 0;
}

// ntt_forward (and ntt_forward_profile).  in2 != null: transform in[j] * in2[j] * pw_scale (plain) instead of in[j], the product
// folded into the load of the first pass only (out may alias in).  skip_if: experiment build, the fallback behind the fused launch.
template <class Emit>
int seq_forward(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, const void *in, void *out, size_t batch, int layout, const void *in2,
                uint64_t pw_scale_plain, const void *skip_if, Emit &&emit) {
    const uint64_t pw_scale = in2 ? pw_scale_form(pf, pw_scale_plain) : 0;
    return seq_passes(pf, passes, 0, passes.size(), false, in, out, batch, layout, [&](ErasedArgs &a, size_t i) {
        a.skip_if = skip_if;
        if (i == 0 && in2) {
            a.in2 = in2;
            a.pw_scale = pw_scale;
        }
    }, emit);
}

// ntt_inverse.  8-byte words: N^-1 rides on the last executed stage (stage 0 of the CONTIG pass, tw_sc) instead of a sweep over
// the outputs.
template <class Emit>
int seq_inverse(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, const void *in, void *out, size_t batch, int layout, int scale, Emit &&emit) {
    return seq_passes(pf, passes, 0, passes.size(), true, in, out, batch, layout, [&](ErasedArgs &a, size_t i) {
        a.do_scale = (scale && i == 0) ? 1 : 0;
        a.scale = pf.scale_tf;
        a.tw_sc = a.do_scale ? pf.tw_inv_sc : nullptr;
    }, emit);
}

// ntt_lde where lde_fused(): the first pass expands while it loads -- it reads the compact `in` through lde_in only and writes
// `out`; its ordinary input is `out`, which it does not read.
template <class Emit>
int seq_lde(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, const void *in, void *out, size_t batch, int layout, Emit &&emit) {
    return seq_passes(pf, passes, 0, passes.size(), false, out, out, batch, layout, [&](ErasedArgs &a, size_t i) {
        if (i == 0) {
            a.lde_in = in;
            a.lde_s = pf.lde_s;
            a.lde_beta = pf.lde_beta;
        }
    }, emit);
}

// ntt_coset_inverse where cinv_pass_fused(): the passes of the unscaled inverse; the last one launched (the CONTIG pass)
// multiplies by the vector, which contains N^-1, before it stores.
template <class Emit>
int seq_coset_inverse(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, const void *in, void *out, size_t batch, int layout, Emit &&emit) {
    return seq_passes(pf, passes, 0, passes.size(), true, in, out, batch, layout, [&](ErasedArgs &a, size_t i) {
        if (i == 0) a.cinv_u = pf.cinv_u;
    }, emit);
}

// ntt_forward_columns / ntt_inverse_columns: count matrices [N][pitch], the first `width` words of a row are live.  Every stage is a
// column pass over the virtual polynomial of 2^(logn + w) words (pass.h: PassCfg::MAT), w = mat_log_w(width).
// ntt_lde_columns (COL_LDE) and ntt_coset_inverse_columns (COL_CINV) are the same loop with the coset twin in the pass that holds
// stage 0 (pass.h: PassCfg::MLDE / MCINV): the LDE reads a compact [N >> beta][in_pitch] source there and is out of place only.
enum ColKind { COL_PLAIN = 0, COL_LDE = 1, COL_CINV = 2 };
template <class Emit>
int seq_columns(const PlanFacts &pf, const std::vector<host::PassDesc> &col_passes, ColKind kind, const void *in, size_t in_pitch, void *out, size_t pitch,
                size_t width, size_t count, bool inverse, int scale, Emit &&emit) {
    const int w = mat_log_w(pf.word_bytes, width);
    const void *src = in;
    for (size_t k = 0; k < col_passes.size(); k++) {
        const size_t i = inverse ? col_passes.size() - 1 - k : k;
        const host::PassDesc &pd = col_passes[i];
        Step st{STEP_MAT, inverse, false, pd.log_m, (int) i, step_args(pf, pd, src, out, count)};
        ErasedArgs &a = st.args;
        a.n = pf.logn + w;
        a.s0 = pd.s0 + w;
        a.mat_w = w;
        a.mat_pitch = (uint32_t) pitch;
        a.mat_width = (uint32_t) width;
        a.tw = inverse ? pf.tw_inv : pf.tw_fwd;
        a.layout = LAYOUT_NATURAL;
        a.do_scale = (inverse && scale && pd.s0 == 0) ? 1 : 0;  // the sweep of the last executed pass, the one that holds stage 0
        a.scale = pf.scale_tf;
        if (kind == COL_LDE && pd.s0 == 0) {  // the first executed pass: compact source in, expanded tile out (`in` is not read)
            a.in = out;
            a.mat_lde_in = in;
            a.mat_lde_s = pf.lde_s;
            a.mat_lde_beta = pf.lde_beta;
            a.mat_src_pitch = (uint32_t) in_pitch;
        }
        if (kind == COL_CINV && pd.s0 == 0) a.mat_cinv_u = pf.cinv_u;  // the last executed pass: N^-1 is inside the vector
        if (const int rc = emit(st)) return rc;
        src = out;
    }
    return 0;
}

// ntt_polymul_negacyclic where polymul_fused(): the column passes (if any) of both unscaled inverse transforms -- per operand, or
// once over 2 * batch rows when the operands are contiguous -- then ONE launch that runs the last inverse pass of a and of b, the
// pointwise product * N^-1 and the first forward pass on each 2^log_m-word unit while it is workgroup-resident (tw = inverse table,
// tw2 = forward table), then the forward column passes in place on `out`.  A single-pass size is the middle step alone.
template <class Emit>
int seq_polymul_fused(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, void *a, void *b, void *out, size_t batch, Emit &&emit) {
    const bool contiguous = operands_contiguous(pf, a, b, batch);
    for (size_t i = passes.size(); i-- > 1;)
        for (int op = 0; op < (contiguous ? 1 : 2); op++) {
            void *buf = op == 0 ? a : b;
            if (const int rc = emit(pass_step(pf, passes[i], (int) i, true, buf, buf, contiguous ? 2 * batch : batch, LAYOUT_NATURAL))) return rc;
        }
    const host::PassDesc &first = passes.front();
    Step mid{STEP_PRODUCT, false, true, first.log_m, 0, step_args(pf, first, a, out, batch)};
    mid.args.in2 = b;
    mid.args.tw = pf.tw_inv;
    mid.args.tw2 = pf.tw_fwd;
    mid.args.layout = LAYOUT_NATURAL;
    mid.args.pw_scale = pw_scale_form(pf, pf.ninv_plain);
    if (const int rc = emit(mid)) return rc;
    return seq_passes(pf, passes, 1, passes.size(), false, out, out, batch, LAYOUT_NATURAL, [](ErasedArgs &, size_t) {}, emit);
}

// ntt_polymul_negacyclic_pre: operand b arrives prepared, bhat = InvU(b) in natural order, canonical words -- [batch][N] (bhat_rows ==
// batch) or ONE row that multiplies every polynomial (bhat_rows == 1); bhat is never written.
// Where polymul_fused(): the inverse column passes of a alone, over `batch` rows, then ONE launch that runs the last inverse pass of a,
// the product with the thread's words of bhat * N^-1 and the first forward pass per resident unit (in2 = bhat, in2_prepared, in2_broadcast),
// then the forward column passes in place on `out`.  A single-pass size is the middle step alone.
// Everywhere else: the unscaled inverse of a in place, then the forward transform with the per-row operand folded into its first pass
// (seq_forward's in2), or -- the broadcast -- row_mul(a, bhat), which multiplies every row of a by bhat * N^-1 in place (a launch of its
// own, kernels.h: launch_pointwise_row), and the plain forward transform.
template <class Emit, class RowMul>
int seq_polymul_pre(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, void *a, const void *bhat, size_t bhat_rows, void *out, size_t batch, Emit &&emit,
                    RowMul &&row_mul) {
    const bool bcast = bhat_rows != batch;  // (batch == 1: the two cases are one, and the per-row addressing serves it)
    if (!polymul_fused(pf, passes, batch)) {
        if (const int rc = seq_inverse(pf, passes, a, a, batch, LAYOUT_NATURAL, 0, emit)) return rc;
        if (!bcast) return seq_forward(pf, passes, a, out, batch, LAYOUT_NATURAL, bhat, pf.ninv_plain, nullptr, emit);
        if (const int rc = row_mul(a, bhat)) return rc;
        return seq_forward(pf, passes, a, out, batch, LAYOUT_NATURAL, nullptr, 1, nullptr, emit);
    }
    for (size_t i = passes.size(); i-- > 1;)
        if (const int rc = emit(pass_step(pf, passes[i], (int) i, true, a, a, batch, LAYOUT_NATURAL))) return rc;
    const host::PassDesc &first = passes.front();
    Step mid{STEP_PRODUCT, false, true, first.log_m, 0, step_args(pf, first, a, out, batch)};
    mid.args.in2 = bhat;
    mid.args.in2_prepared = 1;
    mid.args.in2_broadcast = bcast ? 1 : 0;
    mid.args.tw = pf.tw_inv;
    mid.args.tw2 = pf.tw_fwd;
    mid.args.layout = LAYOUT_NATURAL;
    mid.args.pw_scale = pw_scale_form(pf, pf.ninv_plain);
    if (const int rc = emit(mid)) return rc;
    return seq_passes(pf, passes, 1, passes.size(), false, out, out, batch, LAYOUT_NATURAL, [](ErasedArgs &, size_t) {}, emit);
}

// ntt_polymul_dot_pre: out[r] = Fwd( N^-1 . sum_{k < terms} InvU(a[k][r]) . bhat[k][r | 0] ).  a is [terms][batch][N], contiguous and
// overwritten; bhat is [terms][bhat_rows][N] canonical words in natural order (row (k, .) is what ntt_polymul_prepare writes), bhat_rows ==
// batch or 1, never written; out is [batch][N] and may be a (term 0's block).  The decomposition is the one selected for `batch`.
// Where polymul_dot_fused() -- polymul_fused() and a unit size whose summed middle has a kernel (launch.h: product_dot_used: all but the
// general 64-bit modulus at 2^10 and 4-byte words at 2^13) --: the inverse column passes of a as ONE launch each over terms * batch rows (the blocks are contiguous: the
// contiguous-operands case of seq_polymul_fused), then ONE launch that runs, per resident unit, the last inverse pass of every term
// and sums the products with the thread's words of bhat in registers, scales by N^-1 once and runs the first forward pass (in2 = bhat,
// in2_prepared, in2_broadcast, dot_*), then the forward column passes in place on `out`.  A single-pass size is the middle step alone.
// Everywhere else: the unscaled inverse of all terms * batch rows in place, dot_rows(a, bhat), which leaves the scaled sum in term 0's
// block (a launch of its own, kernels.h: launch_dot_rows), and the plain forward transform from there to `out`.
// ONE forward transform on either path, whatever `terms`.  The caller has checked terms >= 1 and terms * batch <= 2^31 - 1.
inline bool polymul_dot_fused(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, size_t batch) {
    return polymul_fused(pf, passes, batch) && product_dot_used(pf.field, passes.front().log_m);
}
template <class Emit, class DotRows>
int seq_polymul_dot(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, void *a, const void *bhat, size_t bhat_rows, size_t terms, void *out, size_t batch,
                    Emit &&emit, DotRows &&dot_rows) {
    const bool bcast = bhat_rows != batch;  // (batch == 1: the two cases are one, and the per-row addressing serves it)
    if (!polymul_dot_fused(pf, passes, batch)) {
        if (const int rc = seq_inverse(pf, passes, a, a, terms * batch, LAYOUT_NATURAL, 0, emit)) return rc;
        if (const int rc = dot_rows(a, bhat)) return rc;
        return seq_forward(pf, passes, a, out, batch, LAYOUT_NATURAL, nullptr, 1, nullptr, emit);
    }
    for (size_t i = passes.size(); i-- > 1;)
        if (const int rc = emit(pass_step(pf, passes[i], (int) i, true, a, a, terms * batch, LAYOUT_NATURAL))) return rc;
    const host::PassDesc &first = passes.front();
    Step mid{STEP_PRODUCT, false, true, first.log_m, 0, step_args(pf, first, a, out, batch)};
    mid.args.in2 = bhat;
    mid.args.in2_prepared = 1;
    mid.args.in2_broadcast = bcast ? 1 : 0;
    mid.args.dot_terms = (int) terms;
    mid.args.dot_in_stride = (uint64_t) batch << pf.logn;
    mid.args.dot_in2_stride = (uint64_t) (bcast ? 1 : batch) << pf.logn;
    mid.args.tw = pf.tw_inv;
    mid.args.tw2 = pf.tw_fwd;
    mid.args.layout = LAYOUT_NATURAL;
    mid.args.pw_scale = pw_scale_form(pf, pf.ninv_plain);
    if (const int rc = emit(mid)) return rc;
    return seq_passes(pf, passes, 1, passes.size(), false, out, out, batch, LAYOUT_NATURAL, [](ErasedArgs &, size_t) {}, emit);
}

// ntt_polymul_matvec_pre: out[j][r] = Fwd( N^-1 . sum_{k < terms} InvU(a[k][r]) . bhat[j][k][r | 0] ), j < outs: `outs` inner products of
// ONE operand a.  a is [terms][batch][N], contiguous and overwritten; bhat is [outs][terms][bhat_rows][N], block j an operand of
// seq_polymul_dot, never written; out is [outs][batch][N] and lies apart from a (the middle launches of later outputs still read a).
// Where polymul_dot_fused(): a's inverse column passes as ONE launch each over terms * batch rows -- once, whatever `outs` --, then the
// middle launches: ONE per pair of outputs (2g, 2g + 1) through the two-output kernel (mv_*; launch.h: product_mv_used) and, for an odd
// `outs`, the summed launch of seq_polymul_dot for the last output with in2 and out rebased; a unit without a two-output kernel runs
// that summed launch once per output.  Then the forward column passes, ONE launch each over outs * batch rows in place on `out` (the
// blocks are contiguous).  A single-pass size is the middle launches alone.
// Everywhere else: the unscaled inverse of all terms * batch rows in place, mv_rows(a, bhat, out), ONE launch that writes the scaled sums
// of every output (kernels.h: launch_matvec_rows), and ONE plain forward transform over outs * batch rows in place on `out`.
// No path has a loop of `terms` launches and none transforms a more than once.  The caller has checked terms, outs >= 1 and
// terms * batch, outs * batch <= 2^31 - 1.
inline bool polymul_matvec_paired(const PlanFacts &pf, const std::vector<host::PassDesc> &passes) {
    return product_mv_used(pf.field, passes.front().log_m) && !pf.mv_single;
}
template <class Emit, class MvRows>
int seq_polymul_matvec(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, void *a, const void *bhat, size_t bhat_rows, size_t terms, size_t outs, void *out,
                       size_t batch, Emit &&emit, MvRows &&mv_rows) {
    const bool bcast = bhat_rows != batch;  // (batch == 1: the two cases are one, and the per-row addressing serves it)
    if (!polymul_dot_fused(pf, passes, batch)) {
        if (const int rc = seq_inverse(pf, passes, a, a, terms * batch, LAYOUT_NATURAL, 0, emit)) return rc;
        if (const int rc = mv_rows(a, bhat, out)) return rc;
        return seq_forward(pf, passes, out, out, outs * batch, LAYOUT_NATURAL, nullptr, 1, nullptr, emit);
    }
    for (size_t i = passes.size(); i-- > 1;)
        if (const int rc = emit(pass_step(pf, passes[i], (int) i, true, a, a, terms * batch, LAYOUT_NATURAL))) return rc;
    const host::PassDesc &first = passes.front();
    const bool paired = polymul_matvec_paired(pf, passes);
    const uint64_t row = (uint64_t) 1 << pf.logn, in2_stride = (bcast ? 1 : (uint64_t) batch) * row;
    const size_t out_bytes = (size_t) (batch * row) * (size_t) pf.word_bytes, bhat_bytes = (size_t) (terms * in2_stride) * (size_t) pf.word_bytes;  // of ONE output
    for (size_t j = 0; j < outs;) {
        const bool two = paired && j + 1 < outs;
        Step mid{STEP_PRODUCT, false, true, first.log_m, 0, step_args(pf, first, a, (char *) out + j * out_bytes, batch)};
        mid.args.in2 = (const char *) bhat + j * bhat_bytes;
        mid.args.in2_prepared = 1;
        mid.args.in2_broadcast = bcast ? 1 : 0;
        mid.args.dot_terms = (int) terms;
        mid.args.dot_in_stride = batch * row;
        mid.args.dot_in2_stride = in2_stride;
        if (two) {
            mid.args.mv_outs = 2;
            mid.args.mv_in2_stride = terms * in2_stride;
            mid.args.mv_out_stride = batch * row;
        }
        mid.args.tw = pf.tw_inv;
        mid.args.tw2 = pf.tw_fwd;
        mid.args.layout = LAYOUT_NATURAL;
        mid.args.pw_scale = pw_scale_form(pf, pf.ninv_plain);
        if (const int rc = emit(mid)) return rc;
        j += two ? 2 : 1;
    }
    return seq_passes(pf, passes, 1, passes.size(), false, out, out, outs * batch, LAYOUT_NATURAL, [](ErasedArgs &, size_t) {}, emit);
}

// ntt_polymul_gadget_pre: out[j][r] = Fwd( N^-1 . sum_t InvU(digit_{t mod levels}(a[t div levels][r])) . bhat[j][t][r | 0] ), t < polys * levels,
// j < outs: seq_polymul_matvec of the balanced gadget digits of a (pass.h: gadget_digit).  a is [polys][batch][N] canonical words and is
// NEVER written; work is caller scratch of polys * levels * batch * N words; bhat is [outs][polys * levels][bhat_rows][N], never written;
// out is [outs][batch][N]; the four lie apart.
// Where polymul_gadget_fused() -- the decomposition for this batch is ONE pass, polymul_dot_fused(), and the unit has digit kernels
// (launch.h: product_gadget_used) --: only the middle launches of seq_polymul_matvec, as digit launches (gad_*) that read a itself and
// decompose in registers: ONE per pair of outputs where the two-output kernel is used plus a summed one for an odd last output, else one
// per output.  No decomposition step, nothing reads or writes work.
// Everywhere else -- a multi-pass size, a size without a fused middle, a unit without a digit kernel, a pinned alternative without a
// middle, the experiment build's switch --: decompose(a, work), ONE launch of the decomposition kernel (kernels.h:
// launch_gadget_decompose), then exactly seq_polymul_matvec on work.
// Either way block j of out holds the words seq_polymul_matvec leaves for the digits: the digit launches run its kernels' code on the
// same words in the same order.  The caller has checked the digit parameters (pass.h: gadget_params_ok), polys, outs >= 1 and
// polys * levels * batch, outs * batch <= 2^31 - 1.
inline bool polymul_gadget_fused(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, size_t batch) {
    return passes.size() == 1 && polymul_dot_fused(pf, passes, batch) && product_gadget_used(pf.field, passes.front().log_m) && !pf.gadget_unfused;
}
template <class Emit, class MvRows, class Decompose>
int seq_polymul_gadget(const PlanFacts &pf, const std::vector<host::PassDesc> &passes, const void *a, size_t polys, int log_base, int levels, int low_bits, void *work,
                       const void *bhat, size_t bhat_rows, size_t outs, void *out, size_t batch, Emit &&emit, MvRows &&mv_rows, Decompose &&decompose) {
    const size_t terms = polys * (size_t) levels;
    if (!polymul_gadget_fused(pf, passes, batch)) {
        if (const int rc = decompose(a, work)) return rc;
        return seq_polymul_matvec(pf, passes, work, bhat, bhat_rows, terms, outs, out, batch, emit, mv_rows);
    }
    // the middle launches of seq_polymul_matvec with `a` in the place of the digits; the digit parameters ride on each
    return seq_polymul_matvec(
        pf, passes, const_cast<void *>(a), bhat, bhat_rows, terms, outs, out, batch,
        [&](const Step &st) {
            Step mid = st;
            mid.args.gad_log_base = log_base;
            mid.args.gad_levels = levels;
            mid.args.gad_low_bits = low_bits;
            return emit(mid);
        },
        mv_rows);
}

}  // namespace ntt
