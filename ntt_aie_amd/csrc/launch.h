// launch.h -- which kernel runs for a pass, and with which arguments: the field descriptor, the type-erased launch
// arguments, the selection rules and the ErasedArgs -> PassArgs<Cfg> fill.  Host code only (no hip_runtime.h): the GPU
// launchers (pass_kernel.inc, product_kernel.inc, misc_kernels.hip) and the host index model (tests/emu, plain g++)
// both go through here, so what the CPU suite steps is what the GPU launches.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "pass.h"
#include "plan.h"

namespace ntt {

// arithmetic of a plan: FieldM32 (4-byte words), FieldGL (p = 2^64 - 2^32 + 1), FieldM64 (any other odd 8-byte modulus)
enum FieldKind { FK_M32 = 0, FK_GL = 1, FK_M64 = 2 };
struct FieldParams {
    FieldKind kind;
    uint64_t p, pinv, r2;  // modulus and its Montgomery constants (pinv, r2: 0 for Goldilocks, which has none)
};
inline FieldParams field_params(int word_bytes, uint64_t p) {
    if (word_bytes == 4) return {FK_M32, p, host::mont_pinv((uint32_t) p), host::mont_r2((uint32_t) p)};
    if (p == host::GOLDILOCKS) return {FK_GL, p, 0, 0};
    return {FK_M64, p, host::mont_pinv64(p), host::mont_r2_64(p)};
}
inline int field_word_bytes(const FieldParams &fp) { return fp.kind == FK_M32 ? 4 : 8; }
template <class F>
F make_field(const FieldParams &fp) {
    using W = typename F::W;
    if constexpr (std::is_same<F, FieldGL>::value) return FieldGL{};
    else return F{(W) fp.p, (W) fp.pinv, (W) fp.r2};
}
// fn(field object of the plan's arithmetic); the one place a FieldKind turns into a type
template <class Fn>
auto with_field(const FieldParams &fp, Fn &&fn) {
    if (fp.kind == FK_GL) return fn(make_field<FieldGL>(fp));
    if (fp.kind == FK_M64) return fn(make_field<FieldM64>(fp));
    return fn(make_field<FieldM32>(fp));
}

struct ErasedArgs {
    const void *in;
    void *out;
    const void *tw;
    const void *tw_sc;     // scaled inverse, 8-byte CONTIG pass: stage-0 twiddles * N^-1 (PassArgs::tw_sc); null = phase_scale
    FieldParams field;
    int n, s0;
    uint32_t batch;
    int layout;
    int do_scale;
    uint64_t scale;  // table form
    uint32_t target_wgs;
    int dbg;  // timing experiments (NTT_DEBUG_FLAGS), 0 in production
    const void *tw2;     // product_mid launch: the FORWARD table (tw is the inverse one there)
    const void *in2;     // forward CONTIG pass: second operand of a fused pointwise product (or null)
    uint64_t pw_scale;   // scale * R^2 (see PassArgs::pw_scale)
    const void *skip_if;  // experiment build only: device word, non-zero = the launch is a no-op (fallback behind the fused kernel)
    int variant;          // PassDesc::variant (plan.h): 0 = the default kernel of this (contig, log_m); 1 = single-pass CONTIG unit of 10..12
                          // stages as radix-8 rounds in 512 threads (twice the waves per unit: small batches, one generation of workgroups)
    const void *lde_in;   // forward CONTIG first pass of ntt_lde: compact source / coset vector / log2 blow-up (PassArgs::lde_*);
    const void *lde_s;    // lde_beta == 0: an ordinary launch
    int lde_beta;
    const void *cinv_u;   // inverse CONTIG pass of ntt_coset_inverse: the per-position output vector (PassArgs::cinv_u); null: an ordinary launch
    int mat_w;            // column pass over row-major matrices (ntt_*_columns; PassArgs::mat_*): log2 virtual row length / row pitch /
    uint32_t mat_pitch;   // live columns.  n and s0 are then the virtual polynomial's, batch counts matrices.  All zero: an ordinary
    uint32_t mat_width;   // launch
    // The coset twins of the matrix pass (PassCfg::MLDE / MCINV) have operands of their own here -- lde_* and cinv_u above stay "off" in
    // every matrix launch, they select CONTIG kernels -- and share the PassArgs fields: the first pass of ntt_lde_columns reads the compact
    // source mat_lde_in (row pitch mat_src_pitch) times the coset vector mat_lde_s, blow-up 2^mat_lde_beta (0: not such a launch); the
    // last pass of ntt_coset_inverse_columns multiplies row r by mat_cinv_u[r] (null: not such a launch)
    const void *mat_lde_in;
    const void *mat_lde_s;
    int mat_lde_beta;
    uint32_t mat_src_pitch;
    const void *mat_cinv_u;
    // product_mid launch of ntt_polymul_negacyclic_pre: in2 is the PREPARED operand InvU(b), natural order, canonical words -- [batch][N],
    // or ONE row of N words that multiplies every polynomial (in2_broadcast).  Both zero: every other launch
    int in2_prepared;
    int in2_broadcast;
    // product_mid launch of ntt_polymul_dot_pre: the prepared middle summed over dot_terms terms (0: every other launch).  Term k reads its
    // unit of operand a at in + k * dot_in_stride words and its prepared words at in2 + k * dot_in2_stride words (in2_prepared set,
    // in2_broadcast as above, per term); `batch` is the rows of ONE term
    int dot_terms;
    uint64_t dot_in_stride;
    uint64_t dot_in2_stride;
    // product_mid launch of ntt_polymul_matvec_pre that sums for TWO outputs at once (run_product_mv_pass): mv_outs == 2, and a summed
    // launch in everything else (dot_* as above, for output 0).  Output 1 reads its prepared words mv_in2_stride words after output 0's
    // (one output's block of the operand: terms * bhat_rows * N) and stores mv_out_stride words after it (batch * N).  0: every other launch
    int mv_outs;
    uint64_t mv_in2_stride;
    uint64_t mv_out_stride;
    // product_mid launch of ntt_polymul_gadget_pre (the digit variants of the two summed kernels): gad_levels > 0.  `in` is then
    // [dot_terms / gad_levels][batch][N] canonical words that are decomposed in registers: term t is digit_{t % gad_levels} of
    // polynomial t / gad_levels (pass.h: gadget_digit); dot_* and mv_* as above.  All zero: every other launch
    int gad_log_base;
    int gad_levels;
    int gad_low_bits;
#if defined(NTT_PHASE_STAMPS)
    void *stamps;            // diagnostic build: PassArgs::stamps / stamp_records (ntt_stamps_set)
    uint32_t stamp_records;
#endif
};

// ---- the pass kernels of one (field, direction) ------------------------------------------------------------------
// (CINV: the coset-interpolation twin of an inverse kernel, PassCfg::CINV -- the same shape with the vector sweep at its end)
template <class F, int LOG_M, bool INV, bool CINV = false>
using ContigCfg = PassCfg<F, LOG_M, 0, true, INV, contig_preload_mask(LOG_M, sizeof(typename F::W)), 4, LOG_NT, true, false, CINV>;
// 13 stages on an 8192-word tile: 512 threads x 16 words, rounds of 4 + 4 + 4 + 1 stages.  4-byte words keep every round's
// twiddles in registers (99 VGPRs); 8-byte words only the last round's single, wave-uniform one (the others are re-read
// from L2 at the start of their round, as in the 12-stage radix-16 pass: 128 VGPRs, two workgroups per CU)
template <class F, bool INV, bool CINV = false>
using ContigCfg13 = PassCfg<F, 13, 0, true, INV, sizeof(typename F::W) == 4 ? 0xF : 0x8, 4, 9, true, false, CINV>;
// 14 stages on a 16384-word tile of 4-byte words (64 KiB): ONE 1024-thread workgroup per CU, rounds of 4 + 4 + 4 + 2 stages, every
// round's twiddles resident.  Pays only for the lazy butterflies (p < 2^30: N = 2^14 in one pass -21 % forward, -5 % inverse at
// saturating batches; +3 % for a 32-bit prime, +20 % for one polynomial: profiles/r02_ab_13_stage_pass.txt), so the planner offers it
// as a launch-time alternative for that modulus class above a batch threshold (plan.h: plan_alternatives)
template <class F, bool INV, bool CINV = false>
using ContigCfg14 = PassCfg<F, 14, 0, true, INV, 0xF, 4, 10, true, false, CINV>;
// radix-8 rounds: 256 threads up to 9 stages, 512 threads for 10..12.  ALLOW_DMA = false: the same kernel with the tile staged
// by ordinary loads, which is where a fused pointwise product (a.in2) has room to multiply
template <class F, int LOG_M, bool INV, bool ALLOW_DMA = true, bool CINV = false>
using ContigCfgE8 = PassCfg<F, LOG_M, 0, true, INV, 0xF, 3, LOG_M >= 10 ? 9 : 8, ALLOW_DMA, false, CINV>;

// fn(std::integral_constant<int, M>{}) for the M in [LO, HI] that equals log_m; false = none does
template <int LO, int HI, class Fn>
bool with_log_m(int log_m, Fn &&fn) {
    if constexpr (LO > HI) {
        return false;
    } else {
        if (log_m != LO) return with_log_m<LO + 1, HI>(log_m, fn);
        fn(std::integral_constant<int, LO>{});
        return true;
    }
}

// The CONTIG kernel of 2^log_m words for this launch.  CINV: its coset-interpolation twin (inverse only) -- the SAME shape rule, so
// ntt_coset_inverse's last pass is the kernel ntt_inverse would run there plus the vector sweep; twins exist where the pass has two
// register rounds or more (log_m >= 5: every radix-8 shape, 13, 14 of 4-byte words -- the family lde_dispatch covers forward).
constexpr int CINV_MIN_LOG_M = 5;
template <class F, bool INV, bool CINV, class Fn>
bool contig_dispatch(int log_m, const ErasedArgs &a, bool last_pass, Fn &&fn) {
    static_assert(INV || !CINV, "coset interpolation ends an INVERSE transform");
    constexpr int WB = (int) sizeof(typename F::W);
    if (log_m == 13) {
        fn(CfgTag<ContigCfg13<F, INV, CINV>>{});
        return true;
    }
    if (log_m == 14) {
        if constexpr (WB == 4) fn(CfgTag<ContigCfg14<F, INV, CINV>>{});
        return WB == 4;
    }
    // PassDesc::variant 1: a single-pass unit of 2^10 .. 2^12 words on 512 threads x 8 words (radix-8 rounds; 8-byte forward: the
    // LDS-DMA kernel that otherwise runs as the first pass of a two-pass plan) instead of 256 x 16 -- twice the waves for the same
    // work, for launches too small to fill the SIMDs (plan.h: plan_alternatives).  Both layouts (pass.h: elem_off / lane_eff);
    // a fused pointwise operand keeps the default kernel.
    if (a.variant == 1 && a.in2 == nullptr && with_log_m<10, 12>(log_m, [&](auto m) { fn(CfgTag<ContigCfgE8<F, decltype(m)::value, INV, true, CINV>>{}); }))
        return true;
    if constexpr (WB == 8) {
        if (contig_log_e(log_m, WB, last_pass) == 3) {
            if constexpr (!INV) {  // fused pointwise product: the twins without LDS-DMA
                if (a.in2 != nullptr) return with_log_m<7, 12>(log_m, [&](auto m) { fn(CfgTag<ContigCfgE8<F, decltype(m)::value, INV, false>>{}); });
            }
            return with_log_m<7, 12>(log_m, [&](auto m) { fn(CfgTag<ContigCfgE8<F, decltype(m)::value, INV, true, CINV>>{}); });
        }
    }
    return with_log_m<(CINV ? CINV_MIN_LOG_M : 1), 12>(log_m, [&](auto m) { fn(CfgTag<ContigCfg<F, decltype(m)::value, INV, CINV>>{}); });
}

// THE selection rule: fn(CfgTag<Cfg>{}) with the configuration of the pass kernel that runs stages [a.s0, a.s0 + log_m) of
// this launch; false = no such kernel.
template <class F, bool INV, class Fn>
bool pass_dispatch(bool contig, int log_m, const ErasedArgs &a, Fn &&fn) {
    const bool last_pass = a.s0 + log_m == a.n;
    if (a.lde_beta != 0) {  // first pass of ntt_lde: the fused-expansion twin of this shape (pass.h: lde_dispatch)
        if constexpr (INV) return false;
        else return contig && a.cinv_u == nullptr && lde_dispatch<F>(log_m, last_pass, fn);
    }
    if (a.cinv_u != nullptr) {  // last executed pass of ntt_coset_inverse: the twin with the vector sweep
        if constexpr (INV) return contig && contig_dispatch<F, true, true>(log_m, a, last_pass, fn);
        else return false;
    }
    if (!contig)  // 9: 512 rows x one 128-byte segment: N = 2^22 = 13 + 9 in two passes
        return with_log_m<4, 9>(log_m, [&](auto m) { fn(CfgTag<ColPassCfg<F, decltype(m)::value, INV>>{}); });
    return contig_dispatch<F, INV, false>(log_m, a, last_pass, fn);
}

// The matrix twin of the column pass of log_m stages (PassCfg::MAT, pass.h: ColMatCfg); the only kernels a launch with the matrix
// arguments may run, and no other launch may run them (fill_pass_args).
template <class F, bool INV, class Fn>
bool mat_dispatch(int log_m, Fn &&fn) {
    return with_log_m<host::MIN_COL_LOG_M, host::MAX_COL_LOG_M>(log_m, [&](auto m) { fn(CfgTag<ColMatCfg<F, decltype(m)::value, INV>>{}); });
}

// ... and its coset twins (pass.h: ColMatLdeCfg / ColMatCinvCfg), named by the launch's own operands: the fused expansion of
// ntt_lde_columns (a.mat_lde_beta != 0, forward only), the per-row output scaling of ntt_coset_inverse_columns (a.mat_cinv_u, inverse only).
// The rule of every matrix launch of the library; a launch without those operands gets the plain twin, exactly as mat_dispatch names it.
template <class F, bool INV, class Fn>
bool mat_twin_dispatch(int log_m, const ErasedArgs &a, Fn &&fn) {
    if (a.mat_lde_beta != 0 && a.mat_cinv_u != nullptr) return false;
    if (a.mat_lde_beta != 0) {
        if constexpr (INV) return false;
        else return with_log_m<host::MIN_COL_LOG_M, host::MAX_COL_LOG_M>(log_m, [&](auto m) { fn(CfgTag<ColMatLdeCfg<F, decltype(m)::value>>{}); });
    }
    if (a.mat_cinv_u != nullptr) {
        if constexpr (INV) return with_log_m<host::MIN_COL_LOG_M, host::MAX_COL_LOG_M>(log_m, [&](auto m) { fn(CfgTag<ColMatCinvCfg<F, decltype(m)::value>>{}); });
        else return false;
    }
    return mat_dispatch<F, INV>(log_m, fn);
}

// Largest matrix (N * pitch words) and virtual polynomial a matrix launch takes: those of a size-2^28 transform, so that every
// 32-bit lane / element byte offset a column pass forms stays where it is for the largest ordinary plan (NTT_MAX_LOGN)
constexpr int MAT_MAX_LOG_WORDS = 28;
inline uint64_t mat_words(const ErasedArgs &e) { return e.n >= e.mat_w && e.n - e.mat_w < 32 ? ((uint64_t) 1 << (e.n - e.mat_w)) * e.mat_pitch : ~(uint64_t) 0; }
// words of one compact source matrix of an MLDE launch (0 for every other launch)
inline uint64_t mat_src_words(const ErasedArgs &e) {
    return e.mat_lde_beta > 0 && e.n >= e.mat_w + e.mat_lde_beta && e.n - e.mat_w < 32 ? ((uint64_t) 1 << (e.n - e.mat_w - e.mat_lde_beta)) * e.mat_src_pitch : 0;
}
// Unit slots of a MAT workgroup that are used.  A small matrix leaves room for several per workgroup (log_up > 0), whose lane
// offsets reach 2^log_up * N * pitch words whatever the width: no more matrices share a workgroup than keep that within
// 2^MAT_MAX_LOG_WORDS; lanes of the slots beyond are dead (pass.h: Ctx::live).
inline int mat_log_u(const ErasedArgs &e, int log_m, int log_c, int log_u) {
    const int one_matrix = (e.s0 - log_c) + (e.n - e.s0 - log_m);  // log2 units of one matrix
    int k = 0;
    // (an MLDE launch forms the same lane offsets into its compact source: both matrices obey the limit)
    const uint64_t words = mat_words(e) > mat_src_words(e) ? mat_words(e) : mat_src_words(e);
    while (one_matrix + k < log_u && (words << (k + 1)) <= ((uint64_t) 1 << MAT_MAX_LOG_WORDS)) ++k;
    return one_matrix + k < log_u ? one_matrix + k : log_u;
}

template <class Cfg>
PassGeom pass_geometry_of(const ErasedArgs &e) {
    int log_u = Cfg::LOG_U;
    if constexpr (Cfg::MAT) log_u = mat_log_u(e, Cfg::LOG_M, Cfg::LOG_C, Cfg::LOG_U);
    return pass_geometry(e.n, e.s0, Cfg::LOG_M, Cfg::LOG_C, log_u, Cfg::CONTIG, e.batch, e.target_wgs, Cfg::PPW_CAP);
}

// The kernel's argument block for this launch and geometry; false = the launch is refused.  a.tw_sc is set exactly when
// the scaled-inverse specialisation (N^-1 folded into stage 0, pass.h: fold_scale) is the kernel to run.
template <class Cfg>
bool fill_pass_args(const ErasedArgs &e, const PassGeom &g, PassArgs<Cfg> &a) {
    using W = typename Cfg::W;
    a = PassArgs<Cfg>{};
    a.in = (const W *) e.in;
    a.out = (W *) e.out;
    a.tw = (const W *) e.tw;
    a.field = make_field<typename Cfg::F>(e.field);
    a.n = e.n;
    a.s0 = e.s0;
    a.batch = e.batch;
    a.ppw = g.ppw;
    a.tp = g.tp;
    a.log_ul = g.log_ul;
    a.log_uh = g.log_uh;
    a.log_up = g.log_up;
    a.layout = e.layout;
    a.do_scale = e.do_scale;
    a.scale = (W) e.scale;
    a.dbg = e.dbg;
    a.pg_stride = 1;
    a.in2 = (const W *) e.in2;
    a.pw_scale = (W) e.pw_scale;
    a.skip_if = (const uint32_t *) e.skip_if;
    if (e.gad_levels != 0 || e.gad_log_base != 0 || e.gad_low_bits != 0) return false;  // digit parameters: the gadget middle kernels only
    // the fused expansion runs in its own kernels and nowhere else (never beside LDS-DMA or the register prefetch: PassCfg::LDE)
    if ((e.lde_beta != 0) != Cfg::LDE) return false;
    if constexpr (Cfg::LDE) {
        if (e.lde_beta < 1 || e.lde_beta > 4 || e.lde_beta >= e.n || e.s0 != 0 || !e.lde_in || !e.lde_s || e.in2) return false;
        a.lde_in = (const W *) e.lde_in;
        a.lde_s = (const W *) e.lde_s;
        a.lde_beta = e.lde_beta;
    }
    // ... and so does the vector sweep of a coset interpolation (PassCfg::CINV): refused on any other configuration, and a twin
    // is refused without its vector; N^-1 is inside the vector, so such a launch is never a scaled one
    if ((e.cinv_u != nullptr) != Cfg::CINV) return false;
    if constexpr (Cfg::CINV) {
        if (e.s0 != 0 || e.do_scale || e.tw_sc || e.in2) return false;
        a.cinv_u = (const W *) e.cinv_u;
    }
    // ... and the matrix addressing (PassCfg::MAT): its three arguments are refused on any other configuration, a twin is refused
    // without them or with anything a column pass over matrices does not do
    if ((e.mat_w != 0 || e.mat_pitch != 0 || e.mat_width != 0) != Cfg::MAT) return false;
    if constexpr (Cfg::MAT) {
        if (e.mat_w < Cfg::LOG_C || e.mat_w > e.s0 || e.s0 + Cfg::LOG_M > e.n || e.n > MAT_MAX_LOG_WORDS) return false;
        if (e.mat_width == 0 || e.mat_width > e.mat_pitch || e.mat_width > (1u << e.mat_w)) return false;
        if (mat_words(e) > ((uint64_t) 1 << MAT_MAX_LOG_WORDS)) return false;
        if (e.layout != LAYOUT_NATURAL || e.in2 || e.tw_sc || (e.do_scale && !(Cfg::INV && e.s0 == e.mat_w))) return false;
        a.mat_w = e.mat_w;
        a.mat_pitch = e.mat_pitch;
        a.mat_width = e.mat_width;
    }
    // ... and the coset twins of the matrix pass: their operands are refused on any other configuration, a twin is refused without
    // them, on a pass that does not hold stage 0 (s0 != mat_w), and -- the scaling twin, whose vector contains N^-1 -- as a scaled launch
    if ((e.mat_lde_beta != 0 || e.mat_lde_in || e.mat_lde_s || e.mat_src_pitch != 0) != Cfg::MLDE) return false;
    if constexpr (Cfg::MLDE) {
        if (e.mat_lde_beta < 1 || e.mat_lde_beta > 4 || e.mat_lde_beta >= e.n - e.mat_w || e.s0 != e.mat_w || !e.mat_lde_in || !e.mat_lde_s) return false;
        if (e.mat_width > e.mat_src_pitch || mat_src_words(e) > ((uint64_t) 1 << MAT_MAX_LOG_WORDS)) return false;
        a.lde_in = (const W *) e.mat_lde_in;
        a.lde_s = (const W *) e.mat_lde_s;
        a.lde_beta = e.mat_lde_beta;
        a.mat_src_pitch = e.mat_src_pitch;
    }
    if ((e.mat_cinv_u != nullptr) != Cfg::MCINV) return false;
    if constexpr (Cfg::MCINV) {
        if (e.s0 != e.mat_w || e.do_scale) return false;
        a.cinv_u = (const W *) e.mat_cinv_u;
    }
    if constexpr (fold_scale<Cfg>()) {
        if (e.do_scale && e.tw_sc == nullptr) return false;  // these kernels have no scaling sweep
        if (e.do_scale) a.tw_sc = (const W *) e.tw_sc;        // N^-1 rides on stage 0
    }
#if defined(NTT_PHASE_STAMPS)
    a.stamps = (unsigned long long *) e.stamps;
    a.stamp_records = e.stamp_records;
#endif
    return true;
}

// ---- the fused middle pass of the negacyclic product (pass.h: run_product_pass) ------------------------------------
// fn(CfgTag<PC>{}), PC = ProductCfg / ProductCfgM32 of the unit size: every size with a kernel.  8-byte words 2^7 .. 2^12;
// 4-byte words 2^5 .. 2^13
template <class F, class Fn>
bool product_dispatch(int log_m, Fn &&fn) {
    if constexpr (sizeof(typename F::W) == 4) return with_log_m<5, 13>(log_m, [&](auto m) { fn(CfgTag<ProductCfgM32<decltype(m)::value>>{}); });
    else return with_log_m<7, 12>(log_m, [&](auto m) { fn(CfgTag<ProductCfg<decltype(m)::value, F>>{}); });
}
// ... and the sizes ntt_polymul_negacyclic takes it at.  (The 4-byte 2^5 unit has a kernel, which the host-model test runs, but
// its register loads and stores move 8 bytes per polynomial at a time: 3.9 ms per GiB of operands against 1.4 ms for the three
// separate launches, whose small units are staged through LDS -- tools/polymul_small.py)
inline bool product_mid_used(const FieldParams &fp, int log_m) { return fp.kind == FK_M32 ? log_m >= 6 && log_m <= 13 : log_m >= 7 && log_m <= 12; }

template <class PC>
PassGeom product_geometry(int n, uint32_t batch, uint32_t target_wgs) {
    return pass_geometry(n, 0, PC::CI::LOG_M, 0, PC::CI::LOG_U, true, batch, target_wgs);
}
// does the product launch of this unit size cover `batch` polynomials in one grid (blockIdx.y <= 65535)?  The SAME geometry call
// the launcher makes -- the pre-check of ntt_polymul_negacyclic goes through here, so the two cannot disagree
inline bool product_mid_fits(const FieldParams &fp, int log_m, int n, uint32_t batch, uint32_t target_wgs) {
    return with_field(fp, [&](auto f) {
        bool fits = false;
        product_dispatch<decltype(f)>(log_m, [&](auto tag) { fits = product_geometry<typename decltype(tag)::Cfg>(n, batch, target_wgs).grid_y <= 65535u; });
        return fits;
    });
}

// The summed middle of ntt_polymul_dot_pre (pass.h: run_product_dot_pass) has a kernel for every unit size of product_dispatch but two:
// the general 64-bit modulus at 2^10 and 4-byte words at 2^13.  Their prepared twins sit at 125 and 128 VGPRs, and the term loop's
// extra live state tips the register allocator into 20 bytes of scratch under the same 128-VGPR bound; a kernel
// is not shipped with spills, so those two sizes take the path of the sizes without a fused middle.
template <class F>
constexpr bool product_dot_unit(int log_m) {
    return !(std::is_same<F, FieldM64>::value && log_m == 10) && !(std::is_same<F, FieldM32>::value && log_m == 13);
}
template <class F, class Fn>
bool product_dot_dispatch(int log_m, Fn &&fn) {
    bool found = false;
    product_dispatch<F>(log_m, [&](auto tag) {
        if constexpr (product_dot_unit<F>(decltype(tag)::Cfg::CI::LOG_M)) {
            fn(tag);
            found = true;
        }
    });
    return found;
}
// ... and the sizes ntt_polymul_dot_pre takes it at: those of product_mid_used that have such a kernel
inline bool product_dot_used(const FieldParams &fp, int log_m) {
    return product_mid_used(fp, log_m) && with_field(fp, [&](auto f) { return product_dot_unit<decltype(f)>(log_m); });
}

// what a launch of the summed middle (run_product_dot_pass) must carry: shared by the GPU launcher and the host model
inline bool product_no_digits(const ErasedArgs &e) { return e.gad_levels == 0 && e.gad_log_base == 0 && e.gad_low_bits == 0; }
inline bool product_dot_args_ok(const ErasedArgs &e) {
    const uint64_t row = (uint64_t) 1 << e.n;
    return product_no_digits(e) && e.dot_terms > 0 && e.in2_prepared && e.dot_in_stride == (uint64_t) e.batch * row && e.dot_in2_stride == (e.in2_broadcast ? row : (uint64_t) e.batch * row);
}

// The two-output summed middle of ntt_polymul_matvec_pre (pass.h: run_product_mv_pass): which units of product_dot_dispatch have such a
// kernel.  It holds two E-word accumulators beside x, so it is built under a launch bound of its own (product_kernel.inc:
// NTT_PRODUCT_MV_WPE, 3 waves per SIMD); a unit whose kernel needs scratch even there is excluded here and runs one summed launch per
// output instead (register table and the A/B that decides per word class: DESIGN.md section 3.2).  The two units without a summed
// kernel have none of this kind either: an odd number of outputs ends in a summed launch.
// Goldilocks: every unit compiles without scratch, but the A/B rule -- the pair faster than two summed launches in EVERY burst at EVERY
// shape of the class -- failed at one shape (2^12 x 4096 per row: one burst of the pair at 1.091 ms against 1.082 ms;
// profiles/polymul_matvec_ab.txt), so the product library does not use the two-output kernel for that class.  The experiment build
// keeps it, so that tools/bench_polymul_matvec.py can measure it again (legs Ax and C).  Those six kernels are stepped by the host model
// compiled as the experiment build (tests/emu_product_mv_lib.py: lib(experiment=True)); on the GPU only the tool's sampled rows check them.
template <class F>
constexpr bool product_mv_unit(int log_m) {
#if !defined(NTT_EXPERIMENT)
    if (std::is_same<F, FieldGL>::value) return false;
#endif
    return product_dot_unit<F>(log_m);
}
template <class F, class Fn>
bool product_mv_dispatch(int log_m, Fn &&fn) {
    bool found = false;
    product_dispatch<F>(log_m, [&](auto tag) {
        if constexpr (product_mv_unit<F>(decltype(tag)::Cfg::CI::LOG_M)) {
            fn(tag);
            found = true;
        }
    });
    return found;
}
inline bool product_mv_used(const FieldParams &fp, int log_m) {
    return product_dot_used(fp, log_m) && with_field(fp, [&](auto f) { return product_mv_unit<decltype(f)>(log_m); });
}

// what a launch of the two-output summed middle must carry: a summed launch for output 0, and the strides to output 1
inline bool product_mv_args_ok(const ErasedArgs &e) {
    return product_dot_args_ok(e) && e.mv_outs == 2 && e.mv_in2_stride == (uint64_t) e.dot_terms * e.dot_in2_stride &&
           e.mv_out_stride == (uint64_t) e.batch << e.n;
}

// The digit variants of the two summed middle kernels (ntt_polymul_gadget_pre; pass.h: run_product_dot_pass / run_product_mv_pass with
// GAD): which units of product_dot_dispatch have them.  Every unit compiles without scratch under its family's launch bound (register
// table: DESIGN.md section 3.2); one that did not would be excluded here and take the decomposition kernel and the unfused digits, as the
// two units without a summed kernel do.  The two-output digit variant is used exactly where product_mv_unit allows the two-output kernel.
// The A/B rule -- the fused call faster than decomposition kernel + ntt_polymul_matvec_pre in EVERY burst at EVERY shape of the class
// (profiles/polymul_gadget_ab.txt) -- held for the general 64-bit modulus (0.95-0.99x) and failed for Goldilocks (0.96-0.99x in the
// medians, but bursts overlap at three of six shapes) and for 4-byte words (1.09-1.15x at 2^10 and 2^11: slower), so the product library
// uses the digit kernels for the general 64-bit modulus only.  The experiment build keeps all of them, so that
// tools/bench_polymul_gadget.py can measure them again; the host model compiled as the experiment build steps them
// (tests/emu_product_gadget_lib.py: lib(experiment=True)).
template <class F>
constexpr bool product_gadget_unit(int log_m) {
#if !defined(NTT_EXPERIMENT)
    if (!std::is_same<F, FieldM64>::value) return false;
#endif
    return product_dot_unit<F>(log_m);
}
template <class F, class Fn>
bool product_gadget_dispatch(int log_m, Fn &&fn) {
    bool found = false;
    product_dispatch<F>(log_m, [&](auto tag) {
        if constexpr (product_gadget_unit<F>(decltype(tag)::Cfg::CI::LOG_M)) {
            fn(tag);
            found = true;
        }
    });
    return found;
}
inline bool product_gadget_used(const FieldParams &fp, int log_m) {
    return product_dot_used(fp, log_m) && with_field(fp, [&](auto f) { return product_gadget_unit<decltype(f)>(log_m); });
}

// what a launch of a digit kernel must carry: a summed launch (or a two-output one) over dot_terms = polys * gad_levels terms, and
// digit parameters that obey the argument rule
inline bool product_gadget_args_ok(const ErasedArgs &e) {
    if (e.gad_levels <= 0 || e.dot_terms <= 0 || e.dot_terms % e.gad_levels != 0 || !gadget_params_ok(e.field.p, e.gad_log_base, e.gad_levels, e.gad_low_bits)) return false;
    ErasedArgs plain = e;
    plain.gad_log_base = plain.gad_levels = plain.gad_low_bits = 0;
    return e.mv_outs != 0 ? product_mv_args_ok(plain) : product_dot_args_ok(plain);
}

// one leg of the product launch: the inverse pass of an operand (in, no out) or the forward pass of the product (out, no in)
template <class Cfg>
PassArgs<Cfg> product_leg(const ErasedArgs &e, const PassGeom &g, const void *in, void *out, const void *tw, int layout) {
    using W = typename Cfg::W;
    PassArgs<Cfg> a{};
    a.in = (const W *) in;
    a.out = (W *) out;
    a.tw = (const W *) tw;
    a.field = make_field<typename Cfg::F>(e.field);
    a.n = e.n;
    a.batch = e.batch;
    a.ppw = g.ppw;
    a.tp = g.tp;
    a.log_ul = g.log_ul;
    a.log_uh = g.log_uh;
    a.log_up = g.log_up;
    a.layout = layout;
    a.pg_stride = 1;
    return a;
}
// aa: inverse leg of operand e.in (operand e.in2: the same block with that `in`); af: forward leg, product * pw_scale -> e.out
template <class PC>
void fill_product_args(const ErasedArgs &e, const PassGeom &g, PassArgs<typename PC::CI> &aa, PassArgs<typename PC::CF> &af) {
    aa = product_leg<typename PC::CI>(e, g, e.in, nullptr, e.tw, LAYOUT_NATURAL);
    af = product_leg<typename PC::CF>(e, g, nullptr, e.out, e.tw2, e.layout);
    af.pw_scale = (typename PC::CF::W) e.pw_scale;
}

}  // namespace ntt
