// emu_exec.h -- the stepping part of the host index model, shared by every emu*.cpp: the LDS hazard tracker, the executors that
// step every thread context of a workgroup phase by phase (the role __syncthreads() plays on the GPU), one function that runs a
// pass -- or the product's fused middle pass -- over its whole grid with the argument block the GPU launcher fills (csrc/launch.h:
// fill_pass_args / fill_product_args), run_step, which hands a step of the library's own launch list (csrc/sequence.h) to it through
// the launchers' dispatchers, and HostPlan, the plan those lists are made from.  TEST INFRASTRUCTURE.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define NTT_EMU_TRACK 1
#include "../../ntt_aie_amd/csrc/sequence.h"

namespace emu {

using namespace ntt;

// LDS hazard tracker (pass.h: NTT_LDS_ACCESS).  epoch = number of WORKGROUP barriers so far.  A word may be read by a wave
// only if its last write is this wave's own or older than the last barrier; it may be written only if, in addition, every
// read of it since the last barrier was this wave's own.  Wave-local syncs do not advance the epoch: LDS operations of one
// wave execute in order, so same-wave accesses are always fine.  A violation aborts the process (the test then fails).
struct EmuLdsTrack : ntt::LdsTrack {
    struct St {
        int w_wave = -1, w_epoch = -1, r_wave = -1, r_epoch = -1;  // r_wave -2: several waves read it in r_epoch
    };
    std::vector<St> st;
    const char *base = nullptr;
    size_t word_bytes = 1;
    int epoch = 0;
    const char *what = "";
    void reset(const void *tile, size_t words, size_t wb) {  // a new workgroup
        base = (const char *) tile;
        word_bytes = wb;
        st.assign(words, St());
        epoch = 0;
    }
    void barrier() { ++epoch; }
    void access(const void *word, uint32_t tid, bool write) override {
        const int wave = (int) (tid >> 6);
        const size_t idx = (size_t) ((const char *) word - base) / word_bytes;
        if ((const char *) word < base || idx >= st.size()) return;  // not the tile (the product pass's twiddle tables)
        St &s = st[idx];
        const bool raw = s.w_epoch == epoch && s.w_wave != wave && s.w_wave != -1;
        const bool war = write && s.r_epoch == epoch && s.r_wave != wave && s.r_wave != -1;
        if (raw || war) {
            fprintf(stderr, "LDS hazard in %s: wave %d %s a word that wave %d %s since the last workgroup barrier (epoch %d)\n", what, wave,
                    write ? "writes" : "reads", raw ? s.w_wave : s.r_wave, raw ? "wrote" : "read", epoch);
            abort();
        }
        if (write) {
            s.w_wave = wave;
            s.w_epoch = epoch;
        } else if (s.r_epoch == epoch && s.r_wave != wave) {
            s.r_wave = -2;
        } else {
            s.r_wave = wave;
            s.r_epoch = epoch;
        }
    }
};

template <class Cfg>
struct EmuExec {
    static constexpr bool early_ok = true;
    std::vector<Ctx<Cfg>> ctx;
    std::vector<typename Cfg::W> tile;
    uint32_t bx, by;
    EmuExec() : ctx(Cfg::NT), tile(Cfg::DMA ? 2 * Cfg::TILE_WORDS : Cfg::LDS_WORDS) {}
    void init(const PassArgs<Cfg> &a) {
        for (int t = 0; t < Cfg::NT; t++) phase_init<Cfg>(ctx[t], a, (uint32_t) t, bx, by);
    }
    void init_indices(const PassArgs<Cfg> &a) {
        for (int t = 0; t < Cfg::NT; t++) phase_init<Cfg, false>(ctx[t], a, (uint32_t) t, bx, by);
    }
    // only_wave >= 0: step just that wave's 64 lanes (used to prove WAVE_LOCAL passes never read
    // another wave's LDS words: the four waves are then run one after the other, start to finish)
    int only_wave = -1;
    template <class Fn>
    void each(Fn &&f) {
        const int lo = only_wave < 0 ? 0 : 64 * only_wave, hi = only_wave < 0 ? Cfg::NT : lo + 64;
        for (int t = lo; t < hi; t++) f(ctx[t]);
    }
    EmuLdsTrack tr;
    void sync(std::false_type) { tr.barrier(); }
    void sync(std::true_type) {}
    uint32_t pg_base() const { return ctx[0].pg_base; }
    int ppw() const { return ctx[0].ppw; }
    bool iter_begin(int) { return true; }
    void iter_done(int) {}
    void pass_done(int) {}
    typename Cfg::W *lds() { return tile.data(); }
};

// host twin of GpuProductExec (product_kernel.inc): all contexts of the workgroup stepped phase by phase
template <class CI, class CF>
struct EmuProductExec {
    using W = typename CI::W;
    std::vector<Ctx<CI>> ci;
    std::vector<Ctx<CF>> cf;
    std::vector<W> keep, pre, tile, tab_i, tab_f;
    uint32_t bx, by;
    int only_wave = -1;
    EmuProductExec()
        : ci(CI::NT), cf(CI::NT), keep((size_t) CI::NT * CI::E), pre((size_t) CI::NT * CI::E), tile(CI::LDS_WORDS),
          tab_i(tw_table_words<CI>()), tab_f(tw_table_words<CF>()) {}
    void init(const PassArgs<CI> &aa, const PassArgs<CF> &af) {
        for (int t = 0; t < CI::NT; t++) {
            phase_init<CI>(ci[t], aa, (uint32_t) t, bx, by);
            phase_init<CF>(cf[t], af, (uint32_t) t, bx, by);
        }
    }
    int lo() const { return only_wave < 0 ? 0 : 64 * only_wave; }
    int hi() const { return only_wave < 0 ? CI::NT : 64 * only_wave + 64; }
    template <class Fn>
    void eachI(Fn &&f) { for (int t = lo(); t < hi(); t++) f(ci[t]); }
    template <class Fn>
    void eachF(Fn &&f) { for (int t = lo(); t < hi(); t++) f(cf[t]); }
    template <class Fn>
    void eachIF(Fn &&f) { for (int t = lo(); t < hi(); t++) f(ci[t], cf[t], &keep[(size_t) t * CI::E], &pre[(size_t) t * CI::E]); }
    EmuLdsTrack tr;
    void sync(std::false_type) { tr.barrier(); }
    void sync(std::true_type) {}
    uint32_t pg_base() const { return ci[0].pg_base; }
    int ppw() const { return ci[0].ppw; }
    W *lds() { return tile.data(); }
    W *tabI() { return tab_i.data(); }
    W *tabF() { return tab_f.data(); }
};

// One pass launch on the host: every workgroup of the launcher's grid, with the launcher's argument block.  `track`: the LDS
// hazard tracker is on.  0, or -2 when the launcher would refuse these arguments (launch.h: fill_pass_args).
template <class Cfg>
int run_pass_launch(const ErasedArgs &e, bool track) {
    using W = typename Cfg::W;
    const PassGeom g = pass_geometry_of<Cfg>(e);
    PassArgs<Cfg> a;
    if (!fill_pass_args<Cfg>(e, g, a)) return -2;
    EmuExec<Cfg> ex;
    for (uint32_t by = 0; by < g.grid_y; by++)
        for (uint32_t bx = 0; bx < g.grid_x; bx++) {
            ex.bx = bx;
            ex.by = by;
            // poison the tile: a read of a word nobody wrote this launch shows up as garbage
            memset(ex.tile.data(), 0xA5, ex.tile.size() * sizeof(W));
            ex.tr.reset(ex.tile.data(), ex.tile.size(), sizeof(W));
            ex.tr.what = Cfg::CONTIG ? "CONTIG pass" : "column pass";
            ntt::lds_track() = track ? &ex.tr : nullptr;
            auto go = [&]() {
                if constexpr (fold_scale<Cfg>()) {
                    if (a.tw_sc != nullptr) return run_pass<Cfg, EmuExec<Cfg>, -1, true>(ex, a);  // the launcher's rule (pass_kernel.inc)
                }
                return run_pass<Cfg>(ex, a);
            };
            if constexpr (Cfg::WAVE_LOCAL) {
                for (int w = 0; w < Cfg::NT / 64; w++) {
                    ex.only_wave = w;
                    go();
                    memset(ex.tile.data(), 0x5A, ex.tile.size() * sizeof(W));  // nothing may survive
                }
            } else {
                go();
            }
            ntt::lds_track() = nullptr;
        }
    return 0;
}

// the product's fused middle pass (product_kernel.inc: launch_product): operands e.in and e.in2, tables e.tw (inverse) and e.tw2
template <class PC>
int run_product_launch(const ErasedArgs &e, bool track) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    using W = typename CI::W;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    PassArgs<CI> ab = aa;
    ab.in = (const W *) e.in2;
    EmuProductExec<CI, CF> ex;
    for (uint32_t by = 0; by < g.grid_y; by++)
        for (uint32_t bx = 0; bx < g.grid_x; bx++) {
            ex.bx = bx;
            ex.by = by;
            memset(ex.tile.data(), 0xA5, ex.tile.size() * sizeof(W));
            ex.tr.reset(ex.tile.data(), ex.tile.size(), sizeof(W));
            ex.tr.what = "product pass";
            ntt::lds_track() = track ? &ex.tr : nullptr;
            run_product_pass<CI, CF>(ex, aa, ab, af);
            ntt::lds_track() = nullptr;
        }
    return 0;
}

// ---- one step of a sequence (csrc/sequence.h), as ntt_api.hip's launch_step hands it to the GPU launchers --------------------------
// PARTS: which template families the translation unit instantiates (bit set = compiled in); a step of an absent one returns EMU_ABSENT.
//   ordinary passes   0 Goldilocks forward   1 Goldilocks inverse   2 general 64-bit forward   3 general 64-bit inverse
//                     4 4-byte forward       5 4-byte inverse
//   product middle    6 Goldilocks           7 general 64-bit       8 4-byte
//   matrix passes     9 .. 14, in the order of 0 .. 5
// The per-file masks that name FIELDS (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words) become parts through field_parts.
enum { EMU_ABSENT = -100 };
enum { PARTS_PASS = 0, PARTS_PRODUCT = 6, PARTS_MAT = 9 };
// the parts of `fields` in the group that starts at bit `base`; dirs: 1 forward, 2 inverse, 3 both
constexpr unsigned field_parts(unsigned fields, int base, unsigned dirs) {
    unsigned v = 0;
    for (int k = 0; k < 3; k++)
        if ((fields >> k) & 1) v |= dirs << (base + 2 * k);
    return v;
}

template <unsigned PARTS, class F, int K>  // K: 0 Goldilocks, 1 general 64-bit, 2 4-byte words
int run_step_of(const Step &st, bool track, int no_kernel) {
    const ErasedArgs &e = st.args;
    int rc = no_kernel;
    auto pass = [&](auto tag) { rc = run_pass_launch<typename decltype(tag)::Cfg>(e, track); };
    if (st.family == STEP_PRODUCT) {
        if constexpr ((PARTS >> (PARTS_PRODUCT + K)) & 1) product_dispatch<F>(st.log_m, [&](auto tag) { rc = run_product_launch<typename decltype(tag)::Cfg>(e, track); });
        else rc = EMU_ABSENT;
    } else if (st.family == STEP_MAT) {
        constexpr unsigned dirs = (PARTS >> (PARTS_MAT + 2 * K)) & 3;
        rc = (dirs >> (st.inverse ? 1 : 0)) & 1 ? rc : EMU_ABSENT;
        if constexpr (dirs & 1) if (!st.inverse) mat_twin_dispatch<F, false>(st.log_m, e, pass);
        if constexpr (dirs & 2) if (st.inverse) mat_twin_dispatch<F, true>(st.log_m, e, pass);
    } else {
        constexpr unsigned dirs = (PARTS >> (PARTS_PASS + 2 * K)) & 3;
        rc = (dirs >> (st.inverse ? 1 : 0)) & 1 ? rc : EMU_ABSENT;
        if constexpr (dirs & 1) if (!st.inverse) pass_dispatch<F, false>(st.contig, st.log_m, e, pass);
        if constexpr (dirs & 2) if (st.inverse) pass_dispatch<F, true>(st.contig, st.log_m, e, pass);
    }
    return rc;
}
// 0; `no_kernel` when the dispatcher names no kernel for the step; -2 when the launcher would refuse its arguments
template <unsigned PARTS>
int run_step(const Step &st, bool track, int no_kernel) {
    if (st.args.field.kind == FK_GL) return run_step_of<PARTS, FieldGL, 0>(st, track, no_kernel);
    if (st.args.field.kind == FK_M64) return run_step_of<PARTS, FieldM64, 1>(st, track, no_kernel);
    return run_step_of<PARTS, FieldM32, 2>(st, track, no_kernel);
}

// ---- a plan on the host ----------------------------------------------------------------------------------------------------------
// `count` words of the table form of value(i), in an exact-size malloc() block: a sanitizer's red zones sit where the plan's own
// device allocation would end
template <class Fn>
void *table_form_words(size_t count, int word_bytes, uint64_t p, Fn &&value) {
    void *t = malloc(count * (size_t) word_bytes);
    if (!t) abort();
    for (size_t i = 0; i < count; i++) {
        const uint64_t x = host::to_table_form(value(i), p, word_bytes);
        if (word_bytes == 4) ((uint32_t *) t)[i] = (uint32_t) x;
        else ((uint64_t *) t)[i] = x;
    }
    return t;
}

// What ntt_plan_create + ntt_plan_set_twiddles (T_plain: 2^logn plain residues) leave in a plan, and what ntt_plan_set_coset /
// ntt_plan_set_coset_inverse add.  `target` sizes the launches of both pass kinds.  `inverse`: also the inverse table and, for
// 8-byte words, the scaled stage-0 table; invertible = false when the table has an entry that is not a unit.
struct HostPlan : PlanFacts {
    bool invertible = false;
    HostPlan(int word_bytes_, int logn_, uint64_t p_, const void *T_plain, uint32_t target, bool inverse) {
        logn = logn_;
        p = p_;
        word_bytes = word_bytes_;
        field = field_params(word_bytes, p);
        ninv_plain = host::powmod(p / 2 + 1, (uint64_t) logn, p);
        scale_tf = host::to_table_form(ninv_plain, p, word_bytes);
        target_wgs = target_wgs_col = target;
        const size_t N = (size_t) 1 << logn;
        std::vector<uint64_t> T(N), Ti;
        for (size_t i = 0; i < N; i++) T[i] = word_bytes == 4 ? ((const uint32_t *) T_plain)[i] : ((const uint64_t *) T_plain)[i];
        tw_fwd = table_form_words(N, word_bytes, p, [&](size_t i) { return T[i]; });
        if (!inverse || !host::invert_table(T, p, Ti)) return;
        invertible = true;
        tw_inv = table_form_words(N, word_bytes, p, [&](size_t i) { return Ti[i]; });
        if (word_bytes == 8) tw_inv_sc = table_form_words(N / 2, 8, p, [&](size_t i) { return host::mulmod(Ti[N / 2 + i], ninv_plain, p); });
    }
    HostPlan(const HostPlan &) = delete;
    ~HostPlan() {
        for (void *b : {tw_fwd, tw_inv, tw_inv_sc, lde_s, cinv_u}) free(b);
    }
    // s[i] = shift^bitrev(i) over the N >> beta compact rows, periodic up to 4 words
    void set_coset(int beta, uint64_t shift) {
        const int ls = logn - beta;
        const size_t ns = (size_t) 1 << ls;
        free(lde_s);
        lde_s = table_form_words(ns < 4 ? 4 : ns, word_bytes, p, [&](size_t i) { return host::powmod(shift, host::bitrev(i & (ns - 1), ls), p); });
        lde_beta = beta;
    }
    // u[i] = shift^-bitrev(i) * N^-1, periodic up to 4 words; false when the shift is not a unit
    bool set_coset_inverse(uint64_t shift) {
        const uint64_t shift_inv = host::invmod(shift, p);
        if (shift_inv == 0) return false;
        const size_t N = (size_t) 1 << logn;
        free(cinv_u);
        cinv_u = table_form_words(N < 4 ? 4 : N, word_bytes, p, [&](size_t i) { return host::mulmod(host::powmod(shift_inv, host::bitrev(i & (N - 1), logn), p), ninv_plain, p); });
        cinv_set = true;
        return true;
    }
};

}  // namespace emu
