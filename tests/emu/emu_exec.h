// emu_exec.h -- the stepping part of the host index model, shared by emu.cpp and emu_lde.cpp: the LDS hazard tracker, the
// executors that step every thread context of a workgroup phase by phase (the role __syncthreads() plays on the GPU), and
// one function that runs a pass -- or the product's fused middle pass -- over its whole grid with the argument block the GPU
// launcher fills (csrc/launch.h: fill_pass_args / fill_product_args).  TEST INFRASTRUCTURE.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define NTT_EMU_TRACK 1
#include "../../ntt_aie_amd/csrc/launch.h"

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

}  // namespace emu
