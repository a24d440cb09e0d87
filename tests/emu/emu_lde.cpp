// emu_lde.cpp -- host index model of ntt_lde's fused first pass (pass.h: PassCfg::LDE, phase_lde_*).
//
// TEST INFRASTRUCTURE, a sibling of emu.cpp: the same pass.h / plan.h / field.h the HIP kernels are built from, under g++, every
// thread context of a workgroup stepped phase by phase, with the LDS hazard tracker on.  The first pass is the configuration
// lde_dispatch() names -- the rule the launcher itself uses (pass_kernel.inc) -- and the column passes behind it are the plain
// ones, so a whole low-degree extension runs here exactly as ntt_lde sequences it.
//   * as a library (tests/emu_lde_lib.py): emu_lde() on the caller's buffers;
//   * with -DEMU_LDE_MAIN (tests/test_lde_emu_asan.py, built with ASan + UBSan and linked with oracle/ntt_oracle.c): a sweep over
//     word classes x logM 5..17 x blow-up 1..4 x ragged batches x both layouts x every plan alternative on malloc() buffers of
//     EXACTLY batch * N input words, batch * M output words and max(N, 4) coset words, each case compared with the oracle's
//     network applied to the expanded input.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define NTT_EMU_TRACK 1
#include "../../ntt_aie_amd/csrc/pass.h"
#include "../../ntt_aie_amd/csrc/plan.h"

using namespace ntt;
using namespace ntt::host;

// which fields this translation unit instantiates (bit 0 Goldilocks, 1 general 64-bit, 2 4-byte words): the sanitizer test compiles
// one executable per field so that the instrumented builds run in parallel; a call into an absent field returns -100
#ifndef EMU_LDE_FIELDS
#define EMU_LDE_FIELDS 7
#endif

namespace {

// LDS hazard tracker, as in emu.cpp: a word may be read by a wave only if its last write is the wave's own or older than the
// last workgroup barrier, and written only if every read since that barrier was the wave's own
struct Track : ntt::LdsTrack {
    struct St {
        int w_wave = -1, w_epoch = -1, r_wave = -1, r_epoch = -1;
    };
    std::vector<St> st;
    const char *base = nullptr;
    size_t wb = 1;
    int epoch = 0;
    void reset(const void *tile, size_t words, size_t word_bytes) {
        base = (const char *) tile;
        wb = word_bytes;
        st.assign(words, St());
        epoch = 0;
    }
    void access(const void *word, uint32_t tid, bool write) override {
        const int wave = (int) (tid >> 6);
        const size_t idx = (size_t) ((const char *) word - base) / wb;
        if ((const char *) word < base || idx >= st.size()) return;
        St &s = st[idx];
        const bool raw = s.w_epoch == epoch && s.w_wave != wave && s.w_wave != -1;
        const bool war = write && s.r_epoch == epoch && s.r_wave != wave && s.r_wave != -1;
        if (raw || war) {
            fprintf(stderr, "LDS hazard: wave %d %s a word another wave touched since the last workgroup barrier\n", wave, write ? "writes" : "reads");
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
struct Exec {
    static constexpr bool early_ok = true;
    std::vector<Ctx<Cfg>> ctx;
    std::vector<typename Cfg::W> tile;
    uint32_t bx = 0, by = 0;
    Track tr;
    Exec() : ctx(Cfg::NT), tile(Cfg::DMA ? 2 * Cfg::TILE_WORDS : Cfg::LDS_WORDS) {}
    void init(const PassArgs<Cfg> &a) {
        for (int t = 0; t < Cfg::NT; t++) phase_init<Cfg>(ctx[t], a, (uint32_t) t, bx, by);
    }
    void init_indices(const PassArgs<Cfg> &a) {
        for (int t = 0; t < Cfg::NT; t++) phase_init<Cfg, false>(ctx[t], a, (uint32_t) t, bx, by);
    }
    template <class Fn>
    void each(Fn &&f) {
        for (int t = 0; t < Cfg::NT; t++) f(ctx[t]);
    }
    void sync(std::false_type) { ++tr.epoch; }
    void sync(std::true_type) {}
    uint32_t pg_base() const { return ctx[0].pg_base; }
    int ppw() const { return ctx[0].ppw; }
    bool iter_begin(int) { return true; }
    void iter_done(int) {}
    void pass_done(int) {}
    typename Cfg::W *lds() { return tile.data(); }
};

struct Job {
    int wb, logn, beta, layout;
    uint64_t p;
    uint32_t batch, target_wgs;
    const void *tw;   // size-M forward table, table form
    const void *sv;   // coset vector, table form, max(N, 4) words
    const void *in;   // [batch][N]
    void *out;        // [batch][M]
};

template <class F>
F field_of(const Job &j);
template <>
FieldGL field_of<FieldGL>(const Job &) {
    return FieldGL{};
}
template <>
FieldM32 field_of<FieldM32>(const Job &j) {
    return FieldM32{(uint32_t) j.p, mont_pinv((uint32_t) j.p), mont_r2((uint32_t) j.p)};
}
template <>
FieldM64 field_of<FieldM64>(const Job &j) {
    return FieldM64{j.p, mont_pinv64(j.p), mont_r2_64(j.p)};
}

template <class Cfg>
void run_one(const Job &j, const PassDesc &pd, bool lde) {
    using W = typename Cfg::W;
    PassArgs<Cfg> a;
    memset((void *) &a, 0, sizeof(a));
    a.in = lde ? nullptr : (const W *) j.out;  // the fused pass must not read `in` at all
    a.out = (W *) j.out;
    a.tw = (const W *) j.tw;
    a.field = field_of<typename Cfg::F>(j);
    a.n = j.logn;
    a.s0 = pd.s0;
    a.batch = j.batch;
    a.layout = j.layout;
    a.pg_stride = 1;
    if (lde) {
        a.lde_in = (const W *) j.in;
        a.lde_s = (const W *) j.sv;
        a.lde_beta = j.beta;
    }
    const PassGeom g = pass_geometry(j.logn, pd.s0, Cfg::LOG_M, Cfg::LOG_C, Cfg::LOG_U, Cfg::CONTIG, j.batch, j.target_wgs, Cfg::PPW_CAP);
    a.ppw = g.ppw;
    a.tp = g.tp;
    a.log_ul = g.log_ul;
    a.log_uh = g.log_uh;
    a.log_up = g.log_up;
    Exec<Cfg> ex;
    for (uint32_t by = 0; by < g.grid_y; by++)
        for (uint32_t bx = 0; bx < g.grid_x; bx++) {
            ex.bx = bx;
            ex.by = by;
            memset(ex.tile.data(), 0xA5, ex.tile.size() * sizeof(W));  // a word nobody wrote shows up as garbage
            ex.tr.reset(ex.tile.data(), ex.tile.size(), sizeof(W));
            ntt::lds_track() = &ex.tr;
            run_pass<Cfg>(ex, a);
            ntt::lds_track() = nullptr;
        }
}

template <class F>
int run_lde(const Job &j, const std::vector<PassDesc> &passes) {
    for (const PassDesc &pd : passes) {
        if (&pd == &passes.front()) {
            if (!pd.contig || pd.s0 != 0) return -1;
            if (!lde_dispatch<F>(pd.log_m, pd.log_m == j.logn, [&](auto tag) { run_one<typename decltype(tag)::Cfg>(j, pd, true); })) return -2;
            continue;
        }
        switch (pd.log_m) {
            case 4: run_one<ColPassCfg<F, 4, false>>(j, pd, false); break;
            case 5: run_one<ColPassCfg<F, 5, false>>(j, pd, false); break;
            case 6: run_one<ColPassCfg<F, 6, false>>(j, pd, false); break;
            case 7: run_one<ColPassCfg<F, 7, false>>(j, pd, false); break;
            case 8: run_one<ColPassCfg<F, 8, false>>(j, pd, false); break;
            case 9: run_one<ColPassCfg<F, 9, false>>(j, pd, false); break;
            default: return -3;
        }
    }
    return 0;
}

}  // namespace

extern "C" {

// number of launch-time alternatives of the size-2^logn plan (plan.h: plan_alternatives)
int emu_lde_alternatives(int word_bytes, int logn, uint64_t p) { return (int) plan_alternatives(logn, word_bytes, p).size(); }

// One low-degree extension as ntt_lde runs it from logn = 5 on: fused first pass, then the plain column passes, in place on `out`.
// T_plain: the size-2^logn table, plain residues; in: [batch][2^(logn - beta)]; out: [batch][2^logn]; alt: plan alternative, -1 = by batch.
int emu_lde(int word_bytes, int logn, uint64_t p, const void *T_plain, int beta, uint64_t shift, const void *in, void *out,
            uint32_t batch, int layout, uint32_t target_wgs, int alt) {
    if (logn < LDE_MIN_LOG_M || beta < 1 || beta > 4 || beta >= logn || shift == 0 || shift >= p) return -1;
    const size_t M = (size_t) 1 << logn, N = M >> beta;
    const int logN = logn - beta;
    void *tw = malloc(M * (size_t) word_bytes);
    const size_t s_words = N < 4 ? 4 : N;
    void *sv = malloc(s_words * (size_t) word_bytes);
    if (!tw || !sv) abort();
    for (size_t i = 0; i < M; i++) {
        if (word_bytes == 4) ((uint32_t *) tw)[i] = (uint32_t) to_table_form(((const uint32_t *) T_plain)[i], p, 4);
        else ((uint64_t *) tw)[i] = to_table_form(((const uint64_t *) T_plain)[i], p, 8);
    }
    for (size_t i = 0; i < s_words; i++) {  // ntt_plan_set_coset's vector: shift^bitrev_logN(i mod N), periodic up to 4 words
        const uint64_t v = to_table_form(powmod(shift, bitrev(i & (N - 1), logN), p), p, word_bytes);
        if (word_bytes == 4) ((uint32_t *) sv)[i] = (uint32_t) v;
        else ((uint64_t *) sv)[i] = v;
    }
    const std::vector<PlanAlt> alts = plan_alternatives(logn, word_bytes, p);
    const int k = alt >= 0 ? alt : select_alternative(alts, batch);
    int rc = -4;
    if (k < (int) alts.size()) {
        const Job j{word_bytes, logn, beta, layout, p, batch, target_wgs, tw, sv, in, out};
        const std::vector<PassDesc> &passes = alts[(size_t) k].passes;
        rc = -100;
#if EMU_LDE_FIELDS & 1
        if (word_bytes == 8 && p == GOLDILOCKS) rc = run_lde<FieldGL>(j, passes);
#endif
#if EMU_LDE_FIELDS & 2
        if (word_bytes == 8 && p != GOLDILOCKS) rc = run_lde<FieldM64>(j, passes);
#endif
#if EMU_LDE_FIELDS & 4
        if (word_bytes == 4) rc = run_lde<FieldM32>(j, passes);
#endif
    }
    free(tw);
    free(sv);
    return rc;
}

}  // extern "C"

#if defined(EMU_LDE_MAIN)
#include "../../oracle/ntt_oracle.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct Class {
    const char *name;
    int wb;
    uint64_t p, g;
};

// one case on exact-size buffers; returns 0 when every word equals the oracle's
int one_case(const Class &c, int logn, int beta, uint32_t batch, int layout, int alt, uint64_t shift) {
    const size_t M = (size_t) 1 << logn, N = M >> beta;
    const size_t wb = (size_t) c.wb;
    std::vector<uint64_t> T64(M);
    if (oracle_make_table_u64(1, M, T64.data(), c.p, c.g) != 0) return 0;  // 2^logn does not divide p - 1: no such case
    void *T = malloc(M * wb), *in = malloc((size_t) batch * N * wb), *out = malloc((size_t) batch * M * wb), *want = malloc((size_t) batch * M * wb);
    if (!T || !in || !out || !want) abort();
    for (size_t i = 0; i < M; i++) {
        if (c.wb == 4) ((uint32_t *) T)[i] = (uint32_t) T64[i];
        else ((uint64_t *) T)[i] = T64[i];
    }
    memset(want, 0, (size_t) batch * M * wb);
    memset(out, 0xEE, (size_t) batch * M * wb);
    for (size_t b = 0; b < batch; b++)
        for (size_t i = 0; i < N; i++) {
            const uint64_t r = rnd();
            const uint64_t x = (r & 15) == 0 ? 0 : (r & 15) == 1 ? c.p - 1 : (r >> 4) % c.p;  // 0 and p - 1 among the inputs
            const uint64_t sx = mulmod(x, powmod(shift, bitrev(i, logn - beta), c.p), c.p);
            if (c.wb == 4) {
                ((uint32_t *) in)[b * N + i] = (uint32_t) x;
                ((uint32_t *) want)[b * M + (i << beta)] = (uint32_t) sx;
            } else {
                ((uint64_t *) in)[b * N + i] = x;
                ((uint64_t *) want)[b * M + (i << beta)] = sx;
            }
        }
    if (c.wb == 4) oracle_ntt_batch_u32((uint32_t *) want, (uint32_t) M, batch, (const uint32_t *) T, (uint32_t) c.p, 1);
    else oracle_ntt_batch_u64((uint64_t *) want, M, batch, (const uint64_t *) T, c.p, 1);
    if (layout) {
        void *tmp = malloc((size_t) batch * M * wb);
        if (!tmp) abort();
        for (size_t b = 0; b < batch; b++) {
            if (c.wb == 4) oracle_block16_u32((uint32_t *) tmp + b * M, (const uint32_t *) want + b * M, (uint32_t) M);
            else oracle_block16_u64((uint64_t *) tmp + b * M, (const uint64_t *) want + b * M, M);
        }
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
    const Class classes[] = {
        {"gl", 8, GOLDILOCKS, 7},
        {"m64", 8, 0xFFFFFFFC00000001ull, 10},  // general 64-bit class: an NTT prime above 2^63 (sums wrap: the carry paths)
        {"m32", 4, 998244353ull, 3},
    };
    if (argc < 2) return 2;
    const bool quick = argc > 2;
    long cases = 0, bad = 0;
    for (const Class &c0 : classes) {
        if (strcmp(c0.name, argv[1]) != 0) continue;
        const Class &c = c0;
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
    printf("%s: %ld cases, %ld bad\n", argv[1], cases, bad);
    if (bad == 0 && cases > 0) printf("%s: %ld cases clean\n", argv[1], cases);
    return bad ? 1 : (cases ? 0 : 3);
}
#endif
