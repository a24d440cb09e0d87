// emu_negacyclic_map.cpp -- the loops of negacyclic_map_kernel (csrc/misc_kernels.hip) on the host: the kernel's body is
// negacyclic_map_thread of csrc/negacyclic_map.h, written once for device and host, and this stand-alone program runs it for every
// thread of a small grid -- the chunk loop and the word tail -- on malloc() buffers of EXACTLY polys * batch * N words of a,
// polys * (levels or 1) * batch * N words of output and batch exponents, so that AddressSanitizer sees any access outside a row, a
// block or the exponent array (tests/test_negacyclic_map_cpu.py builds it with ASan + UBSan; nothing is loaded into Python).
//
//   emu_negacyclic_map                 the sweep: word sizes 4 and 8 x four moduli x logn 1, 2, 3, 6, 10 x batches 1, 5, 33 x 1 and 2
//                                      polynomials x both flag values x the exponents 0, 1, V - 1, V, N - 1, N, N + 1, 2N - 1, 2N, 2^32 - 1
//                                      and a per-row random array x g in 1, 3, 5, N + 1, 2N - 1 x no digits, a 3-level and a 1-level
//                                      set, each compared with a reference that does NOT use the gather rule: a SCATTER from the ring
//                                      definition (coefficient i goes to exponent i + e, or i * g, mod 2N; an exponent N + d is -X^d),
//                                      the subtraction and the digits in 128-bit integers from the definition of include/ntt_hip.h.
//                                      Prints "negacyclic map: <count> cases clean".
//   emu_negacyclic_map dump wb p logn batch polys kind param perrow flags w K l seed file
//                                      one case, written for the Python reference to compare: a, the exponents, the mapped words,
//                                      the digits (K > 0), as raw little-endian words in that order.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../ntt_aie_amd/csrc/negacyclic_map.h"

using namespace ntt;

namespace {

typedef __int128 i128;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// digit k of the canonical word a, from the definition in integers
uint64_t digit_def(uint64_t a, uint64_t p, int w, int K, int l, int k) {
    const bool neg = a > (p - 1) / 2;
    const i128 m = neg ? (i128) p - a : (i128) a;
    const i128 h = l > 0 ? (i128) 1 << (l - 1) : 0;
    i128 v = (m + h) >> l;
    for (int i = 0; i + 1 < K; ++i) v += (i128) 1 << (i * w + w - 1);
    i128 e = k < K - 1 ? ((v >> (k * w)) & (((i128) 1 << w) - 1)) - ((i128) 1 << (w - 1)) : v >> ((K - 1) * w);
    if (neg) e = -e;
    e %= (i128) p;
    if (e < 0) e += p;
    return (uint64_t) e;
}

// one row by SCATTER from the ring definition, then minus the row itself
template <class W>
void ref_row(const W *row, W *y, int logn, int kind, uint32_t param, int minus_identity, uint64_t p) {
    const uint64_t n = (uint64_t) 1 << logn;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t d = kind == MAP_MONOMIAL ? (i + (uint64_t) param % (2 * n)) % (2 * n) : (i * (uint64_t) param) % (2 * n);
        const uint64_t x = row[i];
        y[d % n] = (W) (d >= n && x != 0 ? p - x : x);
    }
    if (minus_identity)
        for (uint64_t j = 0; j < n; ++j) y[j] = (W) (uint64_t) ((((i128) y[j] - (i128) row[j]) % (i128) p + (i128) p) % (i128) p);
}

struct Case {
    int wb, logn, kind, flags, w, K, l;  // K == 0: the map alone
    uint64_t p;
    size_t batch, polys;
    uint32_t param;
    bool perrow;
};

template <class W>
struct Buffers {
    W *a = nullptr, *out = nullptr, *mapped = nullptr;  // mapped: the reference's words, [polys][batch][N]
    uint32_t *exps = nullptr;
    ~Buffers() {
        free(a);
        free(out);
        free(mapped);
        free(exps);
    }
};

// the kernel's launch on the host: every polynomial (blockIdx.y), every thread of a grid that is deliberately no divisor of anything
template <class W>
void run_kernel(const Case &c, const W *a, W *out, const uint32_t *exps) {
    const size_t block = c.batch << c.logn, threads = 37;
    const uint32_t q = c.kind == MAP_AUTOMORPHISM ? map_ginv(c.param, c.logn) : c.param;
    const MapArgs m{c.kind, c.logn, q, exps, c.flags & MAP_MINUS_IDENTITY, c.p, GadgetParams{c.w, c.K, c.l}};
    auto store16 = [](W *dst, size_t ch, const MapChunk<W> &x) { memcpy(dst + ch * (16 / sizeof(W)), &x, 16); };
    for (size_t y = 0; y < c.polys; ++y)
        for (size_t t = 0; t < threads; ++t) {
            if (c.K)
                negacyclic_map_thread<W, true>(a + y * block, out + y * (size_t) c.K * block, block, m, t, threads, store16);
            else
                negacyclic_map_thread<W, false>(a + y * block, out + y * block, block, m, t, threads, store16);
        }
}

template <class W>
bool fill_and_run(const Case &c, Buffers<W> &b) {
    const size_t n = (size_t) 1 << c.logn, block = c.batch * n, lv = c.K ? c.K : 1;
    b.a = (W *) malloc(c.polys * block * sizeof(W));
    b.out = (W *) malloc(c.polys * lv * block * sizeof(W));
    b.mapped = (W *) malloc(c.polys * block * sizeof(W));
    if (c.perrow) b.exps = (uint32_t *) malloc(c.batch * sizeof(uint32_t));
    if (!b.a || !b.out || !b.mapped || (c.perrow && !b.exps)) return false;
    const uint64_t edge[5] = {0, 1 % c.p, (c.p - 1) / 2, (c.p + 1) / 2, c.p - 1};
    for (size_t i = 0; i < c.polys * block; ++i) b.a[i] = (W) (rnd() % c.p);
    for (size_t y = 0; y < c.polys; ++y)
        for (size_t r = 0; r < c.batch; ++r) {  // the wrap and negation edges
            b.a[y * block + r * n] = (W) edge[r % 5];
            b.a[y * block + r * n + n - 1] = (W) edge[(r + 2) % 5];
        }
    for (size_t r = 0; c.perrow && r < c.batch; ++r) b.exps[r] = (uint32_t) rnd();
    memset(b.out, 0xA5, c.polys * lv * block * sizeof(W));
    run_kernel<W>(c, b.a, b.out, b.exps);
    for (size_t y = 0; y < c.polys; ++y)
        for (size_t r = 0; r < c.batch; ++r)
            ref_row<W>(b.a + y * block + r * n, b.mapped + y * block + r * n, c.logn, c.kind, c.perrow ? b.exps[r] : c.param, c.flags & 1, c.p);
    return true;
}

template <class W>
int check_case(const Case &c) {
    Buffers<W> b;
    if (!fill_and_run<W>(c, b)) return 2;
    const size_t block = c.batch << c.logn;
    for (size_t y = 0; y < c.polys; ++y)
        for (size_t i = 0; i < block; ++i) {
            const uint64_t x = b.mapped[y * block + i];
            if (!c.K) {
                if (b.out[y * block + i] != (W) x) return 1;
            } else {
                for (int k = 0; k < c.K; ++k)
                    if (b.out[(y * c.K + k) * block + i] != (W) digit_def(x, c.p, c.w, c.K, c.l, k)) return 1;
            }
        }
    return 0;
}

int run_case(const Case &c) { return c.wb == 4 ? check_case<uint32_t>(c) : check_case<uint64_t>(c); }

template <class W>
int dump_case(const Case &c, const char *path) {
    Buffers<W> b;
    Case plain = c;
    plain.K = 0;
    if (!fill_and_run<W>(plain, b)) return 2;
    const size_t block = c.batch << c.logn;
    FILE *f = fopen(path, "wb");
    if (!f) return 2;
    fwrite(b.a, sizeof(W), c.polys * block, f);
    for (size_t r = 0; r < c.batch; ++r) {
        const uint32_t e = c.perrow ? b.exps[r] : c.param;
        fwrite(&e, 4, 1, f);
    }
    fwrite(b.out, sizeof(W), c.polys * block, f);
    if (c.K) {
        W *dig = (W *) malloc(c.polys * (size_t) c.K * block * sizeof(W));
        if (!dig) return 2;
        run_kernel<W>(c, b.a, dig, b.exps);
        fwrite(dig, sizeof(W), c.polys * (size_t) c.K * block, f);
        free(dig);
    }
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 16 && !strcmp(argv[1], "dump")) {
        Case c{};
        c.wb = atoi(argv[2]);
        c.p = strtoull(argv[3], nullptr, 0);
        c.logn = atoi(argv[4]);
        c.batch = strtoull(argv[5], nullptr, 0);
        c.polys = strtoull(argv[6], nullptr, 0);
        c.kind = atoi(argv[7]);
        c.param = (uint32_t) strtoull(argv[8], nullptr, 0);
        c.perrow = atoi(argv[9]) != 0;
        c.flags = atoi(argv[10]);
        c.w = atoi(argv[11]);
        c.K = atoi(argv[12]);
        c.l = atoi(argv[13]);
        rng_state = strtoull(argv[14], nullptr, 0);
        return c.wb == 4 ? dump_case<uint32_t>(c, argv[15]) : dump_case<uint64_t>(c, argv[15]);
    }
    struct Modulus {
        int wb;
        uint64_t p;
        int dig[2][3];
    };
    // the digit sets of tests/test_gpu_product_gadget.py: one 3-level and one 1-level set per modulus
    const Modulus mods[4] = {{4, 3329, {{4, 3, 0}, {6, 1, 0}}},
                             {4, 3221225473ull, {{8, 3, 8}, {12, 1, 4}}},
                             {8, 0xFFFFFFFF00000001ull, {{8, 3, 40}, {16, 1, 0}}},
                             {8, 0x3FFFFFEE00000001ull, {{10, 3, 32}, {16, 1, 0}}}};
    const int logns[5] = {1, 2, 3, 6, 10};
    const size_t batches[3] = {1, 5, 33};
    size_t count = 0;
    for (const Modulus &mo : mods)
        for (int logn : logns)
            for (size_t batch : batches)
                for (size_t polys = 1; polys <= 2; ++polys)
                    for (int flags = 0; flags <= 1; ++flags) {
                        const uint32_t n = 1u << logn, V = 16u / (uint32_t) mo.wb;
                        const uint32_t exps[10] = {0, 1, V - 1, V, n - 1, n, n + 1, 2 * n - 1, 2 * n, 0xFFFFFFFFu};
                        const uint32_t gs[5] = {1, 3, 5, n + 1, 2 * n - 1};
                        for (int spec = 0; spec < 16; ++spec) {
                            Case c{};
                            c.wb = mo.wb, c.p = mo.p, c.logn = logn, c.batch = batch, c.polys = polys, c.flags = flags;
                            if (spec < 10) {
                                c.kind = MAP_MONOMIAL, c.param = exps[spec];
                            } else if (spec == 10) {
                                c.kind = MAP_MONOMIAL, c.perrow = true;
                            } else {
                                c.kind = MAP_AUTOMORPHISM, c.param = gs[spec - 11];
                                if (c.param >= 2 * n) continue;
                            }
                            for (int d = -1; d < 2; ++d) {
                                c.w = d < 0 ? 0 : mo.dig[d][0], c.K = d < 0 ? 0 : mo.dig[d][1], c.l = d < 0 ? 0 : mo.dig[d][2];
                                if (c.K && !gadget_params_ok(c.p, c.w, c.K, c.l)) {
                                    fprintf(stderr, "illegal digit set\n");
                                    return 3;
                                }
                                const int rc = run_case(c);
                                if (rc) {
                                    fprintf(stderr, "MISMATCH rc=%d wb=%d p=%llu logn=%d batch=%zu polys=%zu flags=%d kind=%d param=%u perrow=%d digits=(%d,%d,%d)\n", rc, c.wb,
                                            (unsigned long long) c.p, logn, batch, polys, flags, c.kind, c.param, (int) c.perrow, c.w, c.K, c.l);
                                    return 1;
                                }
                                ++count;
                            }
                        }
                    }
    printf("negacyclic map: %zu cases clean\n", count);
    return 0;
}
