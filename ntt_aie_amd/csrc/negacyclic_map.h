// negacyclic_map.h -- the signed coefficient permutations of Z_p[X] / (X^N + 1) that come before a gadget decomposition
// (ntt_negacyclic_map, ntt_gadget_decompose_map, ntt_polymul_gadget_map_pre; include/ntt_hip.h has the definitions), written once for
// the device kernel (misc_kernels.hip: negacyclic_map_kernel), the C-ABI's argument checks and the host program that runs the kernel's
// loops under the sanitizers (tests/emu/emu_negacyclic_map.cpp).
//
// Word level throughout: the modulus alone, no Montgomery constant, no table.  N = 2^logn, M2 = 2N - 1, j < N the DESTINATION index:
//   monomial      y = X^e . a         t = (j - e) & M2          (e: any 32-bit word, taken mod 2N -- 2N divides 2^32)
//   automorphism  y(X) = a(X^g)       t = (j * ginv) & M2       (g odd, ginv = g^-1 mod 2N; the 32-bit product wraps mod 2^32, a multiple of 2N)
//   both          src = t & (N - 1),  neg = (t & N) != 0,       y[j] = neg ? -a[src] : a[src]
// Why: X^(2N) = 1 and X^N = -1, so a[i] lands on X^((i + e) mod 2N), on X^(i g mod 2N) for the automorphism, and an exponent j + N
// is -X^j.  Solving for i with j < N: t < N is the source of +X^j; otherwise t - N is the source of X^(j + N) = -X^j (N ginv = N mod 2N
// because ginv is odd).  Exactly one of the two is below N: the map is a signed permutation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pass.h"  // NTT_HD, gadget_consts / gadget_digit

namespace ntt {

enum { MAP_MONOMIAL = 0, MAP_AUTOMORPHISM = 1 };
enum { MAP_MINUS_IDENTITY = 1 };

struct MapSource {
    uint32_t src;
    bool neg;
};

// q: the exponent e (monomial) or ginv (automorphism)
NTT_HD MapSource map_source(int kind, int logn, uint32_t q, uint32_t j) {
    const uint32_t n = 1u << logn, m2 = 2u * n - 1u;  // logn <= 28: 2N fits with room
    const uint32_t t = (kind == MAP_MONOMIAL ? j - q : j * q) & m2;
    return MapSource{t & (n - 1u), (t & n) != 0u};
}

// g^-1 mod 2N for odd g: Newton's iteration x <- x (2 - g x) mod 2^32 doubles the correct low bits (g g = 1 mod 8: 3, 6, 12, 24, 48)
inline uint32_t map_ginv(uint32_t g, int logn) {
    uint32_t x = g;
    for (int i = 0; i < 4; ++i) x *= 2u - g * x;
    return x & ((2u << logn) - 1u);
}

// (x + y) mod p of canonical words; the sum may wrap the word when p is above half its range: keep the carry
template <class W>
NTT_HD W map_addmod(W x, W y, W p) {
    const W s = (W) (x + y);
    return (s < x || s >= p) ? (W) (s - p) : s;
}

// word j of the mapped row: `row` is the N canonical words of the source row, of which src and (minus_identity) j are read.
// MINUS_IDENTITY, y - a[j] mod p: x - a[j] when x >= a[j] (no borrow), else x + (p - a[j]), where p - a[j] <= p and
// x < a[j] give x + (p - a[j]) < p: neither branch wraps a W word, for any p < 2^32 (4-byte words) or p < 2^64 (8-byte words).
template <class W>
NTT_HD W mapped_word(const W *row, W p, int kind, int logn, uint32_t q, int minus_identity, uint32_t j) {
    const MapSource s = map_source(kind, logn, q, j);
    W x = row[s.src];
    if (s.neg && x != (W) 0) x = (W) (p - x);
    if (minus_identity) {
        const W y = row[j];
        x = x >= y ? (W) (x - y) : (W) (x + (W) (p - y));
    }
    return x;
}

template <class W>
struct alignas(16) MapChunk {
    W v[16 / sizeof(W)];
};

struct MapArgs {
    int kind, logn;
    uint32_t q;            // every row's exponent (monomial, exps == null) or ginv (automorphism)
    const uint32_t *exps;  // monomial only: row r of every polynomial uses exps[r]
    int minus_identity;
    uint64_t p;
    GadgetParams gp;  // DIGITS only
};

// One thread of negacyclic_map_kernel on one polynomial: a is its [batch][N] block of `block` words, out its block of the output
// (DIGITS: its `levels` blocks, digit k of word i at out[k * block + i]).  The thread takes the 16-byte destination chunks first,
// first + stride, ...; the row of a chunk is chunk * V >> logn, its exponent is loaded per chunk, its V source words are gathered one
// by one, and store16(dst, chunk, words) writes one chunk (DIGITS: one per level, each source word gathered ONCE).  A block that is no
// whole number of chunks, or a row shorter than a chunk (N = 2 of 4-byte words), goes word by word.  Nothing outside the row is read.
template <class W, bool DIGITS, class Store>
NTT_HD void negacyclic_map_thread(const W *a, W *out, size_t block, const MapArgs &m, size_t first, size_t stride, Store &&store16) {
    constexpr int V = 16 / sizeof(W);
    const GadgetConsts g = DIGITS ? gadget_consts(m.p, m.gp) : GadgetConsts{};
    const int levels = DIGITS ? m.gp.levels : 1;
    const size_t chunks = (block % V == 0 && ((size_t) 1 << m.logn) >= (size_t) V) ? block / V : 0;
    const uint32_t row_mask = (1u << m.logn) - 1u;
    for (size_t c = first; c < chunks; c += stride) {
        const size_t w0 = c * V, r = w0 >> m.logn;
        const uint32_t j0 = (uint32_t) w0 & row_mask, q = m.exps ? m.exps[r] : m.q;
        const W *row = a + (r << m.logn);
        MapChunk<W> x;
#pragma unroll
        for (int e = 0; e < V; ++e) x.v[e] = mapped_word<W>(row, (W) m.p, m.kind, m.logn, q, m.minus_identity, j0 + (uint32_t) e);
        if (!DIGITS) {
            store16(out, c, x);
        } else {
            for (int k = 0; k < levels; ++k) {
                MapChunk<W> d;
#pragma unroll
                for (int e = 0; e < V; ++e) d.v[e] = (W) gadget_digit(g, (uint64_t) x.v[e], k * m.gp.log_base, k == levels - 1);
                store16(out + (size_t) k * block, c, d);
            }
        }
    }
    for (size_t i = chunks * V + first; i < block; i += stride) {
        const size_t r = i >> m.logn;
        const uint32_t q = m.exps ? m.exps[r] : m.q;
        const W x = mapped_word<W>(a + (r << m.logn), (W) m.p, m.kind, m.logn, q, m.minus_identity, (uint32_t) i & row_mask);
        if (!DIGITS) {
            out[i] = x;
        } else {
            for (int k = 0; k < levels; ++k) out[(size_t) k * block + i] = (W) gadget_digit(g, (uint64_t) x, k * m.gp.log_base, k == levels - 1);
        }
    }
}

}  // namespace ntt
