// emu_sweep.h -- what the stand-alone sweep programs of the host index model share (the *_MAIN sections of emu_lde.cpp,
// emu_coset_inverse.cpp, emu_columns.cpp, emu_lde_columns.cpp; built with ASan + UBSan and linked with oracle/ntt_oracle.c by the
// tests/test_*_emu_asan.py): the random stream, the three word classes, word access of either width, the oracle by word width
// and the closing report.  TEST INFRASTRUCTURE.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/ntt_oracle.h"

namespace sweep {

inline uint64_t rnd() {
    static uint64_t state = 0x9E3779B97F4A7C15ull;
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}
// a residue, 0 and p - 1 among them
inline uint64_t rnd_residue(uint64_t p) {
    const uint64_t r = rnd();
    return (r & 15) == 0 ? 0 : (r & 15) == 1 ? p - 1 : (r >> 4) % p;
}

struct Class {
    const char *name;
    int wb;
    uint64_t p, g;
};
// the class a program was started for (argv[1]: gl | m64 | m32), or null
inline const Class *find_class(const char *name) {
    static const Class classes[] = {
        {"gl", 8, 0xFFFFFFFF00000001ull, 7},
        {"m64", 8, 0xFFFFFFFC00000001ull, 10},  // general 64-bit class: an NTT prime above 2^63 (sums wrap: the carry paths)
        {"m32", 4, 998244353ull, 3},
    };
    for (const Class &c : classes)
        if (strcmp(c.name, name) == 0) return &c;
    return nullptr;
}

inline uint64_t get(const void *b, int wb, size_t i) { return wb == 4 ? ((const uint32_t *) b)[i] : ((const uint64_t *) b)[i]; }
inline void put(void *b, int wb, size_t i, uint64_t v) {
    if (wb == 4) ((uint32_t *) b)[i] = (uint32_t) v;
    else ((uint64_t *) b)[i] = v;
}

// the oracle's network on `batch` polynomials of n words in place (inverse: the scaled one; non-zero = not invertible), and its
// AIE_BLOCK16 permutation of one polynomial
inline int oracle_transform(const Class &c, void *a, size_t n, size_t batch, const void *T, bool inverse) {
    if (c.wb == 4) {
        if (inverse) return oracle_intt_batch_u32((uint32_t *) a, (uint32_t) n, batch, (const uint32_t *) T, (uint32_t) c.p, 1);
        oracle_ntt_batch_u32((uint32_t *) a, (uint32_t) n, batch, (const uint32_t *) T, (uint32_t) c.p, 1);
        return 0;
    }
    if (inverse) return oracle_intt_batch_u64((uint64_t *) a, n, batch, (const uint64_t *) T, c.p, 1);
    oracle_ntt_batch_u64((uint64_t *) a, n, batch, (const uint64_t *) T, c.p, 1);
    return 0;
}
inline void oracle_block16(const Class &c, void *dst, const void *src, size_t n) {
    if (c.wb == 4) oracle_block16_u32((uint32_t *) dst, (const uint32_t *) src, (uint32_t) n);
    else oracle_block16_u64((uint64_t *) dst, (const uint64_t *) src, n);
}
// the size-n kind-1 table of the class as words of its width (malloc), or null when n does not divide p - 1
inline void *oracle_table(const Class &c, size_t n) {
    uint64_t *t64 = (uint64_t *) malloc(n * sizeof(uint64_t));
    void *T = malloc(n * (size_t) c.wb);
    if (!t64 || !T) abort();
    const bool ok = oracle_make_table_u64(1, n, t64, c.p, c.g) == 0;
    for (size_t i = 0; i < n && ok; i++) put(T, c.wb, i, t64[i]);
    free(t64);
    if (!ok) free(T);
    return ok ? T : nullptr;
}

// the last lines of a program and its exit code
inline int report(const char *name, long cases, long bad) {
    printf("%s: %ld cases, %ld bad\n", name, cases, bad);
    if (bad == 0 && cases > 0) printf("%s: %ld cases clean\n", name, cases);
    return bad ? 1 : (cases ? 0 : 3);
}

}  // namespace sweep
