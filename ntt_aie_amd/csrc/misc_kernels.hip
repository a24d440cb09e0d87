// misc_kernels.hip -- the small kernels around the pass kernels:
//   * pointwise product (config 4's middle leg; no reference counterpart),
//   * one-stage-per-launch network (the reference's test_stage hook,
//     src/test.cpp:55-58, 67: "run stages 0..stage and stop"), one thread per
//     butterfly exactly as src/test.cpp:42-51 enumerates them.  Bring-up path
//     and an independent second GPU implementation for the parity tests.
#include <hip/hip_runtime.h>

#include "field.h"
#include "kernels.h"
#include "negacyclic_map.h"

#ifndef NTT_PW_UNROLL
#define NTT_PW_UNROLL 2
#endif
#ifndef NTT_PW_NT
#define NTT_PW_NT 3  // bit 0: non-temporal loads, bit 1: non-temporal stores
#endif

namespace ntt {
namespace {

template <class W, int V>
struct alignas(sizeof(W) * V) Vec {
    W v[V];
};

template <class F>
__global__ __launch_bounds__(256) void pointwise_kernel(const typename F::W *a, const typename F::W *b,
                                                        typename F::W *c, size_t count, F f,
                                                        typename F::W scale, int use_scale) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using Ch = Vec<W, V>;
    const size_t nchunks = count / V;  // count is a multiple of N >= 2; tail handled below
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    // every word is read once and written once: non-temporal accesses, NTT_PW_UNROLL chunks of each operand requested before the
    // first product (same-process A/B in profiles/r02_pointwise.txt)
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const u32x4 *pa = reinterpret_cast<const u32x4 *>(a), *pb = reinterpret_cast<const u32x4 *>(b);
    u32x4 *pc = reinterpret_cast<u32x4 *>(c);
    size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (NTT_PW_UNROLL - 1) * stride < nchunks; i += NTT_PW_UNROLL * stride) {
        u32x4 xs[NTT_PW_UNROLL], ys[NTT_PW_UNROLL];
#pragma unroll
        for (int u = 0; u < NTT_PW_UNROLL; ++u) {
            xs[u] = (NTT_PW_NT & 1) ? __builtin_nontemporal_load(pa + i + u * stride) : pa[i + u * stride];
            ys[u] = (NTT_PW_NT & 1) ? __builtin_nontemporal_load(pb + i + u * stride) : pb[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < NTT_PW_UNROLL; ++u) {
            Ch x, y, z;
            __builtin_memcpy(&x, &xs[u], 16);
            __builtin_memcpy(&y, &ys[u], 16);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                W t = f.mul_plain(x.v[k], y.v[k]);
                z.v[k] = use_scale ? f.mul_plain(t, scale) : t;
            }
            u32x4 zz;
            __builtin_memcpy(&zz, &z, 16);
            if (NTT_PW_NT & 2) __builtin_nontemporal_store(zz, pc + i + u * stride);
            else pc[i + u * stride] = zz;
        }
    }
    for (; i < nchunks; i += stride) {
        Ch x = reinterpret_cast<const Ch *>(a)[i];
        Ch y = reinterpret_cast<const Ch *>(b)[i];
        Ch z;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            W t = f.mul_plain(x.v[k], y.v[k]);
            z.v[k] = use_scale ? f.mul_plain(t, scale) : t;
        }
        reinterpret_cast<Ch *>(c)[i] = z;
    }
    // tail (count not a multiple of V: only N = 2 with 4-byte words and odd batch)
    for (size_t i = nchunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        W t = f.mul_plain(a[i], b[i]);
        c[i] = use_scale ? f.mul_plain(t, scale) : t;
    }
}

// stage s: t = 2^s, butterfly k of a polynomial: block i = k >> s, j = (i << (s+1)) | (k & (t-1))
template <class F>
__global__ __launch_bounds__(256) void stage_kernel(typename F::W *data, const typename F::W *tw, int n,
                                                    int s, size_t total_bf, F f) {
    using W = typename F::W;
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const int half = n - 1;
    for (size_t g = (size_t) blockIdx.x * blockDim.x + threadIdx.x; g < total_bf; g += stride) {
        const size_t poly = g >> half;
        const uint32_t k = (uint32_t) (g & ((1u << half) - 1u));
        const uint32_t t = 1u << s;
        const uint32_t i = k >> s;
        const uint32_t j = (i << (s + 1)) | (k & (t - 1u));
        const uint32_t h = 1u << (n - s - 1);
        W *a = data + (poly << n);
        const W root = tw[h + i];  // table form
        const W v0 = a[j], v1 = a[j + t];
        a[j] = f.add(v0, v1);
        a[j + t] = f.mul(f.sub(v0, v1), root);
    }
}

// T[i] = base^e(i) in table (Montgomery) form, e(i) by the table rule (plan.h:make_table):
//   kind 0: e = i                         (src/test.cpp:27-32: natural-order powers)
//   kind 1: e = bitrev_{log2 h}(i - h) * N/(2h), h = 2^floor(log2 i)      (cyclic)
//   kind 2: e = bitrev_{logN}(i)                                          (negacyclic, base = psi^-1)
// Square-and-multiply per entry: log2(N) products, the whole table in one launch -- no host upload.
template <class F>
__global__ __launch_bounds__(256) void gen_table_kernel(typename F::W *T, int logn, int kind,
                                                        typename F::W base_m, typename F::W one_m, F f) {
    using W = typename F::W;
    const uint32_t N = 1u << logn;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        uint32_t e = i;
        if (kind == 1) {
            if (i == 0) {
                e = 0;
            } else {
                const int lh = 31 - __clz(i);
                const uint32_t idx = i - (1u << lh);
                const uint32_t rev = lh ? (__brev(idx) >> (32 - lh)) : 0u;
                e = rev << (logn - lh - 1);
            }
        } else if (kind == 2) {
            e = __brev(i) >> (32 - logn);
        }
        W r = one_m, b = base_m;
        while (e) {
            if (e & 1u) r = f.mul(r, b);
            b = f.mul(b, b);
            e >>= 1;
        }
        T[i] = r;
    }
}

// Coset vector of a low-degree extension (ntt_plan_set_coset): s[i] = shift^bitrev_logn(i mod 2^logn) in table form, made on
// the device like the twiddle tables (square-and-multiply per entry).  len = max(2^logn, 4): a vector shorter than one 16-byte
// chunk of 4-byte words is stored periodically, so that the fused first pass reads it in whole chunks.
template <class F>
__global__ __launch_bounds__(256) void gen_coset_kernel(typename F::W *s, int logn, uint32_t len, typename F::W shift_m,
                                                        typename F::W one_m, F f) {
    using W = typename F::W;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
        uint32_t e = __brev(i & ((1u << logn) - 1u)) >> (32 - logn);  // logn >= 1
        W r = one_m, b = shift_m;
        while (e) {
            if (e & 1u) r = f.mul(r, b);
            b = f.mul(b, b);
            e >>= 1;
        }
        s[i] = r;
    }
}

// The separate expansion of ntt_lde (sizes without a fused first pass; the fused pass's comparator): one thread per 16-byte
// chunk of the [batch][2^n] output, out[b][i << beta] = in[b][i] * s[i] and zero elsewhere, non-temporal 128-bit stores.
// Word w of the output buffer is live when its low beta bits are clear, and then comes from compact word w >> beta.
template <class F>
__global__ __launch_bounds__(256) void lde_expand_kernel(const typename F::W *in, const typename F::W *sv, typename F::W *out,
                                                         size_t chunks, int n, int beta, F f) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t live_mask = ((size_t) 1 << beta) - 1, row_mask = ((size_t) 1 << (n - beta)) - 1;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        Vec<W, V> z;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const size_t w = c * V + k;
            z.v[k] = (W) 0;
            if ((w & live_mask) == 0) z.v[k] = f.mul(in[w >> beta], sv[(w >> beta) & row_mask]);
        }
        u32x4 zz;
        __builtin_memcpy(&zz, &z, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(out) + c);
    }
}

// The separate scaling of ntt_coset_inverse (sizes whose last pass has no twin with the vector sweep; that sweep's comparator):
// buf[b][i] = buf[b][i] * u[i] in place, one thread per 16-byte chunk of the [batch][2^n] buffer, grid-stride.  A row of 2^n words
// is a whole number of chunks or (n = 1, 4-byte words) half of one: the vector is then stored periodically up to one chunk, so a
// chunk's multipliers are always the aligned chunk (word & u_mask) of it.  Canonical words in, canonical words out.
template <class F>
__global__ __launch_bounds__(256) void row_scale_kernel(typename F::W *buf, const typename F::W *u, size_t count, uint32_t u_mask, F f) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const size_t chunks = count / V, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const u32x4 xx = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(buf) + c);
        const Vec<W, V> m = *reinterpret_cast<const Vec<W, V> *>(u + ((uint32_t) (c * V) & u_mask));
        Vec<W, V> x;
        __builtin_memcpy(&x, &xx, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) x.v[k] = f.mul(x.v[k], m.v[k]);
        u32x4 zz;
        __builtin_memcpy(&zz, &x, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(buf) + c);
    }
    // tail (count not a multiple of V: only N = 2 with 4-byte words and an odd batch)
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) buf[i] = f.mul(buf[i], u[(uint32_t) i & u_mask]);
}

// The broadcast product of ntt_polymul_negacyclic_pre where no fused middle pass runs: buf[b][i] = buf[b][i] * row[i] * scale in place,
// plain (canonical) words throughout, one thread per 16-byte chunk, grid-stride.  `row` has EXACTLY row_mask + 1 words: a row shorter
// than a chunk (N = 2 of 4-byte words) goes word by word, so nothing past the row is read.
template <class F>
__global__ __launch_bounds__(256) void pointwise_row_kernel(typename F::W *buf, const typename F::W *row, size_t count, uint32_t row_mask, F f, typename F::W scale) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const size_t chunks = row_mask + 1u >= (uint32_t) V ? count / V : 0, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const u32x4 xx = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(buf) + c);
        const Vec<W, V> m = *reinterpret_cast<const Vec<W, V> *>(row + ((uint32_t) (c * V) & row_mask));
        Vec<W, V> x;
        __builtin_memcpy(&x, &xx, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) x.v[k] = f.mul_plain(f.mul_plain(x.v[k], m.v[k]), scale);
        u32x4 zz;
        __builtin_memcpy(&zz, &x, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(buf) + c);
    }
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        buf[i] = f.mul_plain(f.mul_plain(buf[i], row[(uint32_t) i & row_mask]), scale);
}

// The sum of ntt_polymul_dot_pre where no fused middle pass runs: a[0][r][i] = scale2 * sum_k a[k][r][i] * bhat[k][r | 0][i] / R^2 in place on
// term 0 (R = 2^32 or 2^64: scale2 = N^-1 * R^2 gives plain words from plain words), one thread per 16-byte chunk of the [batch][N] block,
// grid-stride; term k of a lies a_stride words on, of bhat b_stride words.  mul(x, m) is canonical for canonical m, so the running sum
// is canonical and add() exact; terms + 1 products per word.  bcast: a term of bhat has EXACTLY row_mask + 1 words -- a row shorter
// than a chunk (N = 2 of 4-byte words) goes word by word, so nothing past it is read.  bhat is only read.
template <class F>
__global__ __launch_bounds__(256) void dot_rows_kernel(typename F::W *a, const typename F::W *bhat, size_t count, uint32_t row_mask, int bcast, uint32_t terms,
                                                       size_t a_stride, size_t b_stride, F f, typename F::W scale2) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const size_t chunks = row_mask + 1u >= (uint32_t) V ? count / V : 0, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const size_t w = bcast ? (size_t) ((uint32_t) (c * V) & row_mask) : c * V;  // first word of the chunk inside a term of bhat
        Vec<W, V> acc;
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = (W) 0;
        for (uint32_t t = 0; t < terms; ++t) {
            const u32x4 xx = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a + (size_t) t * a_stride) + c);
            const Vec<W, V> m = *reinterpret_cast<const Vec<W, V> *>(bhat + (size_t) t * b_stride + w);
            Vec<W, V> x;
            __builtin_memcpy(&x, &xx, 16);
#pragma unroll
            for (int k = 0; k < V; ++k) acc.v[k] = f.add(acc.v[k], f.mul(x.v[k], m.v[k]));
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = f.mul(acc.v[k], scale2);
        u32x4 zz;
        __builtin_memcpy(&zz, &acc, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(a) + c);
    }
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        W acc = (W) 0;
        for (uint32_t t = 0; t < terms; ++t) acc = f.add(acc, f.mul(a[(size_t) t * a_stride + i], bhat[(size_t) t * b_stride + (bcast ? (size_t) ((uint32_t) i & row_mask) : i)]));
        a[i] = f.mul(acc, scale2);
    }
}

// The sums of ntt_polymul_matvec_pre where no fused middle pass runs: out[j][r][i] = scale2 * sum_k a[k][r][i] * bhat[j][k][r | 0][i] / R^2 for
// every j < outs in ONE launch -- dot_rows_kernel's arithmetic, word for word, out of place: a is only read (every output needs it).
// blockIdx.y is the output; within it one thread per 16-byte chunk of the [batch][N] block, grid-stride.  Output j's block of bhat lies
// j * terms * b_stride words on, its block of out j * count words.  bcast: a term of bhat has EXACTLY row_mask + 1 words -- a row shorter
// than a chunk goes word by word, so nothing past it is read.
template <class F>
__global__ __launch_bounds__(256) void matvec_rows_kernel(const typename F::W *a, const typename F::W *bhat, typename F::W *out, size_t count, uint32_t row_mask,
                                                          int bcast, uint32_t terms, size_t a_stride, size_t b_stride, F f, typename F::W scale2) {
    using W = typename F::W;
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    bhat += (size_t) blockIdx.y * terms * b_stride;
    out += (size_t) blockIdx.y * count;
    const size_t chunks = row_mask + 1u >= (uint32_t) V ? count / V : 0, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const size_t w = bcast ? (size_t) ((uint32_t) (c * V) & row_mask) : c * V;  // first word of the chunk inside a term of bhat
        Vec<W, V> acc;
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = (W) 0;
        for (uint32_t t = 0; t < terms; ++t) {
            const Vec<W, V> x = *(reinterpret_cast<const Vec<W, V> *>(a + (size_t) t * a_stride) + c);  // read again by every output: cached
            const Vec<W, V> m = *reinterpret_cast<const Vec<W, V> *>(bhat + (size_t) t * b_stride + w);
#pragma unroll
            for (int k = 0; k < V; ++k) acc.v[k] = f.add(acc.v[k], f.mul(x.v[k], m.v[k]));
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = f.mul(acc.v[k], scale2);
        u32x4 zz;
        __builtin_memcpy(&zz, &acc, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(out) + c);
    }
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        W acc = (W) 0;
        for (uint32_t t = 0; t < terms; ++t) acc = f.add(acc, f.mul(a[(size_t) t * a_stride + i], bhat[(size_t) t * b_stride + (bcast ? (size_t) ((uint32_t) i & row_mask) : i)]));
        out[i] = f.mul(acc, scale2);
    }
}

// The balanced gadget decomposition (ntt_gadget_decompose; pass.h: gadget_digit has the definition): digits[q][k][.] = digit_k(a[q][.]) for
// every k < levels.  The field is data: the modulus alone, no Montgomery constant, no table.  blockIdx.y is the polynomial q; within its
// [batch][N] block of `block` words one thread per 16-byte chunk, grid-stride, each word read once and its `levels` digits written to
// the blocks (q * levels + k) of digits; a block that is no whole number of chunks goes word by word.
template <class W>
__global__ __launch_bounds__(256) void gadget_decompose_kernel(const W *a, W *digits, size_t block, uint64_t p, int log_base, int levels, int low_bits) {
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const GadgetConsts g = gadget_consts(p, GadgetParams{log_base, levels, low_bits});
    a += (size_t) blockIdx.y * block;
    digits += (size_t) blockIdx.y * (size_t) levels * block;
    const size_t chunks = block % V == 0 ? block / V : 0, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const Vec<W, V> x = *(reinterpret_cast<const Vec<W, V> *>(a) + c);
        for (int k = 0; k < levels; ++k) {
            Vec<W, V> d;
#pragma unroll
            for (int e = 0; e < V; ++e) d.v[e] = (W) gadget_digit(g, (uint64_t) x.v[e], k * log_base, k == levels - 1);
            u32x4 dd;
            __builtin_memcpy(&dd, &d, 16);
            __builtin_nontemporal_store(dd, reinterpret_cast<u32x4 *>(digits + (size_t) k * block) + c);
        }
    }
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < block; i += stride)
        for (int k = 0; k < levels; ++k) digits[(size_t) k * block + i] = (W) gadget_digit(g, (uint64_t) a[i], k * log_base, k == levels - 1);
}

// The signed negacyclic maps X^e . a and a(X^g), optionally minus a itself, and (DIGITS) the balanced gadget digits of the mapped words
// (ntt_negacyclic_map, ntt_gadget_decompose_map, the first launch of ntt_polymul_gadget_map_pre; negacyclic_map.h has the index rule and
// the thread's loops, shared with the host program that runs them under the sanitizers).  gadget_decompose_kernel's launch shape:
// blockIdx.y is the polynomial q; within its [batch][N] block one thread per 16-byte DESTINATION chunk, grid-stride.  Row r of every
// polynomial takes exps[r] (a device array, loaded per chunk) or the one exponent / ginv of m.q.  The sources are gathered word by word:
// for the monomial adjacent lanes still read adjacent words, for the automorphism the stride is ginv and a row is read again from
// cache.  One 128-bit non-temporal store per chunk, or `levels` of them to the blocks (q * levels + k) of the digits.
template <class W, bool DIGITS>
__global__ __launch_bounds__(256) void negacyclic_map_kernel(const W *a, W *out, size_t block, MapArgs m) {
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    a += (size_t) blockIdx.y * block;
    out += (size_t) blockIdx.y * (size_t) (DIGITS ? m.gp.levels : 1) * block;
    negacyclic_map_thread<W, DIGITS>(a, out, block, m, (size_t) blockIdx.x * blockDim.x + threadIdx.x, (size_t) gridDim.x * blockDim.x,
                                     [](W *dst, size_t c, const MapChunk<W> &x) {
                                         u32x4 xx;
                                         __builtin_memcpy(&xx, &x, 16);
                                         __builtin_nontemporal_store(xx, reinterpret_cast<u32x4 *>(dst) + c);
                                     });
}

// The accumulate of ntt_polymul_gadget_map_pre: out[i] = out[i] + addend[i] mod p in place, canonical words, one thread per 16-byte chunk,
// grid-stride, chunked like row_scale_kernel; a count that is no multiple of V (N = 2 of 4-byte words, an odd row count) ends word by word.
template <class W>
__global__ __launch_bounds__(256) void add_rows_kernel(W *out, const W *addend, size_t count, W p) {
    constexpr int V = 16 / sizeof(W);
    using u32x4 = unsigned int __attribute__((ext_vector_type(4)));
    const size_t chunks = count / V, stride = (size_t) gridDim.x * blockDim.x;
    for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        const u32x4 xx = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(out) + c);
        const Vec<W, V> y = *(reinterpret_cast<const Vec<W, V> *>(addend) + c);
        Vec<W, V> x;
        __builtin_memcpy(&x, &xx, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) x.v[k] = map_addmod<W>(x.v[k], y.v[k], p);
        u32x4 zz;
        __builtin_memcpy(&zz, &x, 16);
        __builtin_nontemporal_store(zz, reinterpret_cast<u32x4 *>(out) + c);
    }
    for (size_t i = chunks * V + (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = map_addmod<W>(out[i], addend[i], p);
}

// out[i] = T[i] * c, both in table (Montgomery) form: the scaled stage-0 twiddles of the inverse transform (pass.h: fold_scale)
template <class F>
__global__ __launch_bounds__(256) void scale_table_kernel(const typename F::W *T, typename F::W *out, size_t count,
                                                          typename F::W c_m, F f) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t) gridDim.x * blockDim.x)
        out[i] = f.mul(T[i], c_m);
}

// precondition check: number of words >= p (the kernels, like the reference's vector_modadd /
// vector_modsub, src/aie_core.cc:41-62, assume canonical residues)
template <class W>
__global__ __launch_bounds__(256) void count_noncanonical_kernel(const W *a, size_t count, W p, unsigned long long *out) {
    unsigned long long bad = 0;
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) bad += a[i] >= p;
    for (int off = 32; off; off >>= 1) bad += __shfl_down(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
}

inline unsigned grid_for(size_t work) {
    size_t g = (work + 255) / 256;
    if (g > 8192) g = 8192;  // 256 CUs x 8 x 4: grid-stride the rest
    if (g == 0) g = 1;
    return (unsigned) g;
}

}  // namespace

// by field: the launchers of the pass / product translation units
hipError_t launch_pass(bool inverse, bool contig, int log_m, const ErasedArgs &a, hipStream_t s) {
    return with_field(a.field, [&](auto f) {
        using F = decltype(f);
        return inverse ? launch_pass_of<F, true>(contig, log_m, a, s) : launch_pass_of<F, false>(contig, log_m, a, s);
    });
}

hipError_t launch_mat_pass(bool inverse, int log_m, const ErasedArgs &a, hipStream_t s) {
    return with_field(a.field, [&](auto f) {
        using F = decltype(f);
        return inverse ? launch_mat_of<F, true>(log_m, a, s) : launch_mat_of<F, false>(log_m, a, s);
    });
}

hipError_t launch_product_mid(int log_m, const ErasedArgs &a, hipStream_t s) {
    return with_field(a.field, [&](auto f) {
        if (!product_no_digits(a)) return launch_product_gad_mid_of<decltype(f)>(log_m, a, s);
        if (a.mv_outs != 0) return launch_product_mv_mid_of<decltype(f)>(log_m, a, s);
        if (a.dot_terms != 0) return launch_product_dot_mid_of<decltype(f)>(log_m, a, s);
        return a.in2_prepared ? launch_product_pre_mid_of<decltype(f)>(log_m, a, s) : launch_product_mid_of<decltype(f)>(log_m, a, s);
    });
}

hipError_t launch_pointwise(const FieldParams &fp, const void *a, const void *b, void *c, size_t count, uint64_t scale, hipStream_t s) {
    if (count == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(pointwise_kernel<F>, dim3(grid_for(count / (16 / sizeof(W)))), dim3(256), 0, s, (const W *) a, (const W *) b, (W *) c, count, f,
                           (W) scale, scale != 1 ? 1 : 0);
        return hipGetLastError();
    });
}

hipError_t launch_pointwise_row(const FieldParams &fp, void *buf, const void *row, int n, size_t batch, uint64_t scale, hipStream_t s) {
    const size_t count = batch << n;
    if (count == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(pointwise_row_kernel<F>, dim3(grid_for((count + 16 / sizeof(W) - 1) / (16 / sizeof(W)))), dim3(256), 0, s, (W *) buf, (const W *) row, count,
                           (uint32_t) (((size_t) 1 << n) - 1), f, (W) scale);
        return hipGetLastError();
    });
}

hipError_t launch_dot_rows(const FieldParams &fp, void *a, const void *bhat, int n, size_t batch, size_t bhat_rows, size_t terms, uint64_t scale2, hipStream_t s) {
    const size_t count = batch << n;
    if (count == 0 || terms == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(dot_rows_kernel<F>, dim3(grid_for((count + 16 / sizeof(W) - 1) / (16 / sizeof(W)))), dim3(256), 0, s, (W *) a, (const W *) bhat, count,
                           (uint32_t) (((size_t) 1 << n) - 1), bhat_rows != batch ? 1 : 0, (uint32_t) terms, count, bhat_rows << n, f, (W) scale2);
        return hipGetLastError();
    });
}

hipError_t launch_matvec_rows(const FieldParams &fp, const void *a, const void *bhat, void *out, int n, size_t batch, size_t bhat_rows, size_t terms, size_t outs,
                              uint64_t scale2, hipStream_t s) {
    const size_t count = batch << n;
    if (count == 0 || terms == 0 || outs == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        // blockIdx.y is the output: one launch up to 65535 outputs, a slice per 65535 beyond
        for (size_t j = 0; j < outs; j += 65535u) {
            const size_t nj = outs - j < 65535u ? outs - j : 65535u;
            hipLaunchKernelGGL(matvec_rows_kernel<F>, dim3(grid_for((count + 16 / sizeof(W) - 1) / (16 / sizeof(W))), (unsigned) nj), dim3(256), 0, s, (const W *) a,
                               (const W *) bhat + j * terms * (bhat_rows << n), (W *) out + j * count, count, (uint32_t) (((size_t) 1 << n) - 1), bhat_rows != batch ? 1 : 0,
                               (uint32_t) terms, count, bhat_rows << n, f, (W) scale2);
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    });
}

hipError_t launch_gadget_decompose(const FieldParams &fp, const void *a, void *digits, int n, size_t polys, size_t batch, int log_base, int levels, int low_bits,
                                   hipStream_t s) {
    const size_t block = batch << n;
    if (block == 0 || polys == 0) return hipSuccess;
    if (!gadget_params_ok(fp.p, log_base, levels, low_bits)) return hipErrorInvalidValue;
    auto go = [&](auto w) {
        using W = decltype(w);
        // blockIdx.y is the polynomial: one launch up to 65535 polynomials, a slice per 65535 beyond
        for (size_t q = 0; q < polys; q += 65535u) {
            const size_t nq = polys - q < 65535u ? polys - q : 65535u;
            hipLaunchKernelGGL(gadget_decompose_kernel<W>, dim3(grid_for((block + 16 / sizeof(W) - 1) / (16 / sizeof(W))), (unsigned) nq), dim3(256), 0, s,
                               (const W *) a + q * block, (W *) digits + q * (size_t) levels * block, block, fp.p, log_base, levels, low_bits);
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    };
    return field_word_bytes(fp) == 4 ? go(uint32_t{}) : go(uint64_t{});
}

hipError_t launch_negacyclic_map(const FieldParams &fp, const void *a, void *out, int n, size_t polys, size_t batch, int kind, uint32_t q, const uint32_t *d_exp,
                                 int minus_identity, int log_base, int levels, int low_bits, hipStream_t s) {
    const size_t block = batch << n;
    if (block == 0 || polys == 0) return hipSuccess;
    if (levels != 0 && !gadget_params_ok(fp.p, log_base, levels, low_bits)) return hipErrorInvalidValue;
    const MapArgs m{kind, n, q, d_exp, minus_identity, fp.p, GadgetParams{log_base, levels, low_bits}};
    auto go = [&](auto w) {
        using W = decltype(w);
        // blockIdx.y is the polynomial: one launch up to 65535 polynomials, a slice per 65535 beyond
        for (size_t y = 0; y < polys; y += 65535u) {
            const size_t ny = polys - y < 65535u ? polys - y : 65535u;
            const dim3 grid(grid_for((block + 16 / sizeof(W) - 1) / (16 / sizeof(W))), (unsigned) ny);
            if (levels != 0)
                hipLaunchKernelGGL((negacyclic_map_kernel<W, true>), grid, dim3(256), 0, s, (const W *) a + y * block, (W *) out + y * (size_t) levels * block, block, m);
            else
                hipLaunchKernelGGL((negacyclic_map_kernel<W, false>), grid, dim3(256), 0, s, (const W *) a + y * block, (W *) out + y * block, block, m);
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    };
    return field_word_bytes(fp) == 4 ? go(uint32_t{}) : go(uint64_t{});
}

hipError_t launch_add_rows(const FieldParams &fp, void *out, const void *addend, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    auto go = [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL(add_rows_kernel<W>, dim3(grid_for((count + 16 / sizeof(W) - 1) / (16 / sizeof(W)))), dim3(256), 0, s, (W *) out, (const W *) addend, count, (W) fp.p);
        return hipGetLastError();
    };
    return field_word_bytes(fp) == 4 ? go(uint32_t{}) : go(uint64_t{});
}

hipError_t launch_gen_table(const FieldParams &fp, void *T, int logn, int kind, uint64_t base_m, uint64_t one_m, hipStream_t s) {
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(gen_table_kernel<F>, dim3(grid_for((size_t) 1 << logn)), dim3(256), 0, s, (W *) T, logn, kind, (W) base_m, (W) one_m, f);
        return hipGetLastError();
    });
}

hipError_t launch_gen_coset(const FieldParams &fp, void *s_out, int logn, uint32_t len, uint64_t shift_m, uint64_t one_m, hipStream_t s) {
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(gen_coset_kernel<F>, dim3(grid_for(len)), dim3(256), 0, s, (W *) s_out, logn, len, (W) shift_m, (W) one_m, f);
        return hipGetLastError();
    });
}

hipError_t launch_lde_expand(const FieldParams &fp, const void *in, const void *s_vec, void *out, int n, int beta, size_t batch, hipStream_t s) {
    const size_t chunks = ((batch << n) * (size_t) field_word_bytes(fp)) / 16;  // 2^n words >= 16 bytes (n >= 2)
    if (chunks == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(lde_expand_kernel<F>, dim3(grid_for(chunks)), dim3(256), 0, s, (const W *) in, (const W *) s_vec, (W *) out, chunks, n, beta, f);
        return hipGetLastError();
    });
}

hipError_t launch_row_scale(const FieldParams &fp, void *buf, const void *u_vec, int n, size_t batch, hipStream_t s) {
    const size_t count = batch << n;
    if (count == 0) return hipSuccess;
    const size_t u_words = ((size_t) 1 << n) < 4 ? 4 : (size_t) 1 << n;  // the vector's (periodic) length, a power of two
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        // (grid_for caps the grid far below the launch limits and the kernel strides over a 64-bit count: no slicing needed)
        hipLaunchKernelGGL(row_scale_kernel<F>, dim3(grid_for((count + 16 / sizeof(W) - 1) / (16 / sizeof(W)))), dim3(256), 0, s, (W *) buf, (const W *) u_vec, count,
                           (uint32_t) (u_words - 1), f);
        return hipGetLastError();
    });
}

hipError_t launch_scale_table(const FieldParams &fp, const void *T, void *out, size_t count, uint64_t c_m, hipStream_t s) {
    if (count == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        if constexpr (sizeof(typename F::W) == 8) {
            hipLaunchKernelGGL(scale_table_kernel<F>, dim3(grid_for(count)), dim3(256), 0, s, (const uint64_t *) T, (uint64_t *) out, count, c_m, f);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;  // 4-byte words keep the scaling sweep (pass.h: fold_scale): no such table
        }
    });
}

hipError_t launch_count_noncanonical(const void *a, size_t count, int word_bytes, uint64_t p, void *d_out, hipStream_t s) {
    if (word_bytes == 8)
        hipLaunchKernelGGL(count_noncanonical_kernel<uint64_t>, dim3(grid_for(count)), dim3(256), 0, s,
                           (const uint64_t *) a, count, p, (unsigned long long *) d_out);
    else
        hipLaunchKernelGGL(count_noncanonical_kernel<uint32_t>, dim3(grid_for(count)), dim3(256), 0, s,
                           (const uint32_t *) a, count, (uint32_t) p, (unsigned long long *) d_out);
    return hipGetLastError();
}

hipError_t launch_stage(const FieldParams &fp, void *data, const void *tw, int n, int stage, size_t batch, hipStream_t s) {
    const size_t total = batch << (n - 1);
    if (total == 0) return hipSuccess;
    return with_field(fp, [&](auto f) {
        using F = decltype(f);
        using W = typename F::W;
        hipLaunchKernelGGL(stage_kernel<F>, dim3(grid_for(total)), dim3(256), 0, s, (W *) data, (const W *) tw, n, stage, total, f);
        return hipGetLastError();
    });
}

}  // namespace ntt
