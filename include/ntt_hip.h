/*
 * ntt_hip.h -- C-ABI of libntt_hip.so, the MI355X (gfx950) NTT engine.
 *
 * This is the drop-in boundary for the hot path of hal-lab-u-tokyo/ntt-aie.
 * Citations are file:line under the reference tree.  The reference launches its
 * device graph as
 *     kernel(bo_instr, n_instr, bo_inA, bo_root, bo_outC); run.wait();
 *                                                   (src/test.cpp:159-160, 181-182)
 * whose runtime sequence is sequence(input, root, output) over three
 * memref<N x i32> (src/aie2.py:320-337).  The same three buffers -- input
 * coefficients, twiddle table "root", output -- are what this library takes;
 * (bo_instr, n_instr) are the AIE instruction stream and have no counterpart.
 *
 * Conventions
 *   - plain C: opaque handle, raw device/host pointers, sizes; no C++/torch types.
 *   - every entry point returns int: 0 = ok, negative = NTT_E_* argument/state
 *     error, positive = hipError_t from the runtime.  Nothing throws or aborts
 *     (reference error contract: ERT state != COMPLETED -> message + return 1,
 *     src/test.cpp:162-166): every entry point is a function-try-block
 *     (csrc/guard.h), a failed host allocation comes back as NTT_E_NOMEM.
 *   - ALIGNMENT: every device DATA pointer handed to a transform (d_in, d_out,
 *     d_a, d_b, d_buf) must be 16-byte aligned -- the kernels move 128-bit
 *     vectors.  hipMalloc / torch allocations are (256 bytes); a row view
 *     &buf[b*N] is whenever N * word_bytes is a multiple of 16, i.e. always
 *     except N = 2 with 4-byte words (and N = 1 rows do not exist: logn >= 1).
 *     A misaligned pointer is refused with NTT_E_ARG before any launch.
 *   - device buffers are caller-owned; polynomials are contiguous [batch][N]
 *     words in the reference's element order (natural order in, src/test.cpp:141).
 *     Words are uint32_t (any odd p < 2^32) or uint64_t (any odd p < 2^64; p = 2^64 - 2^32 + 1 takes a faster path).
 *     Coefficients and twiddles must be canonical residues in [0, p) (the
 *     precondition of vector_modadd / vector_modsub, src/aie_core.cc:41-62).
 *   - launches are asynchronous on the caller's hipStream_t (passed as void*;
 *     NULL = default stream).  A plan is immutable after ntt_plan_set_twiddles
 *     and may be shared by host threads; one plan per device.
 *   - no hidden allocation per call: the plan owns its device twiddle copies (and one counter word for
 *     ntt_count_noncanonical, serialised by a mutex: the only entry point that writes plan state).
 *   - the library reads no environment variable that can change a result (NTT_ROCTX=1 only adds ROCTX ranges);
 *     experiment switches exist only in the separate libntt_hip_exp.so build that tools/ load.
 */
#ifndef NTT_HIP_H
#define NTT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntt_plan *ntt_plan_t;

/* error codes (negative) */
enum {
    NTT_OK = 0,
    NTT_E_ARG = -1,        /* null pointer / size out of range */
    NTT_E_PRIME = -2,      /* p even, p < 3, or p >= 2^32 for 4-byte words */
    NTT_E_LOGN = -3,       /* logn outside [1, NTT_MAX_LOGN] */
    NTT_E_NOTABLE = -4,    /* transform requested before ntt_plan_set_twiddles */
    NTT_E_NOTINVERTIBLE = -5, /* inverse requested but a twiddle is not a unit mod p (0, or shares a factor with a composite p) */
    NTT_E_LAYOUT = -6,     /* NTT_LAYOUT_AIE_BLOCK16 needs N >= 16 */
    NTT_E_RANGE = -7,      /* a twiddle handed to set_twiddles is >= p */
    NTT_E_NODEVICE = -8,   /* no HIP device / device index out of range */
    NTT_E_NOMEM = -9,      /* host memory: a staging buffer (N words) could not be allocated (std::bad_alloc caught at the boundary) */
    NTT_E_INTERNAL = -10   /* any other C++ exception caught at the boundary (never expected; reported instead of terminating the caller) */
};

#define NTT_MAX_LOGN 28

/* element order of the transform-domain buffer */
enum {
    NTT_LAYOUT_NATURAL = 0,
    /* the reference device's output order: 16 blocks of N/16 words, block
     * ans_order[i] holds natural block i (src/test.cpp:69-71, 212-219; caused by the
     * two tile swaps src/aie2.py:192-209, 257-265) */
    NTT_LAYOUT_AIE_BLOCK16 = 1
};

/* library / build identification: returns 10000*major + 100*minor + patch */
int ntt_version(void);
const char *ntt_error_string(int code);
/* number of visible HIP devices (0 if none); never fails */
int ntt_device_count(void);

/* ---- plan -----------------------------------------------------------------
 * Replaces the compile-time constants the reference bakes into every tile call
 * (logN, p, Barrett w/u: src/aie2.py:14-19, 178-306; src/test.cpp:66, 76-77).
 * word_bytes = 4 -> uint32_t words, odd p < 2^32 (Montgomery arithmetic on the
 * device: results are canonical, hence equal to the reference's Barrett words,
 * src/aie_core.cc:27-39, 64-102); word_bytes = 8 -> any odd p < 2^64 (the reference's `%`-based network takes any modulus,
 * src/test.cpp:48-50): p = 2^64-2^32+1 runs the Goldilocks-specific reduction, every other modulus Montgomery with R = 2^64
 * (about 0.74 x the Goldilocks throughput).  Primality is never checked, as in the reference. */
int ntt_plan_create(ntt_plan_t *out, int logn, uint64_t p, int word_bytes, int device);
int ntt_plan_destroy(ntt_plan_t plan);

/* The "root" buffer (bo_root, src/test.cpp:119-120, 137-143, 150): N words,
 * T[0] unused, T[h+i] is the twiddle of block i at the stage with h blocks
 * (src/test.cpp:45).  Copied to the device (and pre-transformed for the
 * arithmetic the kernels use); the inverse table T^-1 is derived here.
 * host_T is a HOST pointer; synchronous. */
int ntt_plan_set_twiddles(ntt_plan_t plan, const void *host_T);

/* Table rule of the reference host (make_roots + modPow + root[0] = 1,
 * src/test.cpp:15-32, 138): w = g^((p-1)/N) with integer division,
 * T[i] = T[i-1]*w mod p.  Fills host_T (N words of the plan's word size). */
int ntt_make_roots(ntt_plan_t plan, uint64_t g, void *host_T);
/* Tables that make the same network a genuine transform:
 *   kind 1: cyclic  T[h+i] = w^(bitrev(i) * N/(2h)),  w = g^((p-1)/N)
 *   kind 2: negacyclic (Longa-Naehrig) T[k] = psi^-bitrev(k), psi = g^((p-1)/(2N))
 * (kind 0 = ntt_make_roots).  Returns NTT_E_ARG when N does not divide the order. */
int ntt_make_table(ntt_plan_t plan, int kind, uint64_t g, void *host_T);

/* The same tables generated ON THE DEVICE (no host table, no upload): one
 * square-and-multiply per entry from w = g^((p-1)/N) (kind 0/1) or psi^-1 (kind 2), forward and
 * inverse table in table form.  Equivalent to ntt_make_table + ntt_plan_set_twiddles. */
int ntt_plan_generate_twiddles(ntt_plan_t plan, int kind, uint64_t g);
/* Read back the plan's table as plain residues (inverse != 0: the T^-1 table). */
int ntt_plan_get_twiddles(ntt_plan_t plan, int inverse, void *host_T);

/* plan introspection (for harnesses): 0 logn, 1 word_bytes, 2 device,
 * 3 number of HBM passes of one forward transform (default decomposition), 4 has-inverse-table,
 * 32 + i: stages in pass i, 64 + i: first stage of pass i (pass 0 is the contiguous one);
 * 6 number of decomposition alternatives, 7 forced alternative (-1 = chosen by batch),
 * 8 the largest number of passes over all alternatives (capacity for ntt_forward_profile),
 * 256 + 16*a + k for alternative a: k = 0 number of passes, k = 1..7 stages in pass k-1,
 * k = 8..14 first stage of pass k-8, k = 15 the smallest batch this alternative is chosen for;
 * 512 + 16*a + k: the kernel variant of pass k of alternative a (0 = the default kernel of that pass shape; 1 = a single-pass
 * size of 2^10..2^12 words on twice the threads, chosen below the batch that fills the device);
 * 9 the coset blow-up log2 set by ntt_plan_set_coset (0 = not set), 10 whether ntt_lde on this plan expands inside its first
 * pass (1) or runs the separate expansion kernel first (0; also 0 while no coset is set);
 * 11 whether a coset-inverse shift is set (ntt_plan_set_coset_inverse), 12 whether ntt_coset_inverse on this plan scales inside
 * its last pass (1) or runs the separate row-scaling kernel after the transform (0; also 0 while nothing is set);
 * 13 number of passes of the columns decomposition (ntt_forward_columns / ntt_inverse_columns; 0 when logn < 4),
 * 14 whether ntt_polymul_matvec_pre on this plan runs ONE middle launch per pair of outputs through the two-output kernel (1) or one
 * summed launch per output or the unfused path (0); answered for the pinned decomposition, else for the one a batch of 1 selects,
 * 15 whether ntt_polymul_gadget_pre on this plan decomposes inside the middle launch (1) or runs the decomposition kernel first (0);
 * answered by the rule of item 14: for the pinned decomposition, else for the one a batch of 1 selects,
 * 96 + i: stages in pass i of it, 128 + i: first stage of pass i of it (every pass is a column pass) */
int64_t ntt_plan_info(ntt_plan_t plan, int what);

/* The stage decomposition into HBM passes is chosen at LAUNCH, by batch size, among alternatives fixed at plan creation
 * from (N, word size, modulus class) -- the role of the reference's slab-size rule, where the per-tile slab follows from
 * N and the number of cores (src/aie2.py:21-28).  The tables are decomposition-agnostic, so alternatives cost no device
 * memory and every alternative computes the same words.
 *   ntt_plan_select: the alternative ntt_forward / ntt_inverse / ntt_polymul_negacyclic run for `batch` (>= 0); a product of
 *   `batch` pairs selects ONCE by `batch` and runs every one of its transforms (also the two-operand launches over 2*batch
 *   rows) with that decomposition.
 *   ntt_plan_set_policy: alternative = -1 (default) chooses by batch; k >= 0 pins alternative k.  Plan configuration, like
 *   ntt_plan_set_twiddles: call it before the plan is shared between host threads. */
int ntt_plan_select(ntt_plan_t plan, size_t batch);
int ntt_plan_set_policy(ntt_plan_t plan, int alternative);

/* A copy of `src` on another device (or the same one): tables are copied device-to-device (hipMemcpyPeer over xGMI, no
 * host round trip, no host table needed -- works after ntt_plan_generate_twiddles too).  This is the multi-device leg of
 * the boundary: the reference broadcasts its one table to every tile below the host (src/aie2.py:96-104, object-fifo
 * broadcast of the root buffer) and scatters / gathers the data per tile (src/aie2.py:83-115); a host shards [B][N]
 * over ntt_device_count() devices by cloning one plan per device and launching each shard on its own stream
 * (tests/cxx/multi_device_host.cpp). */
int ntt_plan_clone(ntt_plan_t src, int device, ntt_plan_t *out);

/* ---- transforms ------------------------------------------------------------
 * Forward = the reference network (src/test.cpp:34-60; tile kernels
 * src/aie_core.cc:161-187, 189-361): stage s = 0..logN-1, stride 2^s,
 *   (x, y) -> (x + y, (x - y) * T[N/2^(s+1) + block])  mod p.
 * d_in natural order, d_out in `out_layout`; d_in == d_out allowed (in place).
 * batch polynomials, contiguous. */
int ntt_forward(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch,
                int out_layout, void *stream);

/* ---- coset low-degree extension (no reference counterpart) --------------------
 * The trace-commitment step of a STARK / Plonky2-style prover: from the N = M / 2^log_blowup coefficients of a polynomial P,
 * its values on the coset shift * <w_M>, M = 2^logn of THIS plan (the size-M plan).
 *
 * ntt_plan_set_coset: plan configuration, like ntt_plan_set_policy -- call it before the plan is shared between host
 * threads; calling it again replaces the setting.  log_blowup in [1, min(4, logn - 1)], shift in [1, p); anything else
 * returns NTT_E_ARG.  Builds on the device (no host table) the plan-owned vector of N words s[i] = shift^bitrev_logN(i)
 * mod p in the arithmetic's table form.  ntt_plan_clone copies the setting and the vector device-to-device;
 * ntt_forward / ntt_inverse on a plan with a coset set are unaffected.
 *
 * ntt_lde: d_in is [batch][N] words, d_out [batch][M] words in `out_layout`.  Defined at network level, hence for any
 * table:  d_out[b] = Forward_M(x_b),  x_b[i * 2^log_blowup] = d_in[b][i] * s[i] mod p,  every other word of x_b zero.
 * With kind-1 (cyclic) tables of size N and M from the same generator, and d_in = ntt_inverse (scaled, natural layout) of
 * the size-N plan applied to P's values on <w_N> -- the inverse network returns coefficients in bit-reversed order, and
 * bitrev_M(j) = bitrev_N(j) * 2^log_blowup for j < N -- this is d_out[b][k] = P_b(shift * w_M^k) in natural order: no
 * bit-reversal pass anywhere ("LDE").
 * Asynchronous on `stream`; no allocation, no host synchronisation.  From logn = 5 on the expansion happens inside the
 * first pass's load (nothing of size M is read or written before that pass's own store: N + M words of HBM traffic per row
 * for the pass); smaller sizes run an expansion kernel first (ntt_plan_info 10).  The decomposition is the one
 * ntt_plan_select(plan, batch) names, a pinned policy is honoured.  No access outside the caller's batch * N input words
 * and batch * M output words.
 * Errors: NTT_E_ARG for a null or misaligned pointer, batch out of range, a bad layout, no coset set, or when the byte
 * ranges of d_in and d_out overlap (d_in != d_out always); NTT_E_NOTABLE before twiddles are set; NTT_E_LAYOUT as ntt_forward.
 * batch == 0 is NTT_OK. */
int ntt_plan_set_coset(ntt_plan_t plan, int log_blowup, uint64_t shift);
int ntt_lde(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch, int out_layout, void *stream);

/* ---- coset interpolation (no reference counterpart) ---------------------------
 * The other half of a prover round: from values on the coset shift * <w_M>, M = 2^logn of this plan, back to coefficients
 * -- the "coset iFFT", an inverse transform followed by coeff[i] *= shift^-i, as ONE call.
 *
 * ntt_plan_set_coset_inverse: plan configuration under the rules of ntt_plan_set_coset (before the plan is shared between
 * host threads; a second call replaces the setting).  Independent of ntt_plan_set_coset: no blow-up, and neither call touches
 * the other's setting or vector.  shift in [1, p), else NTT_E_ARG; a shift that shares a factor with a composite p returns
 * NTT_E_NOTINVERTIBLE.  Builds on the device (no host table) the plan-owned vector of M words
 * u[i] = shift^(-bitrev_logM(i)) * M^-1 mod p in the arithmetic's table form: one more table's worth of device memory,
 * decomposition-agnostic like the tables.  ntt_plan_clone copies the setting and the vector device-to-device;
 * ntt_forward / ntt_inverse / ntt_lde on the plan are unaffected.
 *
 * ntt_coset_inverse: defined at network level, hence for any invertible table:
 *     d_out[b][i] = InvScaled_M(d_in[b])[i] * shift^(-bitrev_logM(i)) mod p,
 * InvScaled_M = exactly what ntt_inverse(..., scale = 1) computes.  d_in is in `in_layout`, d_out in natural order;
 * d_in == d_out allowed, as for ntt_inverse.  With kind-1 tables and d_in[b][k] = P_b(shift * w_M^k), d_out[b][i] is
 * coefficient bitrev_M(i) of P_b: the order ntt_lde consumes, still no bit-reversal pass anywhere ("LDE").
 * Asynchronous on `stream`; no allocation, no host synchronisation; the decomposition is the one ntt_plan_select(plan, batch)
 * names, a pinned policy is honoured.  From logn = 5 on, the inverse's last pass (the contiguous one, stages .. 0) multiplies
 * every output word by its word of u just before the store, where the scaled inverse multiplies by M^-1: no HBM traffic
 * beyond ntt_inverse's own.  Smaller sizes run the unscaled inverse and then a row-scaling kernel (ntt_plan_info 12).
 * No access outside the caller's batch * M words of each buffer; the vector read never leaves its M words.
 * Errors: NTT_E_ARG for a null or misaligned pointer, batch out of range, a bad layout or no coset-inverse shift set;
 * NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE / NTT_E_LAYOUT as ntt_inverse.  batch == 0 is NTT_OK. */
int ntt_plan_set_coset_inverse(ntt_plan_t plan, uint64_t shift);
int ntt_coset_inverse(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch, int in_layout, void *stream);

/* ---- row-major matrix batches: transform the COLUMNS of [N][pitch] (no reference counterpart) ----
 * A Plonky3-style trace is a row-major matrix [N][width]: each column is a polynomial, each row is what gets hashed into a
 * Merkle leaf.  These two entry points transform every column where it lies -- no transpose before or after.
 *
 * Layout.  `count` matrices lie one after another; word (m, r, c) is at ((m * N + r) * pitch + c), r < N = 2^logn of the plan,
 * c < width <= pitch.  Column c of matrix m is one polynomial.  Defined at network level, like everything above: the result equals
 * exactly what ntt_forward / ntt_inverse(scale) with NTT_LAYOUT_NATURAL give on that column laid out contiguously -- for any table,
 * all three word classes, `scale` as in ntt_inverse.
 * Footprint.  Only words with c < width are ever read or written.  Padding columns [width, pitch) of d_in may hold anything,
 * non-canonical words included; padding columns of d_out keep their contents.  A buffer of exactly
 * (count * N - 1) * pitch + width words is sufficient (the last row needs no padding).
 * In place and overlap.  d_in == d_out is allowed; any other overlap of the two byte ranges is NTT_E_ARG, as in ntt_lde.  Out of
 * place, the first executed pass reads d_in and writes d_out, the remaining passes run in place on d_out.
 * Launch.  Asynchronous on `stream`; no allocation, no host synchronisation.  count == 0 or width == 0 is NTT_OK.
 * Alignment.  Pointers 16-byte aligned, as everywhere.  pitch is any value >= width: the passes move single words, an odd pitch
 * is legal.  A pitch that is a multiple of 128 bytes is recommended: a workgroup's tile is 128 bytes of consecutive columns per
 * row (16 columns of 8-byte words, 32 of 4-byte words), which is then exactly one cache line per row instead of parts of two.
 * A tile whose columns lie partly or wholly at or beyond `width` idles those lanes: a width below 16 / 32 columns wastes the
 * rest of the tile and is still correct.
 *
 * How.  Pad every row to 2^w words in thought: the matrix is then, bit for bit, ONE polynomial of 2^(logn + w) words whose word
 * r * 2^w + c is (r, c).  Stage w + s of the size-2^(logn + w) network pairs words 2^(w + s) apart -- rows 2^s apart, same column
 * -- and wants the twiddle of block (index >> (w + s + 1)) = (r >> (s + 1)) among 2^(logn - s - 1) blocks: T[2^(logn-s-1) + block],
 * the plan's own N-word table at the index stage s of a single column uses.  So stages w .. w + logn - 1 of the virtual network
 * ARE the per-column networks, all 2^w columns at once, with twiddles that do not depend on the column.  The stages run as the
 * library's column passes (4..8 stages each, the fewest passes, split evenly: ntt_plan_info 13 / 96+ / 128+) launched on
 * (logn + w, first stage + w); only the word -> address map differs (row * pitch + column), and lanes at columns >= width are
 * idle.  w = max(LOG_C, ceil_log2(width)), LOG_C = 4 for 8-byte words and 5 for 4-byte words.  No contiguous pass, no transpose.
 *
 * Errors (existing codes only).  NTT_E_ARG: null or misaligned pointer, width > pitch, partial overlap, count >= 2^31, or a matrix
 * too large for the 32-bit in-tile byte offsets: the rule is N * pitch <= 2^NTT_MAX_LOGN words and logn + w <= NTT_MAX_LOGN, so
 * every index rule a size-2^28 transform obeys covers this one too.  NTT_E_LOGN: a plan with logn < 4 -- no column kernel
 * shape exists below four stages, and a prover has no such trace.  NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE as for ntt_forward /
 * ntt_inverse.
 * Not provided: other layouts (both entry points are natural order only), multi-device plans.  The coset operations on columns
 * follow the next prototypes. */
int ntt_forward_columns(ntt_plan_t plan, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, void *stream);
int ntt_inverse_columns(ntt_plan_t plan, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, int scale,
                        void *stream);

/* ---- coset LDE and coset interpolation on the columns of row-major matrices (no reference counterpart) ----
 * ntt_lde and ntt_coset_inverse for the trace layout of the section above: a prover round on [N][width] with no transpose and no
 * expanded, zero-filled intermediate.  No new plan state: ntt_lde_columns uses the setting and vector of ntt_plan_set_coset,
 * ntt_coset_inverse_columns those of ntt_plan_set_coset_inverse; ntt_plan_clone copies both.  Defined at network level, for any
 * (invertible) table and all three word classes.
 *
 * ntt_lde_columns.  M = 2^logn of the plan, beta the log_blowup of ntt_plan_set_coset, N = M >> beta.  d_in is `count` matrices
 * [N][in_pitch], d_out `count` matrices [M][out_pitch], the first `width` columns of each are live (width <= both pitches).  Column
 * c of output matrix m is exactly what ntt_lde(..., NTT_LAYOUT_NATURAL) gives on column c of input matrix m laid out contiguously:
 *     Forward_M(x),  x[i << beta] = d_in[(m * N + i) * in_pitch + c] * s[i] mod p,  every other word of x zero.
 * Out of place only: any overlap of the two byte ranges is NTT_E_ARG, d_in == d_out included.  The first executed pass reads d_in
 * and writes d_out, the other passes run in place on d_out; nothing of size M is read or written before the first pass's own
 * store.  In that pass a thread's 16 words are 16 consecutive rows of one column of which every 2^beta-th is live: it loads those
 * from row (row >> beta) of the compact matrix, multiplies by s[row >> beta] -- the multiplier depends on the ROW only -- and keeps
 * the others as zeros in registers.  Every first column pass has at least 4 stages >= beta, so there is no unfused fallback.
 * With kind-1 tables and d_in = ntt_inverse_columns (scaled) of the size-N plan on the trace, row k of d_out holds the values at
 * shift * w_M^k of every column: ready to hash ("Row-major trace").
 *
 * ntt_coset_inverse_columns.  Column c of the output is what ntt_coset_inverse(..., NTT_LAYOUT_NATURAL) gives on that column: row r
 * of InvScaled_M is multiplied by shift^(-bitrev_logM(r)).  The multiplication happens in the last executed pass (the one that
 * holds stage 0), just before its store, where ntt_inverse_columns(scale = 1) multiplies by the constant M^-1.  d_in == d_out is
 * allowed; any other overlap is NTT_E_ARG, as in ntt_inverse_columns.
 *
 * Footprint, launch and alignment are those of ntt_forward_columns: only words with c < width are touched, input padding may hold
 * non-canonical junk, output padding keeps its contents; buffers of exactly (count * rows - 1) * pitch + width words are sufficient,
 * rows = N for the input of ntt_lde_columns and M everywhere else; asynchronous, no allocation, no host synchronisation;
 * count == 0 or width == 0 is NTT_OK.
 * Errors (existing codes only).  NTT_E_ARG: null plan, null or misaligned pointer, width greater than a pitch, forbidden overlap,
 * count >= 2^31, no coset set (ntt_lde_columns) or no coset-inverse shift set (ntt_coset_inverse_columns), or the size rule of the
 * section above applied to the M-row matrix: M * pitch <= 2^NTT_MAX_LOGN words and logn + w <= NTT_MAX_LOGN (the compact source
 * obeys it with its own row count: N * in_pitch <= 2^NTT_MAX_LOGN words).  NTT_E_LOGN: logn < 4.  NTT_E_NOTABLE /
 * NTT_E_NOTINVERTIBLE as for ntt_forward_columns / ntt_inverse_columns.
 * Not provided: other layouts, multi-device plans. */
int ntt_lde_columns(ntt_plan_t plan, const void *d_in, size_t in_pitch, void *d_out, size_t out_pitch, size_t width, size_t count,
                    void *stream);
int ntt_coset_inverse_columns(ntt_plan_t plan, const void *d_in, void *d_out, size_t width, size_t pitch, size_t count, void *stream);

/* Profiling twin of ntt_forward (the reference brackets one kernel iteration with
 * trace events, src/aie_core.cc:129-131, src/aie2.py:168,316): identical launches
 * with a hipEvent recorded on `stream` around every HBM pass; blocks until done.
 * Writes the number of passes to *n_passes and their durations to ms_per_pass[]
 * (capacity max_passes).  The pass count is that of the alternative chosen for THIS batch
 * (ntt_plan_select), which can exceed ntt_plan_info(plan, 3) (the default decomposition): size the
 * array from ntt_plan_info(plan, 8) = the largest pass count over all alternatives (never above 7);
 * a smaller capacity returns NTT_E_ARG with *n_passes set to the count needed. */
int ntt_forward_profile(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch,
                        int out_layout, void *stream, float *ms_per_pass, int max_passes,
                        int *n_passes);

/* Exact inverse of ntt_forward (no reference counterpart; BASELINE configs 3-4):
 * stages logN-1..0, (u, v) -> (u + v/T, u - v/T), then * N^-1 when scale != 0.
 * d_in is in `in_layout` (what ntt_forward produced), d_out natural order. */
int ntt_inverse(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch,
                int in_layout, int scale, void *stream);

/* d_out[i] = d_a[i] * d_b[i] * scale mod p over batch*N words (scale in [0,p),
 * 1 = plain product).  Any of the pointers may alias. */
int ntt_pointwise_mul(ntt_plan_t plan, const void *d_a, const void *d_b, void *d_out,
                      size_t batch, uint64_t scale, void *stream);

/* Negacyclic product c = a*b mod (x^N + 1, p) with a kind-2 table loaded (no reference counterpart; BASELINE config 4):
 * c = Fwd( InvU(a) . InvU(b) . N^-1 ) with the unscaled inverse network InvU.  Sizes N >= 2^7
 * (Goldilocks) / N >= 2^6 (4-byte words) run the column passes (N >= 2^13 only) of both inverse transforms, then ONE
 * fused middle launch per unit of the first pass (last inverse pass of a and of b, word-by-word product, first forward
 * pass: 3 N words of HBM traffic instead of 7 N; for single-pass sizes that launch is the whole product), then the forward
 * column passes (4-byte words: one launch up to N = 2^13); smaller sizes fold the product into the load of the forward
 * transform's first pass.  d_a and d_b are overwritten (scratch); d_out may alias d_a or d_b.  When d_b directly follows
 * d_a in memory (one [2*batch][N] buffer) both operand transforms run as one launch per pass. */
int ntt_polymul_negacyclic(ntt_plan_t plan, void *d_a, void *d_b, void *d_out,
                           size_t batch, void *stream);

/* The same product with operand b PREPARED: b^ = InvU(b), computed once and reused -- a public matrix row, a key-switching key, a
 * plaintext mask; often ONE polynomial that multiplies every row of a batch.
 *
 * ntt_polymul_prepare writes exactly what ntt_inverse(plan, d_b, d_bhat, rows, NTT_LAYOUT_NATURAL, 0, stream) writes, bit for bit
 * (tests/test_gpu_product_pre.py asserts it).  The prepared form is NOT opaque: [rows][N] canonical words in natural order,
 * independent of the plan's decomposition alternative and of the batch, valid for every clone of the plan; a caller may produce
 * it itself.  d_b == d_bhat is allowed.
 *
 * ntt_polymul_negacyclic_pre: d_out[r] = Fwd( InvU(d_a[r]) . d_bhat[bhat_rows == 1 ? 0 : r] . N^-1 ).  With bhat_rows == batch this
 * is word for word what ntt_polymul_negacyclic(plan, a, b, out, batch) returns for bhat = prepare(b); bhat_rows == 1 is the
 * broadcast: the one row multiplies every row of d_a.  Any other bhat_rows is NTT_E_ARG.  d_a is overwritten (scratch: its inverse
 * column passes run in place), d_bhat is never written, d_out may alias d_a; d_a or d_out overlapping the bhat_rows * N words of
 * d_bhat is NTT_E_ARG, as are a null or misaligned pointer and a batch out of range; NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE as for
 * ntt_polymul_negacyclic; batch == 0 is NTT_OK.  The decomposition is the one ntt_plan_select(plan, batch) names.  Asynchronous on
 * `stream`, no allocation, no host synchronisation; nothing outside the caller's batch * N words of d_a / d_out and
 * bhat_rows * N words of d_bhat is accessed.
 * Where the fused middle pass runs (N >= 2^7 Goldilocks and the general 64-bit modulus, N >= 2^6 4-byte words, a first pass of at
 * most 12 / 13 stages) the call is a's inverse column passes, ONE middle launch that reads a and b^ and writes the product's first
 * forward pass, and the forward column passes: at a two-pass size 2 N + 3 N + 2 N = 7 N words of HBM traffic and two transforms'
 * butterflies, against 9 N words and three transforms for ntt_polymul_negacyclic (a single-pass size: one launch, 3 N words).  That
 * claim holds ONLY there: every other size runs a's whole unscaled inverse, then the forward transform with b^ folded into the load
 * of its first pass (per row) or after a separate in-place product launch (broadcast). */
int ntt_polymul_prepare(ntt_plan_t plan, const void *d_b, void *d_bhat, size_t rows, void *stream);
int ntt_polymul_negacyclic_pre(ntt_plan_t plan, void *d_a, const void *d_bhat, size_t bhat_rows,
                               void *d_out, size_t batch, void *stream);

/* The negacyclic INNER product with prepared operands -- an RLWE key switch sum_k digit_k(a) * ksk_k, a module-LWE row sum_k A[i][k] * s[k], a
 * relinearisation -- summed inside the middle pass:
 *   d_out[r] = Fwd( N^-1 . sum_{k < terms} InvU(d_a[k][r]) . d_bhat[k][bhat_rows == 1 ? 0 : r] ),  r < batch,  kind-2 table loaded.
 * d_a is [terms][batch][N] words, contiguous; it is scratch and is overwritten (the inverse column passes run in place, and the sizes
 * without a fused middle leave the sum in term 0's block).  d_bhat is [terms][bhat_rows][N] canonical words in natural order, row (k, .)
 * exactly what ntt_polymul_prepare writes; it is never written.  bhat_rows is batch, or 1: ONE polynomial per term multiplies every row
 * (the key-switching case).  d_out is [batch][N].
 * Values: with terms == 1 the words are ntt_polymul_negacyclic_pre's, bit for bit; for every `terms` they are the sum mod p of the
 * `terms` separate ntt_polymul_negacyclic_pre results (all canonical, so the equality is exact), by linearity of Fwd -- ONE forward
 * transform runs, whatever `terms`, and terms + 1 modular products per word instead of 2 * terms.
 * d_out may be d_a (term 0's block) or lie apart from all terms * batch * N words of d_a; any other overlap with d_a is NTT_E_ARG, as is any
 * overlap of d_a or d_out with the terms * bhat_rows * N words of d_bhat, a null or misaligned pointer, bhat_rows other than 1 or batch,
 * terms == 0 with batch > 0, and terms * batch > 2^31 - 1.  NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE as for ntt_polymul_negacyclic_pre;
 * batch == 0 is NTT_OK whatever the other arguments.  The decomposition is the one ntt_plan_select(plan, batch) names -- selected by
 * `batch`, not by terms * batch -- and a pinned policy is honoured.  Asynchronous on `stream`, no allocation, no host synchronisation;
 * nothing outside the caller's terms * batch * N words of d_a, terms * bhat_rows * N words of d_bhat and batch * N words of d_out is accessed.
 * Where the fused middle pass runs (the sizes named at ntt_polymul_negacyclic_pre) the call is a's inverse column passes as one launch
 * each over terms * batch rows, ONE middle launch that reads every term's unit of a and of b^ and writes the first forward pass of the
 * sum, and the forward column passes over batch rows.  Derived (not measured with counters) HBM traffic at a two-pass size, K = terms:
 * 2 K N + (2 K + 1) N + 2 N = (4 K + 3) N words, against 7 K N for K calls of ntt_polymul_negacyclic_pre plus 3 (K - 1) N for the sums
 * a caller adds; a single-pass size: one launch, (2 K + 1) N words.  (A broadcast reads the K N words of b^ once per workgroup, from
 * cache for all but the first.)  That derivation holds ONLY there: every other size runs the whole unscaled inverse over terms * batch
 * rows, one small launch that sums the products into term 0's block, and the plain forward transform -- still one forward transform,
 * but a pass more each way: (6 K + 5) N words at a two-pass size.  Besides the sizes named there, that is the path of the general 64-bit
 * modulus where the first pass has 10 stages and of 4-byte words where it has 13: the summed middle has no kernel for those two units. */
int ntt_polymul_dot_pre(ntt_plan_t plan, void *d_a, const void *d_bhat, size_t bhat_rows, size_t terms,
                        void *d_out, size_t batch, void *stream);

/* SEVERAL negacyclic inner products of ONE operand a with prepared operands -- the two polynomials of an RLWE key switch,
 * sum_k digit_k(a) * ksk0_k and sum_k digit_k(a) * ksk1_k, from the same digits; the rows of a module-LWE product A . s from the same s:
 *   d_out[j][r] = Fwd( N^-1 . sum_{k < terms} InvU(d_a[k][r]) . d_bhat[j][k][bhat_rows == 1 ? 0 : r] ),  j < outs,  r < batch,  kind-2 table.
 * d_a is [terms][batch][N] words, contiguous; it is scratch and is overwritten, as in ntt_polymul_dot_pre.  d_bhat is
 * [outs][terms][bhat_rows][N] canonical words: block j is exactly an operand of ntt_polymul_dot_pre; it is never written.  bhat_rows is
 * batch, or 1.  d_out is [outs][batch][N].
 * Values: block j of d_out equals what ntt_polymul_dot_pre writes for a copy of a and block j of d_bhat, bit for bit, whatever the
 * decomposition and on every clone.
 * UNLIKE ntt_polymul_dot_pre, d_out may NOT overlap d_a anywhere, not even term 0's block: the middle launches of later outputs still read
 * a.  Any overlap of d_out with the terms * batch * N words of d_a is NTT_E_ARG, as is any overlap of d_a or d_out with the
 * outs * terms * bhat_rows * N words of d_bhat, a null or misaligned pointer, bhat_rows other than 1 or batch, terms == 0 or outs == 0 with
 * batch > 0, and terms * batch or outs * batch > 2^31 - 1.  NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE as for ntt_polymul_dot_pre; batch == 0 is
 * NTT_OK whatever the other arguments.  The decomposition is the one ntt_plan_select(plan, batch) names, and a pinned policy is
 * honoured.  Asynchronous on `stream`, no allocation, no host synchronisation; nothing outside the three word ranges named above is accessed.
 * Where ntt_polymul_dot_pre runs its fused middle pass, the call is a's inverse column passes as ONE launch each over terms * batch rows --
 * once, whatever `outs` --, then the middle launches, ONE per pair of outputs where the two-output kernel is used (4-byte words and the
 * general 64-bit modulus, not Goldilocks: DESIGN.md section 3.2; it runs the last inverse pass of every term once and sums into two accumulators) plus one summed launch for
 * the last output of an odd `outs`, else one summed launch per output; then the forward column passes as ONE launch each over outs * batch
 * rows.  Derived (not measured with counters) at a two-pass size, K = terms, J = outs, paired: (2 K + ceil(J/2) K + J K + 3 J) N words of HBM
 * traffic and K + ceil(J/2) K + 2 J half-transforms, against J (4 K + 3) N words, 2 K N more per copy of a, and J (2 K + 2) half-transforms
 * for J calls of ntt_polymul_dot_pre.  Every other size runs the unscaled inverse over terms * batch rows, ONE small launch that writes
 * the scaled sums of every output, and ONE plain forward transform over outs * batch rows.  No path loops over terms on the host, none
 * transforms a more than once. */
int ntt_polymul_matvec_pre(ntt_plan_t plan, void *d_a, const void *d_bhat, size_t bhat_rows, size_t terms, size_t outs, void *d_out,
                           size_t batch, void *stream);

/* BALANCED GADGET DECOMPOSITION -- the digit_k(a) of the examples above, for all three word classes.  Parameters log_base = w (B = 2^w),
 * levels = K, low_bits = l; p is the plan's modulus.  For a canonical word a, in integers (not residues):
 *   s = +1, m = a          if a <= (p - 1) / 2,  else  s = -1, m = p - a                (centred magnitude, m <= (p - 1) / 2 < 2^63)
 *   u = (m + h) >> l,      h = 2^(l - 1) for l > 0, else 0                              (rounds half away from zero)
 *   v = u + C,             C = sum_{k < K - 1} 2^(k w + w - 1)                          (only the lower K - 1 digits are biased)
 *   e_k = ((v >> k w) & (B - 1)) - B / 2  for k < K - 1, in [-B/2, B/2);   e_{K-1} = v >> (K - 1) w, unmasked, non-negative
 *   digit_k(a) = s . e_k mod p, a canonical word.
 * Then sum_k e_k B^k = u exactly, |s m - s u 2^l| <= 2^(l - 1), and digit_k(p - a) = -digit_k(a) mod p.
 * Argument rule (anything else is NTT_E_ARG): 1 <= w <= 31, K >= 1, 0 <= l, l + (K - 1) w <= 63 (v then fits 64 unsigned bits for every
 * p < 2^64), 2^(w - 1) < p, and (u_max >> (K - 1) w) + 1 < p with u_max = ((p - 1) / 2 + h) >> l (every digit then has a magnitude below p).
 * Goldilocks with (w, K, l) = (16, 4, 0) is legal and exact; (8, 3, 40) is the usual approximate TFHE setting.
 *
 * ntt_gadget_decompose: d_a is [polys][batch][N] canonical words, never written; d_digits is [polys][levels][batch][N], word
 * (q, k, r, i) = digit_k(d_a[q][r][i]) -- with t = q * levels + k exactly an operand `a` of ntt_polymul_dot_pre / ntt_polymul_matvec_pre with
 * terms = polys * levels.  The two byte ranges must lie apart; null or misaligned pointers, polys == 0 and polys * levels * batch >
 * 2^31 - 1 are NTT_E_ARG; batch == 0 is NTT_OK.  ONE small launch; needs only p, so it works before twiddles are set. */
int ntt_gadget_decompose(ntt_plan_t plan, const void *d_a, size_t polys, size_t batch, int log_base, int levels, int low_bits, void *d_digits,
                         void *stream);

/* TFHE external product / key switch FROM COEFFICIENTS: ntt_polymul_matvec_pre of the gadget digits of a, decomposed on the way:
 *   d_out[j][r] = Fwd( N^-1 . sum_t InvU(digit_{t mod K}(d_a[t div K][r])) . d_bhat[j][t][bhat_rows == 1 ? 0 : r] ),  t < polys * levels, j < outs.
 * d_a is [polys][batch][N] canonical words; it is CONST and left intact on every path -- the one behavioural difference from the other
 * products.  d_bhat is [outs][polys * levels][bhat_rows][N], as for ntt_polymul_matvec_pre; d_out is [outs][batch][N].  d_work is caller
 * scratch of polys * levels * batch * N words, required non-null; its contents afterwards are unspecified and the fused path may leave it
 * untouched (no hidden allocation, as everywhere in this library).
 * Values: block j of d_out equals, bit for bit, what ntt_polymul_matvec_pre writes when it is given ntt_gadget_decompose's output as a,
 * for every decomposition alternative and on every clone.
 * All four ranges (d_a, d_work, d_bhat, d_out) are pairwise disjoint, else NTT_E_ARG.  The other rules are those of
 * ntt_polymul_matvec_pre with terms = polys * levels (null or misaligned pointer, bhat_rows not 1 or batch, polys == 0 or outs == 0 with
 * batch > 0, the 2^31 - 1 row limits, NTT_E_NOTABLE / NTT_E_NOTINVERTIBLE, batch == 0 is NTT_OK whatever the other arguments), plus the
 * argument rule of the decomposition.  Asynchronous on `stream`, no allocation, no host synchronisation; the decomposition is
 * selected by `batch`, and a pinned policy is honoured.
 * Where the plan runs ONE pass for this batch, ntt_polymul_dot_pre runs its fused middle and the unit has digit kernels
 * (ntt_plan_info 15), the call is the middle launches alone -- one per pair of outputs where the two-output kernel
 * is used plus one for an odd last output, else one per output -- which read d_a directly and decompose in registers.  Derived (not
 * measured with counters), P = polys, K = levels, J = outs, broadcast b^: (P + J) N words of HBM traffic per row (the K - 1 re-reads of a
 * unit are expected to come from cache) against (P + 2 P K + J) N and one more launch.  Everywhere else -- a multi-pass size, a size
 * without a fused middle, a unit without a digit kernel, a pinned alternative without a middle -- ONE launch of the decomposition
 * kernel d_a -> d_work, then exactly ntt_polymul_matvec_pre on d_work. */
int ntt_polymul_gadget_pre(ntt_plan_t plan, const void *d_a, size_t polys, int log_base, int levels, int low_bits, void *d_work,
                           const void *d_bhat, size_t bhat_rows, size_t outs, void *d_out, size_t batch, void *stream);

/* SIGNED NEGACYCLIC MAPS -- the coefficient permutations that come BEFORE the digits in the two workloads above: a blind-rotation step
 * ACC <- ACC + bsk_i [.] (X^e_r . ACC - ACC), the exponent per row, data-dependent and already on the device, and a slot rotation
 * a(X) -> a(X^g) followed by a gadget key switch.  Defined at word level for all three word classes from the plan's p and logn alone.
 * N = 2^logn, M2 = 2N - 1, j < N the DESTINATION index; both maps are one rule t -> (src, neg) = (t & (N - 1), (t & N) != 0):
 *   NTT_MAP_MONOMIAL      y = X^e . a mod (X^N + 1):  e = exp & M2 -- ANY uint32_t is legal and is taken mod 2N, so a caller's -a_i as an
 *                         unsigned word works (2N divides 2^32) --,  t = (j - e) & M2
 *   NTT_MAP_AUTOMORPHISM  y(X) = a(X^g), g odd, 1 <= g < 2N:  t = (j . ginv) & M2, ginv = g^-1 mod 2N computed on the host (the 32-bit
 *                         product may wrap: harmless, logn <= 28)
 *   value                 x = a[src];  neg and x != 0:  x = p - x
 *   flag NTT_MAP_MINUS_IDENTITY (bit 0 of `flags`; any other bit is NTT_E_ARG):  x = x >= a[j] ? x - a[j] : x + (p - a[j])  (y - a mod p)
 * digit_k(p - a) = -digit_k(a), so the digits of the mapped word are those of the definition above.
 * Shared rules: d_in / d_a is [polys][batch][N] canonical words and is never written.  `param` is the exponent of every row (monomial,
 * d_exp == NULL) or g (automorphism).  d_exp is a device array of `batch` words, monomial only; row r of EVERY polynomial uses d_exp[r]
 * (the polynomials of one GLWE ciphertext rotate together).  NTT_E_ARG: an unknown kind or flag bit; an even g or g >= 2N; d_exp != NULL
 * with the automorphism; d_exp not 4-byte aligned; d_exp[0 .. batch) overlapping any written range; null or misaligned data pointers;
 * polys == 0; the 2^31 - 1 row limits of ntt_gadget_decompose.  batch == 0 is NTT_OK.  Asynchronous on `stream`, no allocation, no host
 * synchronisation: the exponents are read on the device.
 *
 * ntt_negacyclic_map: d_out is [polys][batch][N].  Out of place only -- the gather reads the whole row --: any overlap of the two ranges
 * is NTT_E_ARG.  ONE launch; like ntt_gadget_decompose it needs no twiddles.
 *
 * ntt_gadget_decompose_map: d_digits is, bit for bit, ntt_gadget_decompose of ntt_negacyclic_map's output, in ONE launch: each source
 * word is gathered once and its `levels` digits are written with 128-bit non-temporal stores.
 *
 * ntt_polymul_gadget_map_pre: block j of d_out is, bit for bit, what ntt_polymul_gadget_pre writes for the mapped operand; with a
 * non-null d_addend ([outs][batch][N] canonical words) d_addend[j] is added mod p.  It ALWAYS takes the decomposition-kernel route: one
 * launch of the map kernel d_a -> d_work (the digits of the mapped words), then exactly ntt_polymul_matvec_pre on d_work, then, with an
 * addend, one elementwise in-place launch on d_out.  ntt_plan_info 15 does not apply to it.  d_a, d_work, d_bhat and d_out are pairwise
 * disjoint.  d_addend may be d_a itself (the CMUX / blind-rotation case, outs == polys) or any range disjoint from d_work and d_out; it is
 * only read.  The remaining rules are those of ntt_polymul_gadget_pre.
 * Derived, NOT measured with counters (P = polys, K = levels, J = outs, words per row): against ntt_negacyclic_map followed by
 * ntt_polymul_gadget_pre where that call runs the decomposition kernel, the fused decomposition saves the mapped copy's write and
 * re-read, 2 P N words, and one launch per call.  The accumulate is a launch of its own after the forward passes and costs 3 J N words
 * (read d_out, read d_addend, write d_out); fusing it into the last forward pass is not done. */
enum { NTT_MAP_MONOMIAL = 0, NTT_MAP_AUTOMORPHISM = 1 };
enum { NTT_MAP_MINUS_IDENTITY = 1 };
int ntt_negacyclic_map(ntt_plan_t plan, const void *d_in, void *d_out, size_t polys, size_t batch, int kind, uint32_t param,
                       const uint32_t *d_exp, int flags, void *stream);
int ntt_gadget_decompose_map(ntt_plan_t plan, const void *d_a, size_t polys, size_t batch, int kind, uint32_t param, const uint32_t *d_exp,
                             int flags, int log_base, int levels, int low_bits, void *d_digits, void *stream);
int ntt_polymul_gadget_map_pre(ntt_plan_t plan, const void *d_a, size_t polys, int kind, uint32_t param, const uint32_t *d_exp, int flags,
                               int log_base, int levels, int low_bits, void *d_work, const void *d_bhat, size_t bhat_rows, size_t outs,
                               const void *d_addend, void *d_out, size_t batch, void *stream);

/* Precondition check (blocking, diagnostic): how many of the batch*N words are >= p.  The transforms
 * assume canonical residues, as the reference's vector_modadd / vector_modsub do (src/aie_core.cc:41-62);
 * a non-canonical word gives an unspecified (but memory-safe) result: no kernel reads or writes outside the caller's
 * batch*N words whatever they hold (tests/test_emu_asan.py: the kernels' index rules under AddressSanitizer, exact-size buffers). */
int ntt_count_noncanonical(ntt_plan_t plan, const void *d_buf, size_t batch, uint64_t *host_count);

/* Reference-style partial network (test_stage hook, src/test.cpp:55-58, 67):
 * run stages 0..stage only.  Slow path (one launch per stage), for bring-up. */
int ntt_forward_stages(ntt_plan_t plan, const void *d_in, void *d_out, size_t batch,
                       int stage, void *stream);

#ifdef __cplusplus
}
#endif
#endif
