// kernels.h -- type-erased launch interface between the C-ABI (ntt_api.hip) and the kernel translation units: one entry
// point per operation, the field travels as data (launch.h: FieldParams).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace ntt {

// The pass kernels of one (field, direction): defined in pass_kernel.inc, instantiated by kernels_<field>_<dir>.hip (one
// translation unit each: the build's parallelism).  hipErrorInvalidValue for an unsupported (contig, log_m) combination.
// ONE explicit instantiation per specialisation in the whole library: a translation unit that sees the definition must not
// use any other specialisation (it would be instantiated there, with that unit's kernels), hence the extern templates.
template <class F, bool INV>
hipError_t launch_pass_of(bool contig, int log_m, const ErasedArgs &a, hipStream_t s);
#define NTT_PASS_UNIT(F) \
    extern template hipError_t launch_pass_of<F, false>(bool, int, const ErasedArgs &, hipStream_t); \
    extern template hipError_t launch_pass_of<F, true>(bool, int, const ErasedArgs &, hipStream_t);
NTT_PASS_UNIT(FieldGL) NTT_PASS_UNIT(FieldM32) NTT_PASS_UNIT(FieldM64)
#undef NTT_PASS_UNIT
hipError_t launch_pass(bool inverse, bool contig, int log_m, const ErasedArgs &a, hipStream_t s);  // misc_kernels.hip: by a.field

// The matrix twins of the column passes (launch.h: mat_dispatch), same units, same instantiation rule.  a.n / a.s0 are the virtual
// polynomial's, a.mat_* the matrix geometry; hipErrorInvalidValue outside 4..8 stages or when fill_pass_args refuses the arguments.
template <class F, bool INV>
hipError_t launch_mat_of(int log_m, const ErasedArgs &a, hipStream_t s);
#define NTT_MAT_UNIT(F) \
    extern template hipError_t launch_mat_of<F, false>(int, const ErasedArgs &, hipStream_t); \
    extern template hipError_t launch_mat_of<F, true>(int, const ErasedArgs &, hipStream_t);
NTT_MAT_UNIT(FieldGL) NTT_MAT_UNIT(FieldM32) NTT_MAT_UNIT(FieldM64)
#undef NTT_MAT_UNIT
hipError_t launch_mat_pass(bool inverse, int log_m, const ErasedArgs &a, hipStream_t s);  // misc_kernels.hip: by a.field

// Fused middle of a negacyclic product (pass.h: run_product_pass): per 2^log_m-word unit, inverse CONTIG pass of a.in
// and of a.in2, word-by-word product * pw_scale, forward CONTIG pass -> a.out.  tw = inverse table, tw2 = forward table.
// hipErrorInvalidValue when this (word size, log_m) has no fused kernel or the batch does not fit one grid (launch.h:
// product_mid_used / product_mid_fits; callers then run the separate passes).  product_kernel.inc, kernels_<field>_product.hip
template <class F>
hipError_t launch_product_mid_of(int log_m, const ErasedArgs &a, hipStream_t s);
extern template hipError_t launch_product_mid_of<FieldGL>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_mid_of<FieldM32>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_mid_of<FieldM64>(int, const ErasedArgs &, hipStream_t);
// ... with operand b prepared (a.in2_prepared: a.in2 is InvU(b), [batch][N] canonical words, or one row when a.in2_broadcast): the
// second inverse pass is gone.  Kernels of their own (run_product_pass<.., PRE = true>), same unit sizes, kernels_<field>_product_pre.hip
template <class F>
hipError_t launch_product_pre_mid_of(int log_m, const ErasedArgs &a, hipStream_t s);
extern template hipError_t launch_product_pre_mid_of<FieldGL>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_pre_mid_of<FieldM32>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_pre_mid_of<FieldM64>(int, const ErasedArgs &, hipStream_t);
// ... summed over a.dot_terms terms (ntt_polymul_dot_pre): per unit, for every term the inverse pass of its block of a and the product
// with its block of the prepared operand, accumulated in registers; ONE scaling by pw_scale, forward pass -> a.out.  Kernels of their
// own (run_product_dot_pass), same unit sizes, kernels_<field>_product_dot.hip
template <class F>
hipError_t launch_product_dot_mid_of(int log_m, const ErasedArgs &a, hipStream_t s);
extern template hipError_t launch_product_dot_mid_of<FieldGL>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_dot_mid_of<FieldM32>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_dot_mid_of<FieldM64>(int, const ErasedArgs &, hipStream_t);
// ... for two outputs of one operand a at once (ntt_polymul_matvec_pre; a.mv_outs == 2): per unit and term ONE inverse pass of a's block,
// two accumulators, then two forward passes -> a.out and a.out + a.mv_out_stride.  Kernels of their own under a register bound of their
// own (run_product_mv_pass), the unit sizes of launch.h's product_mv_unit, kernels_<field>_product_mv.hip
template <class F>
hipError_t launch_product_mv_mid_of(int log_m, const ErasedArgs &a, hipStream_t s);
extern template hipError_t launch_product_mv_mid_of<FieldGL>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_mv_mid_of<FieldM32>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_mv_mid_of<FieldM64>(int, const ErasedArgs &, hipStream_t);
// ... the digit variants of the last two (ntt_polymul_gadget_pre; a.gad_levels > 0): a.in is [a.dot_terms / a.gad_levels][batch][N]
// canonical words, decomposed in registers between the load and the first inverse round (pass.h: gadget_digit); a summed launch, or a
// two-output one (a.mv_outs == 2) where the unit has that kernel.  The unit sizes of launch.h's product_gadget_unit,
// kernels_<field>_product_gad.hip
template <class F>
hipError_t launch_product_gad_mid_of(int log_m, const ErasedArgs &a, hipStream_t s);
extern template hipError_t launch_product_gad_mid_of<FieldGL>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_gad_mid_of<FieldM32>(int, const ErasedArgs &, hipStream_t);
extern template hipError_t launch_product_gad_mid_of<FieldM64>(int, const ErasedArgs &, hipStream_t);
hipError_t launch_product_mid(int log_m, const ErasedArgs &a, hipStream_t s);  // misc_kernels.hip: by a.field, a.gad_levels, a.in2_prepared, a.dot_terms and a.mv_outs

#if defined(NTT_EXPERIMENT)
// Tools-side experiment, NOT part of libntt_hip.so (tools/fused_gl16.hip, libntt_hip_exp.so only):
// N = 2^16 Goldilocks forward as one persistent XCD-local launch: memset + fused +
// check; must be followed by the ordinary passes with skip_if = fused_gl16_ok_word(ctl).
size_t fused_gl16_ctl_bytes(size_t max_batch);
const void *fused_gl16_ok_word(const void *ctl);
hipError_t launch_fused_gl16(const void *in, void *out, const void *tw, size_t batch, void *ctl_mem, hipStream_t s,
                             int dbg = 0);
#endif

// The small kernels (misc_kernels.hip).  Field elements travel as uint64_t whatever the word size.
// elementwise c = a*b*scale (scale in plain form; scale == 1 skips the second product)
hipError_t launch_pointwise(const FieldParams &fp, const void *a, const void *b, void *c, size_t count, uint64_t scale, hipStream_t s);
// in place: buf[r][i] = buf[r][i] * row[i] * scale (plain form all), buf: [batch][2^n] words, row: 2^n words -- the broadcast product of
// ntt_polymul_negacyclic_pre at the sizes without a fused middle
hipError_t launch_pointwise_row(const FieldParams &fp, void *buf, const void *row, int n, size_t batch, uint64_t scale, hipStream_t s);
// in place on term 0: a[0][r][i] = scale2 * sum_k a[k][r][i] * bhat[k][bhat_rows == 1 ? 0 : r][i] / R^2 -- plain words in and out when scale2
// is the scale times R^2 in table form (sequence.h: pw_scale_form); a: [terms][batch][2^n] words, bhat: [terms][bhat_rows][2^n] words, read
// only.  The sum of ntt_polymul_dot_pre at the sizes without a fused middle
hipError_t launch_dot_rows(const FieldParams &fp, void *a, const void *bhat, int n, size_t batch, size_t bhat_rows, size_t terms, uint64_t scale2, hipStream_t s);
// out[j][r][i] = scale2 * sum_k a[k][r][i] * bhat[j][k][bhat_rows == 1 ? 0 : r][i] / R^2 for every j < outs, as launch_dot_rows computes it for one j;
// a: [terms][batch][2^n] words, read only here; bhat: [outs][terms][bhat_rows][2^n] words, read only; out: [outs][batch][2^n] words, apart from
// both.  ONE launch: the sums of ntt_polymul_matvec_pre at the sizes without a fused middle
hipError_t launch_matvec_rows(const FieldParams &fp, const void *a, const void *bhat, void *out, int n, size_t batch, size_t bhat_rows, size_t terms, size_t outs,
                              uint64_t scale2, hipStream_t s);
// digits[q][k][r][i] = digit_k(a[q][r][i]) (pass.h: gadget_digit), k < levels: a is [polys][batch][2^n] canonical words, read only; digits is
// [polys][levels][batch][2^n] words, apart from a.  The decomposition of ntt_gadget_decompose, and of ntt_polymul_gadget_pre where the
// middle launch does not decompose.  Needs p alone, no table
hipError_t launch_gadget_decompose(const FieldParams &fp, const void *a, void *digits, int n, size_t polys, size_t batch, int log_base, int levels, int low_bits,
                                   hipStream_t s);
// the signed negacyclic map of every row (negacyclic_map.h): out[q][r][j] = +-a[q][r][src(j)], minus a[q][r][j] with minus_identity; kind 0 the
// monomial X^e with e = d_exp[r] (a device array of batch words) or, d_exp null, q for every row; kind 1 the automorphism with q = g^-1 mod 2N.
// levels == 0: out is [polys][batch][2^n] words; levels > 0: out is [polys][levels][batch][2^n], the gadget digits of the mapped words (what
// launch_gadget_decompose writes for them), each source word gathered once.  a is read only and lies apart from out.  ONE launch; p alone
hipError_t launch_negacyclic_map(const FieldParams &fp, const void *a, void *out, int n, size_t polys, size_t batch, int kind, uint32_t q, const uint32_t *d_exp,
                                 int minus_identity, int log_base, int levels, int low_bits, hipStream_t s);
// in place: out[i] = out[i] + addend[i] mod p, canonical words, i < count -- the accumulate of ntt_polymul_gadget_map_pre
hipError_t launch_add_rows(const FieldParams &fp, void *out, const void *addend, size_t count, hipStream_t s);
// device-side table generation (no host upload): T[i] = base^e_kind(i), table form
hipError_t launch_gen_table(const FieldParams &fp, void *T, int logn, int kind, uint64_t base_m, uint64_t one_m, hipStream_t s);
// coset vector of ntt_plan_set_coset: s[i] = shift^bitrev_logn(i mod 2^logn), table form, i < len (len = max(2^logn, 4));
// one_m = the table form of a constant c instead of 1: s[i] * c (ntt_plan_set_coset_inverse: shift^-1 and c = N^-1)
hipError_t launch_gen_coset(const FieldParams &fp, void *s_out, int logn, uint32_t len, uint64_t shift_m, uint64_t one_m, hipStream_t s);
// the separate expansion of ntt_lde: out[b][i << beta] = in[b][i] * s[i], zeros between; in: [batch][2^(n - beta)], out: [batch][2^n] words
hipError_t launch_lde_expand(const FieldParams &fp, const void *in, const void *s_vec, void *out, int n, int beta, size_t batch, hipStream_t s);
// the separate scaling of ntt_coset_inverse, in place: buf[b][i] *= u[i]; buf: [batch][2^n] words, u: max(2^n, 4) words, table form
hipError_t launch_row_scale(const FieldParams &fp, void *buf, const void *u_vec, int n, size_t batch, hipStream_t s);
// out[i] = T[i] * c (table form both): the N/2 scaled stage-0 twiddles of the inverse transform (8-byte words only)
hipError_t launch_scale_table(const FieldParams &fp, const void *T, void *out, size_t count, uint64_t c_m, hipStream_t s);
// number of words >= p in a buffer (precondition check); d_out = one zeroed 64-bit device word
hipError_t launch_count_noncanonical(const void *a, size_t count, int word_bytes, uint64_t p, void *d_out, hipStream_t s);
// one stage of the network, one thread per butterfly (bring-up path, test_stage hook)
hipError_t launch_stage(const FieldParams &fp, void *data, const void *tw, int n, int stage, size_t batch, hipStream_t s);

}  // namespace ntt
