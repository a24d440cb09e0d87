// product_kernel.inc -- executor, __global__ wrapper and launcher of the product's fused middle pass (pass.h:
// run_product_pass).  Included by the three kernels_<field>_product.hip translation units, which define NTT_FIELD, and by the three
// kernels_<field>_product_pre.hip ones, which define NTT_PRODUCT_PRE as well: the same middle with operand b prepared
// (run_product_pass<.., PRE = true>, ntt_polymul_negacyclic_pre), and by the three kernels_<field>_product_dot.hip ones, which define
// NTT_PRODUCT_DOT: that middle summed over the terms of an inner product (run_product_dot_pass, ntt_polymul_dot_pre), and by the three
// kernels_<field>_product_mv.hip ones, which define NTT_PRODUCT_MV: the summed middle for two outputs at once (run_product_mv_pass,
// ntt_polymul_matvec_pre), and by the three kernels_<field>_product_gad.hip ones, which define NTT_PRODUCT_GAD: the digit variants of
// the last two (GAD = true: the balanced gadget decomposition in registers, ntt_polymul_gadget_pre).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "launch.h"

namespace ntt {
namespace {

template <class CI, class CF>
struct GpuProductExec {
    using W = typename CI::W;
    Ctx<CI> ci;
    Ctx<CF> cf;
    W keep[CI::E];  // the transformed words of operand a while operand b is transformed (unused, and gone, when b is prepared);
                    // the accumulator of an inner product
    W pre[CI::E];   // register prefetch: operand b of this unit -- its round R-1 words, or its prepared round-0 words;
                    // the second accumulator of the two-output inner product
    W *tile, *tab_i, *tab_f;
    __device__ __forceinline__ void init(const PassArgs<CI> &aa, const PassArgs<CF> &af) {
        phase_init<CI>(ci, aa, threadIdx.x, blockIdx.x, blockIdx.y);
        phase_init<CF>(cf, af, threadIdx.x, blockIdx.x, blockIdx.y);
    }
    template <class Fn>
    __device__ __forceinline__ void eachI(Fn &&f) { f(ci); }
    template <class Fn>
    __device__ __forceinline__ void eachF(Fn &&f) { f(cf); }
    template <class Fn>
    __device__ __forceinline__ void eachIF(Fn &&f) { f(ci, cf, keep, pre); }
    __device__ __forceinline__ void sync(std::false_type) { __syncthreads(); }
    __device__ __forceinline__ void sync(std::true_type) {  // wave-local unit: LDS operations of one wave execute in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ uint32_t pg_base() const { return ci.pg_base; }
    __device__ __forceinline__ int ppw() const { return ci.ppw; }
    __device__ __forceinline__ W *lds() { return tile; }
    __device__ __forceinline__ W *tabI() { return tab_i; }
    __device__ __forceinline__ W *tabF() { return tab_f; }
};

#ifndef NTT_PRODUCT_WPE
#define NTT_PRODUCT_WPE 4  // waves per SIMD the register allocator must leave room for (128 VGPRs)
#endif
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_WPE)
void product_kernel(PassArgs<CI> aa, const typename CI::W *in_b, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    PassArgs<CI> ab = aa;
    ab.in = in_b;
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        // one uniform decision per launch, three specialised copies of the pass (see pass_kernel.inc)
        if (aa.field.p < 0x40000000u) run_product_pass<CI, CF, GpuProductExec<CI, CF>, 0>(ex, aa, ab, af);
        else if (aa.field.p < 0x80000000u) run_product_pass<CI, CF, GpuProductExec<CI, CF>, 1>(ex, aa, ab, af);
        else run_product_pass<CI, CF, GpuProductExec<CI, CF>, 2>(ex, aa, ab, af);
    } else {
        run_product_pass<CI, CF>(ex, aa, ab, af);
    }
}

// ... with operand b prepared: bhat = InvU(b), [batch][N] canonical words, or one row of N words when bcast != 0
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_WPE)
void product_pre_kernel(PassArgs<CI> aa, const typename CI::W *bhat, int bcast, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    PassArgs<CI> ab = aa;
    ab.in = bhat;
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        if (aa.field.p < 0x40000000u) run_product_pass<CI, CF, GpuProductExec<CI, CF>, 0, true>(ex, aa, ab, af, bcast != 0);
        else if (aa.field.p < 0x80000000u) run_product_pass<CI, CF, GpuProductExec<CI, CF>, 1, true>(ex, aa, ab, af, bcast != 0);
        else run_product_pass<CI, CF, GpuProductExec<CI, CF>, 2, true>(ex, aa, ab, af, bcast != 0);
    } else {
        run_product_pass<CI, CF, GpuProductExec<CI, CF>, -1, true>(ex, aa, ab, af, bcast != 0);
    }
}

// ... summed over e.dot_terms terms: a is [terms][batch][N], bhat [terms][batch][N] or, when bcast != 0, [terms][N]
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_WPE)
void product_dot_kernel(PassArgs<CI> aa, const typename CI::W *bhat, int bcast, int terms, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        if (aa.field.p < 0x40000000u) run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 0>(ex, aa, bhat, af, bcast != 0, terms);
        else if (aa.field.p < 0x80000000u) run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 1>(ex, aa, bhat, af, bcast != 0, terms);
        else run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 2>(ex, aa, bhat, af, bcast != 0, terms);
    } else {
        run_product_dot_pass<CI, CF>(ex, aa, bhat, af, bcast != 0, terms);
    }
}

// ... for TWO outputs of one operand a: output 1 reads its prepared words b_out_stride words after output 0's and stores o_out_stride
// words after it.  x and two accumulators are live in the term loop, which does not fit 128 VGPRs: a register bound of its own
#ifndef NTT_PRODUCT_MV_WPE
#define NTT_PRODUCT_MV_WPE 3  // waves per SIMD (168 VGPRs): DESIGN.md section 3.2 has the table
#endif
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_MV_WPE)
void product_mv_kernel(PassArgs<CI> aa, const typename CI::W *bhat, int bcast, int terms, size_t b_out_stride, size_t o_out_stride, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        if (aa.field.p < 0x40000000u) run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 0>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride);
        else if (aa.field.p < 0x80000000u) run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 1>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride);
        else run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 2>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride);
    } else {
        run_product_mv_pass<CI, CF>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride);
    }
}

// ... the digit variants (ntt_polymul_gadget_pre): a is [terms / levels][batch][N] canonical words, decomposed in registers; the three
// digit parameters travel as kernel arguments.  Each under the launch bound of the kernel it is a variant of
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_WPE)
void product_dot_gad_kernel(PassArgs<CI> aa, const typename CI::W *bhat, int bcast, int terms, int log_base, int levels, int low_bits, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    const GadgetParams gp{log_base, levels, low_bits};
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        if (aa.field.p < 0x40000000u) run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 0, true>(ex, aa, bhat, af, bcast != 0, terms, gp);
        else if (aa.field.p < 0x80000000u) run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 1, true>(ex, aa, bhat, af, bcast != 0, terms, gp);
        else run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, 2, true>(ex, aa, bhat, af, bcast != 0, terms, gp);
    } else {
        run_product_dot_pass<CI, CF, GpuProductExec<CI, CF>, -1, true>(ex, aa, bhat, af, bcast != 0, terms, gp);
    }
}
template <class CI, class CF>
__global__ __launch_bounds__(CI::NT, NTT_PRODUCT_MV_WPE)
void product_mv_gad_kernel(PassArgs<CI> aa, const typename CI::W *bhat, int bcast, int terms, size_t b_out_stride, size_t o_out_stride, int log_base, int levels,
                           int low_bits, PassArgs<CF> af) {
    __shared__ __attribute__((aligned(16))) typename CI::W tile[CI::LDS_WORDS];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_i[tw_table_words<CI>()];
    __shared__ __attribute__((aligned(16))) typename CI::W tab_f[tw_table_words<CF>()];
    GpuProductExec<CI, CF> ex;
    ex.tile = tile;
    ex.tab_i = tab_i;
    ex.tab_f = tab_f;
    const GadgetParams gp{log_base, levels, low_bits};
    if constexpr (std::is_same<typename CI::F, FieldM32>::value) {
        if (aa.field.p < 0x40000000u) run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 0, true>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride, gp);
        else if (aa.field.p < 0x80000000u) run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 1, true>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride, gp);
        else run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, 2, true>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride, gp);
    } else {
        run_product_mv_pass<CI, CF, GpuProductExec<CI, CF>, -1, true>(ex, aa, bhat, af, bcast != 0, terms, b_out_stride, o_out_stride, gp);
    }
}

template <class PC, bool PRE>
hipError_t launch_product(const ErasedArgs &e, hipStream_t s) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    if ((e.in2_prepared != 0) != PRE || (!PRE && e.in2_broadcast) || e.dot_terms != 0 || !product_no_digits(e)) return hipErrorInvalidValue;  // each kernel family runs its own launches only
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) return hipErrorInvalidValue;  // callers fall back to the separate passes (launch.h: product_mid_fits)
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    if constexpr (PRE)
        hipLaunchKernelGGL((product_pre_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, e.in2_broadcast, af);
    else
        hipLaunchKernelGGL((product_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, af);
    return hipGetLastError();
}

template <class PC>
hipError_t launch_product_dot(const ErasedArgs &e, hipStream_t s) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    if (!product_dot_args_ok(e)) return hipErrorInvalidValue;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) return hipErrorInvalidValue;  // callers fall back to the separate passes (launch.h: product_mid_fits)
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    hipLaunchKernelGGL((product_dot_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, e.in2_broadcast,
                       e.dot_terms, af);  // (the term strides are batch * N and bhat_rows * N words: product_dot_args_ok)
    return hipGetLastError();
}

template <class PC>
hipError_t launch_product_mv(const ErasedArgs &e, hipStream_t s) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    if (!product_mv_args_ok(e)) return hipErrorInvalidValue;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) return hipErrorInvalidValue;  // callers fall back to the separate passes (launch.h: product_mid_fits)
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    hipLaunchKernelGGL((product_mv_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, e.in2_broadcast,
                       e.dot_terms, (size_t) e.mv_in2_stride, (size_t) e.mv_out_stride, af);
    return hipGetLastError();
}

// the digit variants: a summed launch, or -- e.mv_outs == 2, only where the unit has a two-output kernel -- a two-output one
template <class PC>
hipError_t launch_product_gad(const ErasedArgs &e, hipStream_t s) {
    using CI = typename PC::CI;
    using CF = typename PC::CF;
    using F = typename CI::F;
    if (!product_gadget_args_ok(e)) return hipErrorInvalidValue;
    const PassGeom g = product_geometry<PC>(e.n, e.batch, e.target_wgs);
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) return hipErrorInvalidValue;  // callers fall back to the separate passes (launch.h: product_mid_fits)
    PassArgs<CI> aa;
    PassArgs<CF> af;
    fill_product_args<PC>(e, g, aa, af);
    if (e.mv_outs != 0) {
        if constexpr (product_mv_unit<F>(CI::LOG_M))
            hipLaunchKernelGGL((product_mv_gad_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, e.in2_broadcast,
                               e.dot_terms, (size_t) e.mv_in2_stride, (size_t) e.mv_out_stride, e.gad_log_base, e.gad_levels, e.gad_low_bits, af);
        else
            return hipErrorInvalidValue;
    } else {
        hipLaunchKernelGGL((product_dot_gad_kernel<CI, CF>), dim3(g.grid_x, g.grid_y, 1), dim3(CI::NT, 1, 1), 0, s, aa, (const typename CI::W *) e.in2, e.in2_broadcast,
                           e.dot_terms, e.gad_log_base, e.gad_levels, e.gad_low_bits, af);
    }
    return hipGetLastError();
}

}  // namespace

// every unit size with a kernel (launch.h: product_dispatch); instantiated for this unit's field only, as launch_pass_of is (kernels.h)
#if defined(NTT_PRODUCT_GAD)
template <class F>
hipError_t launch_product_gad_mid_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    product_gadget_dispatch<F>(log_m, [&](auto tag) { err = launch_product_gad<typename decltype(tag)::Cfg>(a, s); });
    return err;
}
template hipError_t launch_product_gad_mid_of<NTT_FIELD>(int, const ErasedArgs &, hipStream_t);
#elif defined(NTT_PRODUCT_MV)
template <class F>
hipError_t launch_product_mv_mid_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    product_mv_dispatch<F>(log_m, [&](auto tag) { err = launch_product_mv<typename decltype(tag)::Cfg>(a, s); });
    return err;
}
template hipError_t launch_product_mv_mid_of<NTT_FIELD>(int, const ErasedArgs &, hipStream_t);
#elif defined(NTT_PRODUCT_DOT)
template <class F>
hipError_t launch_product_dot_mid_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    product_dot_dispatch<F>(log_m, [&](auto tag) { err = launch_product_dot<typename decltype(tag)::Cfg>(a, s); });
    return err;
}
template hipError_t launch_product_dot_mid_of<NTT_FIELD>(int, const ErasedArgs &, hipStream_t);
#elif defined(NTT_PRODUCT_PRE)
template <class F>
hipError_t launch_product_pre_mid_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    product_dispatch<F>(log_m, [&](auto tag) { err = launch_product<typename decltype(tag)::Cfg, true>(a, s); });
    return err;
}
template hipError_t launch_product_pre_mid_of<NTT_FIELD>(int, const ErasedArgs &, hipStream_t);
#else
template <class F>
hipError_t launch_product_mid_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    product_dispatch<F>(log_m, [&](auto tag) { err = launch_product<typename decltype(tag)::Cfg, false>(a, s); });
    return err;
}
template hipError_t launch_product_mid_of<NTT_FIELD>(int, const ErasedArgs &, hipStream_t);
#endif

}  // namespace ntt
