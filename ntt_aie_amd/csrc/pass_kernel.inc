// pass_kernel.inc -- the __global__ wrapper around run_pass() and the switch that
// instantiates it for one (field, direction).  Included by the four
// kernels_<field>_<dir>.hip translation units, which define
//   NTT_FIELD      ntt::FieldGL | ntt::FieldM32
//   NTT_INV        true | false
//   NTT_LAUNCH_FN  launch_gl_fwd | ...
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pass.h"

namespace ntt {
namespace {

#if defined(NTT_PHASE_STAMPS)
__device__ unsigned long long stamp_dummy[STAMP_RECORD];  // where stamps go when no buffer is set: the store count per wave must not change
#endif

template <class Cfg>
struct GpuExec {
    static constexpr bool early_ok = true;  // run_pass may request the first tile before the resident twiddles
    Ctx<Cfg> ctx;
    typename Cfg::W *tile;
    __device__ __forceinline__ void init(const PassArgs<Cfg> &a) {
#if defined(NTT_PHASE_STAMPS)
        stamp_init(a);
#endif
        phase_init<Cfg>(ctx, a, threadIdx.x, blockIdx.x, blockIdx.y);
    }
    __device__ __forceinline__ void init_indices(const PassArgs<Cfg> &a) {
#if defined(NTT_PHASE_STAMPS)
        stamp_init(a);
#endif
        phase_init<Cfg, false>(ctx, a, threadIdx.x, blockIdx.x, blockIdx.y);
    }
    template <class Fn>
    __device__ __forceinline__ void each(Fn &&f) {
        f(ctx);
    }
    __device__ __forceinline__ void sync(std::false_type) { __syncthreads(); }
    // wave-local exchange: LDS ops of one wave are executed in order by the hardware; only the
    // compiler has to be kept from moving the reads above the writes
    __device__ __forceinline__ void sync(std::true_type) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ uint32_t pg_base() const { return ctx.pg_base; }
    __device__ __forceinline__ int ppw() const { return ctx.ppw; }
    __device__ __forceinline__ bool iter_begin(int) { return true; }
    __device__ __forceinline__ void iter_done(int) {}
    __device__ __forceinline__ typename Cfg::W *lds() { return tile; }
#if defined(NTT_PHASE_STAMPS)
    // Diagnostic build only.  Lane 0 of EVERY wave writes s_memtime to slot STAMP_HEADER + k of the wave's own record.  The
    // stamp first waits for the wave's outstanding LDS / scalar traffic (and, where the kernel loads straight into registers,
    // for its global loads) so that a phase ends when its data is there, not when its instructions were issued; LDS-DMA
    // kernels must NOT wait on vmcnt here (the next tile's prefetch is in flight by design), their tile has its own stamp.
    unsigned long long *sp;
    __device__ __forceinline__ void stamp_init(const PassArgs<Cfg> &a) {
        const uint32_t rec = ((blockIdx.y * gridDim.x + blockIdx.x) * (Cfg::NT / 64)) + (threadIdx.x >> 6);
        sp = (a.stamps != nullptr && rec < a.stamp_records) ? a.stamps + (size_t) rec * STAMP_RECORD : stamp_dummy;
        if ((threadIdx.x & 63u) == 0) {
            sp[0] = __builtin_amdgcn_s_memrealtime();
            sp[1] = __builtin_amdgcn_s_memtime();
            uint32_t hw_id, xcc_id;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
            sp[2] = (unsigned long long) hw_id | ((unsigned long long) (xcc_id & 15u) << 32);
        }
    }
    __device__ __forceinline__ void stamp(int k) {
        if constexpr (Cfg::DMA) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        // k < (STAMP_ITERS + 1) * STAMPS_PER_ITER by construction: run_pass() numbers the stamps of every iteration from STAMP_ITERS on
        // into ONE overflow block behind the eight recorded ones (pass.h: stamp_base), so the store never leaves the wave's record
        if ((threadIdx.x & 63u) == 0) __builtin_nontemporal_store(t, sp + STAMP_HEADER + k);
    }
    __device__ __forceinline__ void pass_done(int completed) {
        if ((threadIdx.x & 63u) == 0) {
            sp[3] = (unsigned long long) completed;
            sp[STAMP_RECORD - 2] = __builtin_amdgcn_s_memtime();
            sp[STAMP_RECORD - 1] = __builtin_amdgcn_s_memrealtime();
        }
    }
#else
    __device__ __forceinline__ void pass_done(int) {}
#endif
};

#ifndef NTT_E8_WPE
#define NTT_E8_WPE 4
#endif
// second argument = minimum waves per SIMD the register allocator must leave room for
#ifndef NTT_R3_WPE
#define NTT_R3_WPE 1
#endif
#ifndef NTT_COL9_WPE
#define NTT_COL9_WPE 4  // 9-stage column pass of 8-byte words: 512 threads, 68 KiB of LDS -> two workgroups per CU need <= 128 VGPRs
#endif
// SC: the scaled-inverse specialisation with N^-1 folded into stage 0 (pass.h: fold_scale) -- a kernel of its own, so that
// its heavier last stage does not touch the register allocation of the unscaled one
template <class Cfg, bool SC = false>
__global__ __launch_bounds__(Cfg::NT, (Cfg::LOG_E < 4 && Cfg::LOG_M >= 7) ? NTT_E8_WPE
                                 : (Cfg::CONTIG && Cfg::R == 3 && sizeof(typename Cfg::W) == 8) ? NTT_R3_WPE
                                 : (!Cfg::CONTIG && Cfg::LOG_M == 9 && sizeof(typename Cfg::W) == 8) ? NTT_COL9_WPE : 1)
void pass_kernel(PassArgs<Cfg> a) {
    constexpr bool ANY_LDS = Cfg::R > 1 || !Cfg::DIRECT_LOAD || !Cfg::DIRECT_STORE;
    __shared__ __attribute__((aligned(16))) typename Cfg::W tile[Cfg::DMA ? 2 * Cfg::TILE_WORDS : (ANY_LDS ? Cfg::LDS_WORDS : 4)];
#if defined(NTT_EXPERIMENT)
    if (a.skip_if != nullptr && __builtin_nontemporal_load(a.skip_if) != 0) return;  // guarded fallback launch (tools-side fused experiment)
#endif
    GpuExec<Cfg> ex;
    ex.tile = tile;
    if constexpr (std::is_same<typename Cfg::F, FieldM32>::value && Cfg::E >= 8) {
        // one uniform decision per launch, three specialised copies of the pass
        static_assert(!SC, "folded scaling is a Goldilocks specialisation");
        if (a.field.p < 0x40000000u) run_pass<Cfg, GpuExec<Cfg>, 0>(ex, a);
        else if (a.field.p < 0x80000000u) run_pass<Cfg, GpuExec<Cfg>, 1>(ex, a);
        else run_pass<Cfg, GpuExec<Cfg>, 2>(ex, a);
    } else {
        run_pass<Cfg, GpuExec<Cfg>, -1, SC>(ex, a);
    }
}

template <class F>
F make_field(const ErasedArgs &e);
template <>
FieldGL make_field<FieldGL>(const ErasedArgs &) {
    return FieldGL{};
}
template <>
FieldM32 make_field<FieldM32>(const ErasedArgs &e) {
    return FieldM32{e.p, e.pinv, e.r2};
}
template <>
FieldM64 make_field<FieldM64>(const ErasedArgs &e) {
    return FieldM64{e.p64, e.pinv64, e.r2_64};
}

template <class Cfg>
hipError_t launch_cfg(const ErasedArgs &e, hipStream_t s) {
    using W = typename Cfg::W;
    PassArgs<Cfg> a;
    a.in = (const W *) e.in;
    a.out = (W *) e.out;
    a.tw = (const W *) e.tw;
    a.tw_sc = nullptr;
    a.field = make_field<typename Cfg::F>(e);
    a.n = e.n;
    a.s0 = e.s0;
    a.batch = e.batch;
    a.layout = e.layout;
    a.do_scale = e.do_scale;
    a.scale = (W) e.scale;
    a.dbg = e.dbg;
    a.pg_stride = 1;
    a.in2 = (const W *) e.in2;
    a.pw_scale = (W) e.pw_scale;
    a.skip_if = (const uint32_t *) e.skip_if;
    // the fused expansion runs in its own kernels and nowhere else (never beside LDS-DMA or the register prefetch: PassCfg::LDE)
    if ((e.lde_beta != 0) != Cfg::LDE) return hipErrorInvalidValue;
    if constexpr (Cfg::LDE) {
        if (e.lde_beta < 1 || e.lde_beta > 4 || e.lde_beta >= e.n || e.s0 != 0 || !e.lde_in || !e.lde_s || e.in2) return hipErrorInvalidValue;
        a.lde_in = (const W *) e.lde_in;
        a.lde_s = (const W *) e.lde_s;
        a.lde_beta = e.lde_beta;
    }
#if defined(NTT_PHASE_STAMPS)
    a.stamps = (unsigned long long *) e.stamps;
    a.stamp_records = e.stamp_records;
#endif
    PassGeom g = pass_geometry(e.n, e.s0, Cfg::LOG_M, Cfg::LOG_C, Cfg::LOG_U, Cfg::CONTIG, e.batch,
                               e.target_wgs, Cfg::PPW_CAP);
#if defined(NTT_EXPERIMENT)
    if ((e.dbg & 0x1000) && g.grid_x == 1 && g.ppw == 1) {
        // EXPERIMENT (round 6, config 2): ONE generation of `cap` = dbg >> 16 workgroups for cap < groups <= 2 cap: the first
        // (groups - cap) rows stream two polynomial groups each (the second one prefetched, PassCfg::PREFETCH), the rest one
        const uint32_t cap = (uint32_t) e.dbg >> 16, groups = g.grid_y;
        if (cap > 0 && groups > cap && groups <= 2 * cap) {
            g.ppw = 2;
            g.tp = Taper{{groups - cap, 2 * cap - groups, 0, 0}};
            g.grid_y = cap;
        }
    }
#endif
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) {
        // more polynomial groups than blockIdx.y can number (tiny N, batch beyond ~10^9): polynomials are
        // independent, so run the batch in slices; a slice is a multiple of 2^log_up polynomials and of 16 bytes
        const uint64_t slice = ((uint64_t) 65535u * (uint32_t) g.ppw) << g.log_up;
        for (uint64_t done = 0; done < e.batch; done += slice) {
            ErasedArgs sub = e;
            const size_t off = (size_t) ((done << e.n) * sizeof(W));
            sub.in = (const char *) e.in + off;
            sub.out = (char *) e.out + off;
            if (e.in2) sub.in2 = (const char *) e.in2 + off;
            if (e.lde_beta) sub.lde_in = (const char *) e.lde_in + (off >> e.lde_beta);
            sub.batch = (uint32_t) (e.batch - done < slice ? e.batch - done : slice);
            const hipError_t err = launch_cfg<Cfg>(sub, s);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    a.ppw = g.ppw;
    a.tp = g.tp;
    a.log_ul = g.log_ul;
    a.log_uh = g.log_uh;
    a.log_up = g.log_up;
    if constexpr (fold_scale<Cfg>()) {
        if (e.do_scale && e.tw_sc == nullptr) return hipErrorInvalidValue;  // these kernels have no scaling sweep
        if (e.do_scale) {  // scaled inverse: N^-1 rides on stage 0 (no scaling sweep)
            a.tw_sc = (const W *) e.tw_sc;
            hipLaunchKernelGGL((pass_kernel<Cfg, true>), dim3(g.grid_x, g.grid_y, 1), dim3(Cfg::NT, 1, 1), 0, s, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((pass_kernel<Cfg, false>), dim3(g.grid_x, g.grid_y, 1), dim3(Cfg::NT, 1, 1), 0, s, a);
    return hipGetLastError();
}

template <int LOG_M>
using ContigCfg = PassCfg<NTT_FIELD, LOG_M, 0, true, NTT_INV, contig_preload_mask(LOG_M, sizeof(typename NTT_FIELD::W))>;
// 13 stages on an 8192-word tile: 512 threads x 16 words, rounds of 4 + 4 + 4 + 1 stages.  4-byte words keep every round's
// twiddles in registers (99 VGPRs); 8-byte words only the last round's single, wave-uniform one (the others are re-read
// from L2 at the start of their round, as in the 12-stage radix-16 pass: 128 VGPRs, two workgroups per CU)
using ContigCfg13 = PassCfg<NTT_FIELD, 13, 0, true, NTT_INV, sizeof(typename NTT_FIELD::W) == 4 ? 0xF : 0x8, 4, 9>;
// 14 stages on a 16384-word tile of 4-byte words (64 KiB): ONE 1024-thread workgroup per CU, rounds of 4 + 4 + 4 + 2 stages, every
// round's twiddles resident.  Pays only for the lazy butterflies (p < 2^30: N = 2^14 in one pass -21 % forward, -5 % inverse at
// saturating batches; +3 % for a 32-bit prime, +20 % for one polynomial: profiles/r02_ab_13_stage_pass.txt), so the planner offers it
// as a launch-time alternative for that modulus class above a batch threshold (plan.h: plan_alternatives)
using ContigCfg14 = PassCfg<NTT_FIELD, 14, 0, true, NTT_INV, 0xF, 4, 10>;
template <int LOG_M>
using ContigCfgE8 = PassCfg<NTT_FIELD, LOG_M, 0, true, NTT_INV, 0xF, 3>;
template <int LOG_M>
using ContigCfgE8W = PassCfg<NTT_FIELD, LOG_M, 0, true, NTT_INV, 0xF, 3, 9>;  // 512 threads
// forward pass with a fused pointwise product (a.in2): same kernels, tile staged by ordinary loads
template <int LOG_M>
using ContigCfgE8P = PassCfg<NTT_FIELD, LOG_M, 0, true, NTT_INV, 0xF, 3, 8, false>;
template <int LOG_M>
using ContigCfgE8WP = PassCfg<NTT_FIELD, LOG_M, 0, true, NTT_INV, 0xF, 3, 9, false>;
template <int LOG_M>
using ColCfg = ColPassCfg<NTT_FIELD, LOG_M, NTT_INV>;

}  // namespace

hipError_t NTT_LAUNCH_FN(bool contig, int log_m, const ErasedArgs &a, hipStream_t s) {
    if (a.lde_beta != 0) {  // first pass of ntt_lde: the fused-expansion twin of this shape (pass.h: lde_dispatch)
        if constexpr (NTT_INV) {
            return hipErrorInvalidValue;
        } else {
            hipError_t err = hipErrorInvalidValue;
            if (!contig || !lde_dispatch<NTT_FIELD>(log_m, a.s0 + log_m == a.n, [&](auto tag) { err = launch_cfg<typename decltype(tag)::Cfg>(a, s); }))
                return hipErrorInvalidValue;
            return err;
        }
    }
    if (contig) {
        if (log_m == 13) return launch_cfg<ContigCfg13>(a, s);
        if (log_m == 14) {
            if constexpr (sizeof(typename NTT_FIELD::W) == 4) return launch_cfg<ContigCfg14>(a, s);
            else return hipErrorInvalidValue;
        }
        // PassDesc::variant 1: a single-pass unit of 2^10 .. 2^12 words on 512 threads x 8 words (radix-8 rounds; 8-byte forward: the
        // LDS-DMA kernel that otherwise runs as the first pass of a two-pass plan) instead of 256 x 16 -- twice the waves for the same
        // work, for launches too small to fill the SIMDs (plan.h: plan_alternatives).  Both layouts (pass.h: elem_off / lane_eff);
        // a fused pointwise operand keeps the default kernel.
        if (a.variant == 1 && a.in2 == nullptr) {
            if (log_m == 10) return launch_cfg<ContigCfgE8W<10>>(a, s);
            if (log_m == 11) return launch_cfg<ContigCfgE8W<11>>(a, s);
            if (log_m == 12) return launch_cfg<ContigCfgE8W<12>>(a, s);
        }
        if (contig_log_e(log_m, sizeof(typename NTT_FIELD::W), a.s0 + log_m == a.n) == 3) {
            if constexpr (sizeof(typename NTT_FIELD::W) == 8 && !NTT_INV) {
                if (a.in2 != nullptr) {
                    if (log_m == 7) return launch_cfg<ContigCfgE8P<7>>(a, s);
                    if (log_m == 8) return launch_cfg<ContigCfgE8P<8>>(a, s);
                    if (log_m == 9) return launch_cfg<ContigCfgE8P<9>>(a, s);
                    if (log_m == 10) return launch_cfg<ContigCfgE8WP<10>>(a, s);
                    if (log_m == 11) return launch_cfg<ContigCfgE8WP<11>>(a, s);
                    return launch_cfg<ContigCfgE8WP<12>>(a, s);
                }
            }
            if constexpr (sizeof(typename NTT_FIELD::W) == 8) {
                if (log_m == 7) return launch_cfg<ContigCfgE8<7>>(a, s);
                if (log_m == 8) return launch_cfg<ContigCfgE8<8>>(a, s);
                if (log_m == 9) return launch_cfg<ContigCfgE8<9>>(a, s);
                if (log_m == 10) return launch_cfg<ContigCfgE8W<10>>(a, s);
                if (log_m == 11) return launch_cfg<ContigCfgE8W<11>>(a, s);
                return launch_cfg<ContigCfgE8W<12>>(a, s);
            }
        }
        switch (log_m) {
            case 1: return launch_cfg<ContigCfg<1>>(a, s);
            case 2: return launch_cfg<ContigCfg<2>>(a, s);
            case 3: return launch_cfg<ContigCfg<3>>(a, s);
            case 4: return launch_cfg<ContigCfg<4>>(a, s);
            case 5: return launch_cfg<ContigCfg<5>>(a, s);
            case 6: return launch_cfg<ContigCfg<6>>(a, s);
            case 7: return launch_cfg<ContigCfg<7>>(a, s);
            case 8: return launch_cfg<ContigCfg<8>>(a, s);
            case 9: return launch_cfg<ContigCfg<9>>(a, s);
            case 10: return launch_cfg<ContigCfg<10>>(a, s);
            case 11: return launch_cfg<ContigCfg<11>>(a, s);
            case 12: return launch_cfg<ContigCfg<12>>(a, s);
            default: return hipErrorInvalidValue;
        }
    }
    switch (log_m) {
        case 4: return launch_cfg<ColCfg<4>>(a, s);
        case 5: return launch_cfg<ColCfg<5>>(a, s);
        case 6: return launch_cfg<ColCfg<6>>(a, s);
        case 7: return launch_cfg<ColCfg<7>>(a, s);
        case 8: return launch_cfg<ColCfg<8>>(a, s);
        case 9: return launch_cfg<ColCfg<9>>(a, s);  // 512 rows x one 128-byte segment: N = 2^22 = 13 + 9 in two passes
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ntt
