// pass_kernel.inc -- the __global__ wrapper around run_pass() and the launcher that instantiates it for every
// configuration launch.h selects for one (field, direction).  Included by the six kernels_<field>_<dir>.hip
// translation units, which define
//   NTT_FIELD      ntt::FieldGL | ntt::FieldM32 | ntt::FieldM64
//   NTT_INV        true | false
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "launch.h"

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
// (the fused expansion on columns keeps the occupancy bracket of the plain matrix pass it stands in for: 4 waves of 8-byte words, 6 of
// 4-byte words -- left alone, the 8-stage kernel of general 8-byte words takes 129 VGPRs and the 6-stage one of 4-byte words 81.  The
// 8-stage kernel of 4-byte words is the exception: it needs 87, held to 80 it spills 20 bytes, so it runs at 5 waves and no scratch)
template <class Cfg, bool SC = false>
__global__ __launch_bounds__(Cfg::NT, (Cfg::MLDE && !(sizeof(typename Cfg::W) == 4 && Cfg::LOG_M == 8)) ? (sizeof(typename Cfg::W) == 8 ? 4 : 6)
                                 : (Cfg::LOG_E < 4 && Cfg::LOG_M >= 7) ? NTT_E8_WPE
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

template <class Cfg>
hipError_t launch_cfg(const ErasedArgs &e, hipStream_t s) {
    using W = typename Cfg::W;
    // the fused expansion runs in its own kernels and nowhere else (never beside LDS-DMA or the register prefetch: PassCfg::LDE);
    // refused here before anything else, and again by the fill below, which the host index model shares
    if ((e.lde_beta != 0) != Cfg::LDE) return hipErrorInvalidValue;
    if ((e.cinv_u != nullptr) != Cfg::CINV) return hipErrorInvalidValue;  // ... likewise the coset interpolation's vector (PassCfg::CINV)
    if ((e.mat_w != 0 || e.mat_pitch != 0 || e.mat_width != 0) != Cfg::MAT) return hipErrorInvalidValue;  // ... and the matrix addressing (PassCfg::MAT)
    if ((e.mat_lde_beta != 0) != Cfg::MLDE || (e.mat_cinv_u != nullptr) != Cfg::MCINV) return hipErrorInvalidValue;  // ... and its coset twins' operands (PassCfg::MLDE / MCINV)
    PassGeom g = pass_geometry_of<Cfg>(e);
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
    PassArgs<Cfg> a;
    if (!fill_pass_args<Cfg>(e, g, a)) return hipErrorInvalidValue;  // launch.h: LDE argument ranges, do_scale without tw_sc, ...
    if (g.grid_y == 0) return hipSuccess;
    if (g.grid_y > 65535u) {
        // more polynomial groups than blockIdx.y can number (tiny N, batch beyond ~10^9): polynomials are
        // independent, so run the batch in slices; a slice is a multiple of 2^log_up polynomials and of 16 bytes
        const uint64_t slice = ((uint64_t) 65535u * (uint32_t) g.ppw) << g.log_up;
        for (uint64_t done = 0; done < e.batch; done += slice) {
            ErasedArgs sub = e;
            // (matrices: a slice of `done` matrices of N * pitch words each; the compact LDE source below does not exist there)
            const size_t off = (size_t) ((Cfg::MAT ? done * mat_words(e) : done << e.n) * sizeof(W));
            sub.in = (const char *) e.in + off;
            sub.out = (char *) e.out + off;
            if (e.in2) sub.in2 = (const char *) e.in2 + off;
            if constexpr (Cfg::MLDE) sub.mat_lde_in = (const char *) e.mat_lde_in + (size_t) (done * mat_src_words(e) * sizeof(W));
            if (e.lde_beta) sub.lde_in = (const char *) e.lde_in + (off >> e.lde_beta);
            sub.batch = (uint32_t) (e.batch - done < slice ? e.batch - done : slice);
            const hipError_t err = launch_cfg<Cfg>(sub, s);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    if constexpr (fold_scale<Cfg>() && !Cfg::CINV) {  // (a coset interpolation is never a scaled launch: fill_pass_args)
        if (a.tw_sc != nullptr) {  // scaled inverse: N^-1 rides on stage 0 (no scaling sweep)
            hipLaunchKernelGGL((pass_kernel<Cfg, true>), dim3(g.grid_x, g.grid_y, 1), dim3(Cfg::NT, 1, 1), 0, s, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((pass_kernel<Cfg, false>), dim3(g.grid_x, g.grid_y, 1), dim3(Cfg::NT, 1, 1), 0, s, a);
    return hipGetLastError();
}

}  // namespace

// the kernel launch.h's pass_dispatch selects for this pass.  (This definition names launch_cfg of THIS unit's anonymous namespace:
// it is explicitly instantiated below for the unit's one (field, direction) and for nothing else -- see kernels.h)
template <class F, bool INV>
hipError_t launch_pass_of(bool contig, int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    if (!pass_dispatch<F, INV>(contig, log_m, a, [&](auto tag) { err = launch_cfg<typename decltype(tag)::Cfg>(a, s); })) return hipErrorInvalidValue;
    return err;
}
template hipError_t launch_pass_of<NTT_FIELD, NTT_INV>(bool, int, const ErasedArgs &, hipStream_t);

// ... and the matrix twin of the column pass that launch.h's mat_twin_dispatch selects (ntt_forward_columns / ntt_inverse_columns: the
// plain twin mat_dispatch names; ntt_lde_columns / ntt_coset_inverse_columns: the coset twin of the pass that holds stage 0)
template <class F, bool INV>
hipError_t launch_mat_of(int log_m, const ErasedArgs &a, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    if (!mat_twin_dispatch<F, INV>(log_m, a, [&](auto tag) { err = launch_cfg<typename decltype(tag)::Cfg>(a, s); })) return hipErrorInvalidValue;
    return err;
}
template hipError_t launch_mat_of<NTT_FIELD, NTT_INV>(int, const ErasedArgs &, hipStream_t);

}  // namespace ntt
