// Which instantiation of k_rt_flux and k_rt_coef a batch runs, written once for both widths of the coefficient planes.  CT is the
// plane element type: double in rt_fused.hip, float in rt_fused_f32.hip (`precision = single`).  Each translation unit
// instantiates the rows of its own width only, so the two sets of kernels compile side by side.
#pragma once
#include <type_traits>

#include "rt_kernels.h"

namespace hx {

template <class CT> constexpr bool planes_fp32 = std::is_same_v<CT, float>;

// fp64 planes: every tiling choose_geometry selects.  fp32 planes: those of coef_fp32_tiling -- up to 14 rows, 14 rows on 16
// lanes with the compile-time scans only, and the sweeps only (the matrix method keeps fp64 planes).
template <class CT> constexpr bool plane_rows(int rows) { return !planes_fp32<CT> || rows <= 14; }

// fn(std::integral_constant<int, ROWS>) for the batch's rows (a row count without a case of its own runs as the widest tiling)
template <class CT, class F>
auto for_rows(int rows, F&& fn) {
    switch (rows) {
#define HX_ROWS(n) \
    case n:        \
        if constexpr (plane_rows<CT>(n)) return fn(std::integral_constant<int, n>{}); else break;
        HX_ROWS(1) HX_ROWS(2) HX_ROWS(3) HX_ROWS(4) HX_ROWS(5) HX_ROWS(6) HX_ROWS(7) HX_ROWS(8) HX_ROWS(9) HX_ROWS(10)
        HX_ROWS(11) HX_ROWS(12) HX_ROWS(13) HX_ROWS(14) HX_ROWS(15) HX_ROWS(20) HX_ROWS(24) HX_ROWS(28) HX_ROWS(32)
#undef HX_ROWS
    }
    return fn(std::integral_constant<int, planes_fp32<CT> ? 14 : 16>{});
}

inline size_t flux_shmem_bytes(const hx_rt* rt) {
    const TileGeom& g = rt->g;
    return ((size_t)g.nxb * (rt->H + 3) + (size_t)g.nxb * 2 * rt->I + (size_t)g.ypb * g.nxb * 2 * rt->I) *
           sizeof(double);
}

// The k_rt_flux instantiation this batch runs: launched with `f`, or -- f == nullptr -- its dynamic-LDS limit raised to the
// batch's demand
template <class CT, int ROWS, int K, bool MATRIX>
hipError_t flux_kernel(hx_rt* rt, const FluxArgs* f) {
    const size_t shmem = flux_shmem_bytes(rt);
    const dim3 grid(rt->g.nblk_x, rt->C), block(rt->g.threads);
    if constexpr (planes_fp32<CT>) {
        if (!f) return hipFuncSetAttribute((const void*)k_rt_flux_f32<ROWS, K, MATRIX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_flux_f32<ROWS, K, MATRIX>), grid, block, shmem, rt->ctx->stream, *f, (const float*)rt->coef32);
    } else {
        if (!f) return hipFuncSetAttribute((const void*)k_rt_flux<ROWS, K, MATRIX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_flux<ROWS, K, MATRIX>), grid, block, shmem, rt->ctx->stream, *f);
    }
    return hipSuccess;
}

template <class CT, int ROWS, bool MATRIX>
hipError_t flux_method(hx_rt* rt, const FluxArgs* f) {
    if constexpr (ROWS > 16) return flux_kernel<CT, ROWS, 64, MATRIX>(rt, f);   // (only on 64 lanes: choose_geometry)
    else if constexpr (planes_fp32<CT> && ROWS == 14) return flux_kernel<CT, 14, 16, MATRIX>(rt, f);   // (coef_fp32_tiling)
    else {
        const int k = rt->generic_scans ? 0 : rt->g.k;
        if (k == 16) return flux_kernel<CT, ROWS, 16, MATRIX>(rt, f);
        if (k == 32) return flux_kernel<CT, ROWS, 32, MATRIX>(rt, f);
        if (k == 64) return flux_kernel<CT, ROWS, 64, MATRIX>(rt, f);
        return flux_kernel<CT, ROWS, 0, MATRIX>(rt, f);
    }
}

template <class CT>
hipError_t select_flux(hx_rt* rt, const FluxArgs* f) {
    return for_rows<CT>(rt->g.ROWS, [&](auto rows) {
        constexpr int ROWS = decltype(rows)::value;
        if constexpr (!planes_fp32<CT>)
            if (rt->matrix) return flux_method<CT, ROWS, true>(rt, f);
        return flux_method<CT, ROWS, false>(rt, f);
    });
}

// LDS demand of k_rt_coef with `tpb` tiles per workgroup, without the optional cloud image; coef_nbx: the bins it stages
inline int coef_nbx(const hx_rt* rt, int tpb) { return rt->g.nxb * ((tpb - 1) / (rt->g.NW * rt->g.nparts) + 2); }
inline size_t coef_shmem_bytes(const hx_rt* rt, int tpb) {
    const int TS = tpb * rt->g.S;
    return ((size_t)(rt->L + rt->I) * TS + (size_t)rt->H * (coef_nbx(rt, tpb) + 2)) * sizeof(double) + 2 * TS * sizeof(int);
}

// Does this refresh run k_rt_coef_plain?  Exactly the flags that kernel holds at compile time (CoefPlainFlags, rt_kernels.h),
// on fp64 planes, unless HELIOS_RT_COEF_GENERAL=1 keeps the general kernel (A/B and tests: same bits)
inline bool coef_runs_plain(const hx_rt* rt, const KArgs& a) {
    return !rt->coef32 && !rt->coef_general && a.matrix == 0 && a.iso == 0 && a.dir_beam != 1 && a.clouds != 1 && a.cloud_lds == 0 &&
           a.scat_corr != 1 && a.has_vp == 0 && a.g_0 == 0.0;
}

template <int ROWS, int TPB, bool FROM_TABLE>
void coef_plain_kernel(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem) {
    if (shmem > 64 * 1024 && !rt->coef_plain_shmem_raised[FROM_TABLE]) {
        (void)hipFuncSetAttribute((const void*)k_rt_coef_plain<ROWS, TPB, FROM_TABLE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        rt->coef_plain_shmem_raised[FROM_TABLE] = true;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_coef_plain<ROWS, TPB, FROM_TABLE>), grid, dim3(64 * TPB), shmem, rt->ctx->stream, a);
}

template <class CT, int ROWS, int TPB>
void coef_kernel(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem) {
    if constexpr (!planes_fp32<CT>)
        if (coef_runs_plain(rt, a)) {
            if (a.from_table) coef_plain_kernel<ROWS, TPB, true>(rt, a, grid, shmem);
            else coef_plain_kernel<ROWS, TPB, false>(rt, a, grid, shmem);
            return;
        }
    const void* kernel;
    if constexpr (planes_fp32<CT>) kernel = (const void*)k_rt_coef_f32<ROWS, TPB>;
    else kernel = (const void*)k_rt_coef<ROWS, TPB>;
    if (shmem > 64 * 1024 && !rt->coef_shmem_raised) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        rt->coef_shmem_raised = true;
    }
    if constexpr (planes_fp32<CT>)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_coef_f32<ROWS, TPB>), grid, dim3(64 * TPB), shmem, rt->ctx->stream, a, rt->coef32);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_coef<ROWS, TPB>), grid, dim3(64 * TPB), shmem, rt->ctx->stream, a);
}

// k_rt_coef with rt->coef_tpb tiles per workgroup: kernels of 1, 2, 4 and 8 tiles, any other value runs as 4
template <class CT>
void select_coef(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem) {
    for_rows<CT>(rt->g.ROWS, [&](auto rows) {
        constexpr int ROWS = decltype(rows)::value;
        switch (rt->coef_tpb) {
            case 1: coef_kernel<CT, ROWS, 1>(rt, a, grid, shmem); break;
            case 2: coef_kernel<CT, ROWS, 2>(rt, a, grid, shmem); break;
            case 8:
                if constexpr (ROWS <= 16) { coef_kernel<CT, ROWS, 8>(rt, a, grid, shmem); break; }   // (big columns: at most four tiles fit the LDS)
                [[fallthrough]];
            default: coef_kernel<CT, ROWS, 4>(rt, a, grid, shmem); break;
        }
    });
}

// ---- fp32 coefficient planes (`precision = single`, hx_rt_flags.coef_fp32): rt_fused_f32.hip -----------------------------
// The tilings with an fp32 instantiation: every tiling choose_geometry selects without scratch (columns of up to 416
// layers, isothermal ones up to 512).  Other tilings run on fp64 planes.
bool coef_fp32_tiling(int rows, int k, bool generic_scans);
// select_flux / select_coef on rt->coef32 (the batch was given fp32 planes only where coef_fp32_tiling holds: rt_create_into)
hipError_t select_flux_f32(hx_rt* rt, const FluxArgs* f);
void select_coef_f32(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem);

}  // namespace hx
