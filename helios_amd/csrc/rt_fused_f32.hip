// `precision = single`: the coefficient kernel and the flux kernel on fp32 coefficient planes (hx_rt_flags.coef_fp32).
// Same source as the fp64 kernels of rt_fused.hip (rt_coef_kernel.inc, rt_flux_kernel.inc, plane element type CT = float):
// the planes -- coded without cancellation, plane_code.h -- are rounded to fp32 once, where k_rt_coef_f32 stores
// them, and widened to fp64 where k_rt_flux_f32 loads them; all arithmetic, the up-flux state and everything else stay
// fp64.  A translation unit of its own, so that the build compiles these instantiations next to rt_fused.hip's instead of
// after them.
#define HX_PLANE_KERNELS_ONLY
#include "rt_kernels.h"

using namespace hx;

namespace hx {

// Columns of up to 416 layers (832 half-layers) get at most 13 rows on 64 lanes; the one 14-row tiling choose_geometry picks
// without scratch is k = 16 with the compile-time scans.  The fp64 kernels of 14 rows on other lane counts and of 15 rows and
// more keep part of their register image in scratch (rt_fused.hip, flux_variant_spills): those tilings have no fp32 variant.
bool coef_fp32_tiling(int rows, int k, bool generic_scans) {
    return rows <= 13 || (rows == 14 && k == 16 && !generic_scans);
}

namespace {

template <int ROWS, int TPB>
void coef_tpb(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem) {
    if (shmem > 64 * 1024 && !rt->coef_shmem_raised) {
        (void)hipFuncSetAttribute((const void*)k_rt_coef_f32<ROWS, TPB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)shmem);
        rt->coef_shmem_raised = true;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_coef_f32<ROWS, TPB>), grid, dim3(64 * TPB), shmem, rt->ctx->stream, a,
                       rt->coef32);
}

template <int ROWS>
void coef_rows(hx_rt* rt, const KArgs& a, int tpb, dim3 grid, size_t shmem) {
    switch (tpb) {   // (launch_coef's choice: 1, 2, 4 or 8)
        case 1: coef_tpb<ROWS, 1>(rt, a, grid, shmem); break;
        case 2: coef_tpb<ROWS, 2>(rt, a, grid, shmem); break;
        case 8: coef_tpb<ROWS, 8>(rt, a, grid, shmem); break;
        default: coef_tpb<ROWS, 4>(rt, a, grid, shmem); break;
    }
}

// the kernel launch_flux would take for this batch, on fp32 planes; `raise` sets its dynamic-LDS limit instead
template <int ROWS, int K, bool MATRIX>
hipError_t flux_kernel(hx_rt* rt, const FluxArgs* f, dim3 grid, size_t shmem, int raise) {
    if (raise)
        return hipFuncSetAttribute((const void*)k_rt_flux_f32<ROWS, K, MATRIX>, hipFuncAttributeMaxDynamicSharedMemorySize, raise);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rt_flux_f32<ROWS, K, MATRIX>), grid, dim3(rt->g.threads), shmem, rt->ctx->stream, *f,
                       (const float*)rt->coef32);
    return hipSuccess;
}

template <int ROWS, bool MATRIX>
hipError_t flux_method(hx_rt* rt, const FluxArgs* f, dim3 grid, size_t shmem, int raise) {
    const int k = rt->g.k;
    const bool generic = rt->generic_scans;
    if constexpr (ROWS == 14) {
        (void)k; (void)generic;
        return flux_kernel<14, 16, MATRIX>(rt, f, grid, shmem, raise);   // (coef_fp32_tiling: k = 16 only)
    } else {
        if (k == 16 && !generic) return flux_kernel<ROWS, 16, MATRIX>(rt, f, grid, shmem, raise);
        if (k == 32 && !generic) return flux_kernel<ROWS, 32, MATRIX>(rt, f, grid, shmem, raise);
        if (k == 64 && !generic) return flux_kernel<ROWS, 64, MATRIX>(rt, f, grid, shmem, raise);
        return flux_kernel<ROWS, 0, MATRIX>(rt, f, grid, shmem, raise);
    }
}

template <int ROWS>
hipError_t flux_rows(hx_rt* rt, const FluxArgs* f, dim3 grid, size_t shmem, int raise) {
    return flux_method<ROWS, false>(rt, f, grid, shmem, raise);   // (the sweeps only: the matrix method keeps fp64 planes)
}

#define F32_DISPATCH_ROWS(fn, ...)                          \
    switch (rt->g.ROWS) {                                   \
        case 1: return fn<1>(rt, __VA_ARGS__);              \
        case 2: return fn<2>(rt, __VA_ARGS__);              \
        case 3: return fn<3>(rt, __VA_ARGS__);              \
        case 4: return fn<4>(rt, __VA_ARGS__);              \
        case 5: return fn<5>(rt, __VA_ARGS__);              \
        case 6: return fn<6>(rt, __VA_ARGS__);              \
        case 7: return fn<7>(rt, __VA_ARGS__);              \
        case 8: return fn<8>(rt, __VA_ARGS__);              \
        case 9: return fn<9>(rt, __VA_ARGS__);              \
        case 10: return fn<10>(rt, __VA_ARGS__);            \
        case 11: return fn<11>(rt, __VA_ARGS__);            \
        case 12: return fn<12>(rt, __VA_ARGS__);            \
        case 13: return fn<13>(rt, __VA_ARGS__);            \
        default: return fn<14>(rt, __VA_ARGS__);            \
    }

}  // namespace

// (the batch was given fp32 planes only where coef_fp32_tiling holds: rt_create_into)
void launch_coef_f32(hx_rt* rt, const KArgs& a, int tpb, dim3 grid, size_t shmem) {
    F32_DISPATCH_ROWS(coef_rows, a, tpb, grid, shmem);
}

void launch_flux_f32(hx_rt* rt, const FluxArgs& f, dim3 grid, size_t shmem) {
    (void)[&]() -> hipError_t { F32_DISPATCH_ROWS(flux_rows, &f, grid, shmem, 0); }();
}

hipError_t raise_flux_shmem_f32(hx_rt* rt, int shmem) {
    F32_DISPATCH_ROWS(flux_rows, nullptr, dim3(1), 0, shmem);
}

}  // namespace hx
