// `precision = single`: the coefficient kernel and the flux kernel on fp32 coefficient planes (hx_rt_flags.coef_fp32).
// Same source as the fp64 kernels of rt_fused.hip (rt_coef_kernel.inc, rt_flux_kernel.inc, plane element type CT = float):
// the planes -- coded without cancellation, plane_code.h -- are rounded to fp32 once, where k_rt_coef_f32 stores
// them, and widened to fp64 where k_rt_flux_f32 loads them; all arithmetic, the up-flux state and everything else stay
// fp64.  A translation unit of its own, so that the build compiles these instantiations next to rt_fused.hip's instead of
// after them.
#define HX_PLANE_KERNELS_ONLY
#include "rt_select.h"

using namespace hx;

namespace hx {

// Columns of up to 416 layers (832 half-layers) get at most 13 rows on 64 lanes; the one 14-row tiling choose_geometry picks
// without scratch is k = 16 with the compile-time scans.  The fp64 kernels of 14 rows on other lane counts and of 15 rows and
// more keep part of their register image in scratch (rt_fused.hip, flux_variant_spills): those tilings have no fp32 variant.
bool coef_fp32_tiling(int rows, int k, bool generic_scans) {
    return rows <= 13 || (rows == 14 && k == 16 && !generic_scans);
}

hipError_t select_flux_f32(hx_rt* rt, const FluxArgs* f) { return select_flux<float>(rt, f); }
void select_coef_f32(hx_rt* rt, const KArgs& a, dim3 grid, size_t shmem) { select_coef<float>(rt, a, grid, shmem); }

}  // namespace hx
