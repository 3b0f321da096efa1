// How the fp32 coefficient planes (`precision = single`, hx_rt_flags.coef_fp32) hold alpha, beta and rest = 1 - alpha - beta.
// Included by rt_kernels.h; plain C++ as well, so that tests/test_precision_single.py compiles these very functions on the host.
//
// Rounded one by one, the fp64 planes' values would lose what a thin half-layer emits: its emission K (1 - alpha - beta) B --
// u' + v' -- is a small difference of values near one (alpha ~ 1, u' and v' of opposite sign), and an fp32 rounding of each
// is an error of 6e-8 / dtau relative to it: a few per cent in the thin top layers of a column, where it decides the
// equilibrium temperature (measured: a whole on-the-fly run at 500 x 50 x 6 did not converge).  So the fp32 planes store the
// same tiles in a form without cancellation, each value computed in fp64 and rounded once:
//   plane 0: the smaller of alpha and rest -- alpha as +alpha, rest as -rest: the sign bit is the tag (-0.0 is rest = 0);
//   plane 1: beta, or -(1 - beta) when beta > 1/2;
//   v' plane: u' + v' in place of v' (rt_coef_kernel.inc).
// k_rt_flux_f32 forms the larger of alpha and rest as (1 - beta) - the smaller, in fp64: no value is a difference of nearly
// equal ones, so alpha, beta and rest all keep about fp32's relative precision.
// The tag must not depend on the sign of the value it tags: rest, computed in fp64 as (1 - alpha) - beta, comes out slightly
// negative for nearly conservative scatterers (w0 at w_0_limit: -1.4e-12 at dtau = 7e-8), and stored as -rest that would be a
// positive code, read back as alpha = 1.4e-12.  So every value is clamped to >= +0.0 before it is tagged.
#pragma once

#ifdef __HIPCC__
#define HX_PLANE_HD __host__ __device__ __forceinline__
#else
#define HX_PLANE_HD inline
#endif

namespace hx {

HX_PLANE_HD double plane_nonneg(double v) { return v > 0.0 ? v : 0.0; }   // (-0.0 and negative values -> +0.0)

HX_PLANE_HD float plane0_code(double alpha, double beta) {
    const double a = plane_nonneg(alpha), rest = plane_nonneg((1.0 - alpha) - beta);
    return a <= rest ? (float)a : -(float)rest;
}
HX_PLANE_HD float plane1_code(double beta) {
    return beta > 0.5 ? -(float)plane_nonneg(1.0 - beta) : (float)plane_nonneg(beta);
}
// codes -> alpha, beta (in place) and rest
HX_PLANE_HD double plane_decode(double& al, double& be) {
    const double c0 = al, c1 = be;
    const bool rest0 = __builtin_signbit(c0), comp1 = __builtin_signbit(c1);
    const double one_minus_beta = comp1 ? -c1 : 1.0 - c1;
    const double small = __builtin_fabs(c0), large = one_minus_beta - small;
    be = comp1 ? 1.0 + c1 : c1;
    al = rest0 ? large : small;
    return rest0 ? small : large;
}

}  // namespace hx
