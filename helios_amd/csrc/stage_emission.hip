// Angular emission spectrum of a column: the formal solution of the transfer equation along N emission angles, with a
// source linear in tau per shell built from the run's own fluxes (README, "Angular emission spectrum"; not in the
// reference).
//
// Every operation is written in the order of the contract's plain fp64 statement (tests/emission_reference.py) and the
// library is built with -ffp-contract=off, so everything but exp() and expm1() rounds exactly like that statement; only
// those two are the device's own.
#include "hx_common.h"

namespace {

constexpr int NA = 16;   // emission angles a thread carries in registers (the option's upper limit)
constexpr int TT = 256;  // threads per workgroup

constexpr double T_SWITCH = 0.05;  // below it the weights of the source come from their series, ten terms

struct EmissionArgs {
    // shell arrays: [c + nc * i] (c = y + ny * x) and, the clouds', [x + nbin * i].  Isothermal layers: the `_a` arrays are
    // the layers', the `_b` ones null; otherwise `_a` is the lower half of layer i and `_b` its upper half
    const double *dtau_a, *dtau_b, *cloud_a, *cloud_b, *w0_a, *w0_b;
    const double *planck_lay, *planck_int;     // [i + x * (nlayer + 2)], [i + x * (nlayer + 1)]
    const double *F_up, *F_down, *F_dir;       // interfaces, [c + nc * i]; F_dir null: no beam
    const double *Fc_up, *Fc_down, *Fc_dir;    // layer centres (non-isothermal layers only)
    const double *gauss_weight, *mu_inv;
    double beta;
    double *I_band, *I_wg;
    int nbin, ny, nlayer, nangle;
};

// what one layer's step needs beyond the boundary below it, loaded a layer ahead of its use
struct LayerLoad {
    double dt_a, cl_a, w_a, dt_b, cl_b, w_b;   // optical depths and albedo of the shell(s)
    double B_mid, B_top;                       // Planck value of the layer (its centre) and of the interface above
    double fu_mid, fd_mid, fr_mid;             // fluxes at the centre
    double fu_top, fd_top, fr_top;             // fluxes at the interface above
};

template <bool NONISO>
__device__ __forceinline__ LayerLoad load_layer(const EmissionArgs& p, size_t c, size_t nc, long long x, int i) {
    LayerLoad l = {};
    const size_t k = c + nc * i, b = (size_t)x + (size_t)p.nbin * i;
    const bool beam = p.F_dir != nullptr;
    l.dt_a = p.dtau_a[k];
    l.cl_a = p.cloud_a[b];
    l.w_a = p.w0_a[k];
    // the Planck arrays are layer-fastest: the lanes of a bin read one address, and the 128-byte line it lies in serves the
    // next fifteen layers of the walk from the caches
    l.B_mid = p.planck_lay[(size_t)x * (p.nlayer + 2) + i];
    l.fu_top = p.F_up[k + nc];
    l.fd_top = p.F_down[k + nc];
    l.fr_top = beam ? p.F_dir[k + nc] : 0.0;
    if (NONISO) {
        l.dt_b = p.dtau_b[k];
        l.cl_b = p.cloud_b[b];
        l.w_b = p.w0_b[k];
        l.B_top = p.planck_int[(size_t)x * (p.nlayer + 1) + i + 1];
        l.fu_mid = p.Fc_up[k];
        l.fd_mid = p.Fc_down[k];
        l.fr_mid = beam ? p.Fc_dir[k] : 0.0;
    }
    return l;
}

// J = (F_up + F_down) / (2 pi) + beta |F_dir|; without a beam the last term is absent
__device__ __forceinline__ double mean_intensity(double fu, double fd, double fr, double beta, bool beam) {
    double J = (fu + fd) / (2.0 * HX_PI);
    if (beam) J = J + beta * fabs(fr);
    return J;
}

// one shell along one angle: I <- I e + S_top a + S_bot b with t = dtau / mu
__device__ __forceinline__ void angle_step(double& I, double t, double S_bot, double S_top) {
    double e, a, b;
    if (t >= T_SWITCH) {
        const double u = -expm1(-t);
        e = 1.0 - u;
        const double q = u / t;
        a = 1.0 - q;
        b = q - e;
    } else {
        e = exp(-t);
        // c_n = (-1)^(n+1) / (n+1)!,  d_n = (-1)^(n+1) n / (n+1)!,  n = 1 ... 10: each one division of two exact numbers
        constexpr double C[10] = {1.0 / 2.0,     -1.0 / 6.0,    1.0 / 24.0,      -1.0 / 120.0,    1.0 / 720.0,
                                  -1.0 / 5040.0, 1.0 / 40320.0, -1.0 / 362880.0, 1.0 / 3628800.0, -1.0 / 39916800.0};
        constexpr double D[10] = {1.0 / 2.0,     -2.0 / 6.0,    3.0 / 24.0,      -4.0 / 120.0,    5.0 / 720.0,
                                  -6.0 / 5040.0, 7.0 / 40320.0, -8.0 / 362880.0, 9.0 / 3628800.0, -10.0 / 39916800.0};
        double pw = t;
        a = pw * C[0];
        b = pw * D[0];
#pragma unroll
        for (int n = 1; n < 10; n++) {  // every term formed and added in ascending n
            pw = pw * t;
            a = a + pw * C[n];
            b = b + pw * D[n];
        }
    }
    I = (I * e + S_top * a) + S_bot * b;
}

// one shell, upward, for the first `nangle` angles.  The angles are independent; the switch enters the unrolled chain at
// the last one, so the count costs one scalar jump and every intensity keeps its register
__device__ __forceinline__ void shell_step(double (&I)[NA], const double* __restrict__ mu_inv, int nangle, double dtau,
                                           double w0, double B_bot, double J_bot, double B_top, double J_top) {
    const double S_bot = (1.0 - w0) * B_bot + w0 * J_bot;
    const double S_top = (1.0 - w0) * B_top + w0 * J_top;
#define HX_EM_ANGLE(M)                                                                                                 \
    case M + 1:                                                                                                        \
        angle_step(I[M], dtau * mu_inv[M], S_bot, S_top);                                                              \
        [[fallthrough]];
    switch (nangle) {
        HX_EM_ANGLE(15) HX_EM_ANGLE(14) HX_EM_ANGLE(13) HX_EM_ANGLE(12) HX_EM_ANGLE(11) HX_EM_ANGLE(10) HX_EM_ANGLE(9)
        HX_EM_ANGLE(8) HX_EM_ANGLE(7) HX_EM_ANGLE(6) HX_EM_ANGLE(5) HX_EM_ANGLE(4) HX_EM_ANGLE(3) HX_EM_ANGLE(2)
        HX_EM_ANGLE(1) HX_EM_ANGLE(0)
        default:
            break;
    }
#undef HX_EM_ANGLE
}

// A workgroup owns TT / ny whole bins (thread = one (x, y), c = y + ny * x contiguous over the threads, so every load of
// a spectral point's value is coalesced) and a thread the intensities of all angles in registers.  It walks the layers
// upward once; a layer's values are requested a layer ahead of their use.  1 / mu is the same for every lane and comes
// through scalar loads.  The Gauss sum of a bin runs through LDS in the order of y, so it does not depend on how bins fall
// on wavefronts.
template <bool NONISO>
__global__ void __launch_bounds__(TT) k_emission_angles(EmissionArgs p) {
    __shared__ double sm[NA * TT];
    const int ny = p.ny, nangle = p.nangle, L = p.nlayer;
    const int pb = TT / ny;  // whole bins per workgroup
    const int t = threadIdx.x;
    const int xl = t / ny, y = t - xl * ny;
    const long long x0 = (long long)blockIdx.x * pb;  // the workgroup's first bin
    const long long x = x0 + xl;
    const bool active = xl < pb && x < p.nbin;
    const size_t nc = (size_t)ny * p.nbin;
    const size_t c = (size_t)x * ny + y;
    const bool beam = p.F_dir != nullptr;
    const double* __restrict__ mu_inv = p.mu_inv;
    double I[NA];
#pragma unroll
    for (int m = 0; m < NA; m++) I[m] = 0.0;
    if (active) {
        const double fu0 = p.F_up[c];
        // boundary 0: the run's own BOA up-flux, taken as isotropic
        const double I0 = fu0 / HX_PI;
#pragma unroll
        for (int m = 0; m < NA; m++) I[m] = I0;
        double J_bot = mean_intensity(fu0, p.F_down[c], beam ? p.F_dir[c] : 0.0, p.beta, beam);
        double B_bot = NONISO ? p.planck_int[(size_t)x * (L + 1)] : 0.0;
        LayerLoad next = load_layer<NONISO>(p, c, nc, x, 0);
        for (int i = 0; i < L; i++) {
            const LayerLoad l = next;
            next = load_layer<NONISO>(p, c, nc, x, i + 1 < L ? i + 1 : i);
            const double J_top = mean_intensity(l.fu_top, l.fd_top, l.fr_top, p.beta, beam);
            if (NONISO) {
                // shell 2i: the lower half of layer i, shell 2i + 1: its upper half
                const double J_mid = mean_intensity(l.fu_mid, l.fd_mid, l.fr_mid, p.beta, beam);
                shell_step(I, mu_inv, nangle, l.dt_a + l.cl_a, l.w_a, B_bot, J_bot, l.B_mid, J_mid);
                shell_step(I, mu_inv, nangle, l.dt_b + l.cl_b, l.w_b, l.B_mid, J_mid, l.B_top, J_top);
                B_bot = l.B_top;
            } else {
                // an isothermal layer has its own Planck value at both ends
                shell_step(I, mu_inv, nangle, l.dt_a + l.cl_a, l.w_a, l.B_mid, J_bot, l.B_mid, J_top);
            }
            J_bot = J_top;
        }
        if (p.I_wg) {
#pragma unroll
            for (int m = 0; m < NA; m++)
                if (m < nangle) p.I_wg[(size_t)m * nc + c] = I[m];
        }
    }
    const double hw = active ? 0.5 * p.gauss_weight[y] : 0.0;
#pragma unroll
    for (int m = 0; m < NA; m++)
        if (m < nangle) sm[m * TT + t] = hw * I[m];
    __syncthreads();
    for (int r = t; r < pb * nangle; r += TT) {
        const int m = r / pb, xq = r - m * pb;
        const long long xx = x0 + xq;
        if (xx < p.nbin) {
            const double* term = sm + m * TT + xq * ny;
            double acc = 0.0;
            for (int yy = 0; yy < ny; yy++) acc = acc + term[yy];
            p.I_band[(size_t)m * p.nbin + xx] = acc;
        }
    }
}

}  // namespace

extern "C" {

int hx_emission_angles(hx_context* ctx, const double* delta_tau_wg, const double* delta_tau_wg_upper,
                       const double* delta_tau_clouds, const double* delta_tau_clouds_upper, const double* w_0,
                       const double* w_0_upper, const double* planckband_lay, const double* planckband_int,
                       const double* F_up_wg, const double* F_down_wg, const double* F_dir_wg, const double* Fc_up_wg,
                       const double* Fc_down_wg, const double* Fc_dir_wg, const double* gauss_weight,
                       const double* mu_inv, double beta, int nbin, int ny, int nlayer, int nangle, double* I_band,
                       double* I_wg) {
    const bool noniso = delta_tau_wg_upper != nullptr;
    const bool beam = F_dir_wg != nullptr;
    HX_REQUIRE(ctx, nbin >= 1 && nlayer >= 1, HX_E_ARG, "at least one bin and one layer");
    HX_REQUIRE(ctx, nangle >= 1 && nangle <= NA, HX_E_ARG, "1 to 16 emission angles");
    HX_REQUIRE(ctx, ny >= 1 && ny <= TT, HX_E_UNSUPPORTED, "more than 256 Gauss points per bin");
    HX_REQUIRE(ctx, noniso == (delta_tau_clouds_upper != nullptr) && noniso == (w_0_upper != nullptr), HX_E_ARG,
               "the upper-half arrays of gas, clouds and albedo come together");
    HX_REQUIRE(ctx, delta_tau_wg && delta_tau_clouds && w_0 && planckband_lay && F_up_wg && F_down_wg && gauss_weight &&
                        mu_inv && I_band,
               HX_E_ARG, "null array");
    HX_REQUIRE(ctx, !noniso || (planckband_int && Fc_up_wg && Fc_down_wg && (Fc_dir_wg != nullptr) == beam), HX_E_ARG,
               "half-layer shells need the interfaces' Planck values and the centres' fluxes");
    const long long nblocks = hx_cdiv(nbin, TT / ny);
    EmissionArgs p = {delta_tau_wg, delta_tau_wg_upper, delta_tau_clouds, delta_tau_clouds_upper, w_0, w_0_upper,
                      planckband_lay, planckband_int, F_up_wg, F_down_wg, F_dir_wg, Fc_up_wg, Fc_down_wg, Fc_dir_wg,
                      gauss_weight, mu_inv, beam ? beta : 0.0, I_band, I_wg, nbin, ny, nlayer, nangle};
    if (noniso)
        k_emission_angles<true><<<dim3((unsigned)nblocks), TT, 0, ctx->stream>>>(p);
    else
        k_emission_angles<false><<<dim3((unsigned)nblocks), TT, 0, ctx->stream>>>(p);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

}  // extern "C"
