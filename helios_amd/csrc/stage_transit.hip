// Transit depth spectrum of a column: slant-path optical depths through homogeneous spherical shells, band transmission
// per impact parameter and the occulting area per bin (README, "Transit depth spectrum"; not in the reference).
//
// Every operation is written in the order of the contract's plain fp64 statement (tests/transit_reference.py) and the
// library is built with -ffp-contract=off, so the optical depths round exactly like that statement; only exp() is the
// device's own.
#include "hx_common.h"

namespace {

constexpr int TB = 16;   // impact parameters a thread carries in registers (hx_transit_chord_block)
constexpr int TT = 256;  // threads per workgroup

// Geometry shared by every spectral point: dz[s] = zb[s+1] - zb[s] and the path lengths, one row of TB chords per
// (chord block jb, shell s): G[(jb * S + s) * TB + b] = l_{s,j}, j = jb * TB + b; 0 where the chord passes below shell s
// (j > s) or does not exist (j >= S).  q is taken in its product form, z - z_j from altitudes before any radius is added.
__global__ void __launch_bounds__(TT)
k_transit_geometry(double* __restrict__ G, double* __restrict__ dz, const double* __restrict__ zb, double R0, int S,
                   int njb) {
    const long long n = (long long)njb * S * TB;
    const long long t = (long long)blockIdx.x * TT + threadIdx.x;
    if (t < S) dz[t] = zb[t + 1] - zb[t];
    if (t >= n) return;
    const int b = (int)(t % TB);
    const long long row = t / TB;
    const int s = (int)(row % S);
    const long long j = (row / S) * TB + b;
    double ell = 0.0;
    if (j <= s) {
        const double zj = (zb[j] + zb[j + 1]) / 2.0;
        const double bj = R0 + zj;
        const double q_up = sqrt((zb[s + 1] - zj) * ((R0 + zb[s + 1]) + bj));
        const double q_low = j == s ? 0.0 : sqrt((zb[s] - zj) * ((R0 + zb[s]) + bj));
        ell = 2.0 * (q_up - q_low);
    }
    G[t] = ell;
}

// A workgroup owns TT / ny whole bins (thread = one (x, y), c = y + ny * x contiguous over the threads) and the TB
// chords of one block.  It walks the shells upward from the block's first chord, reads each optical depth once
// (coalesced over c), divides by the shell's thickness and adds alpha * l to the TB optical depths in registers; the row
// of path lengths is the same for every lane and comes through scalar loads.  The chord block is the fastest index of
// the grid: the workgroups that read the same optical depths run next to each other, so an array of 320 MB comes from
// HBM about once and the re-reads of the other chord blocks from the caches.  The Gauss sum of a bin runs through LDS in
// the order of y, so it does not depend on how bins fall on wavefronts.
template <bool NONISO>
__global__ void __launch_bounds__(TT)
k_transit_chords(double* __restrict__ T_band, const double* __restrict__ dtau_a, const double* __restrict__ dtau_b,
                 const double* __restrict__ cloud_a, const double* __restrict__ cloud_b,
                 const double* __restrict__ G, const double* __restrict__ dz, const double* __restrict__ gauss_weight,
                 int nbin, int ny, int S, int njb) {
    __shared__ double sm[TB * TT];
    const int pb = TT / ny;  // whole bins per workgroup
    const int t = threadIdx.x;
    const int xl = t / ny, y = t - xl * ny;
    const int jb = blockIdx.x % njb;
    const long long x0 = (long long)(blockIdx.x / njb) * pb;  // the workgroup's first bin
    const long long x = x0 + xl;
    const bool active = xl < pb && x < nbin;
    const size_t nc = (size_t)ny * nbin;
    const size_t c = (size_t)x * ny + y;
    const int j0 = jb * TB;
    const double* __restrict__ g = G + (size_t)jb * S * TB;
    double tau[TB];
#pragma unroll
    for (int b = 0; b < TB; b++) tau[b] = 0.0;
    if (active) {
        // shell 2i: lower half of layer i, shell 2i + 1: its upper half
        auto gas_of = [&](int s) {
            return ((NONISO && (s & 1)) ? dtau_b : dtau_a)[c + nc * (NONISO ? s >> 1 : s)];
        };
        auto cloud_of = [&](int s) {
            return ((NONISO && (s & 1)) ? cloud_b : cloud_a)[(size_t)x + (size_t)nbin * (NONISO ? s >> 1 : s)];
        };
        double gas_next = gas_of(j0), cl_next = cloud_of(j0);
        for (int s = j0; s < S; s++) {
            const double gas = gas_next, cl = cl_next;
            const int sn = s + 1 < S ? s + 1 : s;  // the next shell's values are requested a shell ahead of their use
            gas_next = gas_of(sn);
            cl_next = cloud_of(sn);
            const double alpha = (gas + cl) / dz[s];
            const double* __restrict__ row = g + (size_t)s * TB;
#pragma unroll
            for (int b = 0; b < TB; b++) tau[b] = tau[b] + alpha * row[b];
        }
    }
    const double hw = active ? 0.5 * gauss_weight[y] : 0.0;
#pragma unroll
    for (int b = 0; b < TB; b++) sm[b * TT + t] = hw * exp(-tau[b]);
    __syncthreads();
    for (int r = t; r < pb * TB; r += TT) {
        const int b = r / pb, xq = r - b * pb;
        const long long xx = x0 + xq;
        const int j = j0 + b;
        if (xx < nbin && j < S) {
            const double* term = sm + b * TT + xq * ny;
            double acc = 0.0;
            for (int yy = 0; yy < ny; yy++) acc = acc + term[yy];
            T_band[(size_t)j * nbin + xx] = acc;
        }
    }
}

// midpoint rule in b^2 over the chords, in ascending order; the deepest chord's transmission
__global__ void __launch_bounds__(TT)
k_transit_area(double* __restrict__ A, double* __restrict__ T_floor, const double* __restrict__ T_band,
               const double* __restrict__ zb, double R0, int nbin, int S) {
    const long long x = (long long)blockIdx.x * TT + threadIdx.x;
    if (x >= nbin) return;
    double a = 0.0;
#pragma unroll 8
    for (int j = 0; j < S; j++)
        a = a + ((1.0 - T_band[(size_t)j * nbin + x]) * (zb[j + 1] - zb[j])) * ((2.0 * R0 + zb[j + 1]) + zb[j]);
    A[x] = a;
    T_floor[x] = T_band[x];
}

long long chord_blocks(int nshell) { return ((long long)nshell + TB - 1) / TB; }

}  // namespace

extern "C" {

int hx_transit_chord_block(void) { return TB; }

int64_t hx_transit_work_doubles(int nshell, int nbin) {
    if (nshell < 1 || nbin < 1) return 0;
    return chord_blocks(nshell) * nshell * TB + nshell + (int64_t)nshell * nbin;
}

int hx_transit_depth(hx_context* ctx, const double* delta_tau_wg, const double* delta_tau_wg_upper,
                     const double* delta_tau_clouds, const double* delta_tau_clouds_upper, const double* zb,
                     const double* gauss_weight, double R0, int nbin, int ny, int nshell, double* work, double* A,
                     double* T_floor, double* T_band) {
    const bool noniso = delta_tau_wg_upper != nullptr;
    HX_REQUIRE(ctx, nbin >= 1 && nshell >= 1, HX_E_ARG, "at least one bin and one shell");
    HX_REQUIRE(ctx, ny >= 1 && ny <= TT, HX_E_UNSUPPORTED, "more than 256 Gauss points per bin");
    HX_REQUIRE(ctx, noniso == (delta_tau_clouds_upper != nullptr), HX_E_ARG,
               "the upper-half arrays of gas and clouds come together");
    HX_REQUIRE(ctx, !noniso || nshell % 2 == 0, HX_E_ARG, "half-layer shells come in pairs");
    HX_REQUIRE(ctx, delta_tau_wg && delta_tau_clouds && zb && gauss_weight && work && A && T_floor, HX_E_ARG,
               "null array");
    const long long njb = chord_blocks(nshell);
    const long long nblocks = njb * hx_cdiv(nbin, TT / ny);
    HX_REQUIRE(ctx, nblocks <= 0x7fffffffLL && njb * nshell * TB / TT < 0x7fffffffLL, HX_E_UNSUPPORTED,
               "more than 2^31 - 1 workgroups");
    double* G = work;
    double* dz = G + njb * nshell * TB;
    double* Tb = T_band ? T_band : dz + nshell;
    k_transit_geometry<<<hx_cdiv(njb * nshell * TB, TT), TT, 0, ctx->stream>>>(G, dz, zb, R0, nshell, (int)njb);
    HX_LAUNCH_CHECK(ctx);
    const dim3 grid((unsigned)nblocks);
    if (noniso)
        k_transit_chords<true><<<grid, TT, 0, ctx->stream>>>(Tb, delta_tau_wg, delta_tau_wg_upper, delta_tau_clouds,
                                                            delta_tau_clouds_upper, G, dz, gauss_weight, nbin, ny,
                                                            nshell, (int)njb);
    else
        k_transit_chords<false><<<grid, TT, 0, ctx->stream>>>(Tb, delta_tau_wg, nullptr, delta_tau_clouds, nullptr, G,
                                                             dz, gauss_weight, nbin, ny, nshell, (int)njb);
    HX_LAUNCH_CHECK(ctx);
    k_transit_area<<<hx_cdiv(nbin, TT), TT, 0, ctx->stream>>>(A, T_floor, Tb, zb, R0, nbin, nshell);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

}  // extern "C"
