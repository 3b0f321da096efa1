// On-the-fly opacity mixing of the fused refresh: the species loop of
// calculate_total_opacity_and_scat_cross_sections_from_species (computation.py:1454-1501) and the host steps around it
// (host_functions.py:874-959, :1050-1056) as THREE launches for all columns, levels and species of a batch.
//
//   k_rt_species_prep   per (column, level): mean molecular mass from the mixing ratios, fractional (T, log10 P)
//                       table indices with the species clamp [0, n-1] (kernels.cu:3233, :3238), and the factor
//                       vmr * mass / mu of every absorber (:3293)
//   k_rt_mix_species    per (column, level, bin) -- one wavefront at a time: the running k-distribution stays in 20 lanes'
//                       registers while the absorbers are folded in one after the other (correlated-k for the first
//                       species and for CIA pairs, random overlap via ro::mix otherwise).  Each absorber's 20 coefficients
//                       are interpolated from the four table corners as they are needed (opac_species_interpol, :3209-3259:
//                       the reference writes them to a 161 MB array per species and reads them back); the next absorber's
//                       corners are in flight while the present one is mixed.  opac_wg_lay / opac_wg_int are written once.
//   k_rt_scat_species   per (column, level, bin): sum of vmr * sigma over the scattering species (add_to_mixed_scat,
//                       :3444-3459; water vapour through calc_h2o_scat, :3404-3440)
//
// Columns whose loop has ended (done[c]) are skipped on the device: no host round trip inside a refresh.
#pragma once
#include "random_overlap_ny.h"
#include "two_stream.h"

namespace hx {

struct SpeciesDev {
    const double* pretab;      // [t][p][x][y] flat (reference order) or null
    const double* scat_cross;  // [x] or null
    const double* vmr_tab;     // mixing ratio on the opacity tables' (T, P) grid, one table per column: [column][p + npress * t],
                               // or null: profile given by the host
    double weight;             // molar weight
    int absorbing, scattering, is_h2o, ro, in_mu, pad;
};

// Mixing ratio of a tabulated species at one level: bilinear in (T, log10 P) on the nodes of the opacity tables, clamped to
// the table edges -- interpolate_grid_to_lay_or_int (host_functions.py:904-910: scipy's RectBivariateSpline(kx = 1,
// ky = 1) evaluated point by point), in the term order of helios_amd/host_functions.py.  The nodes are searched (no
// uniform-grid assumption, as in scipy).
__device__ __forceinline__ int last_node_not_above(const double* grid, int n, double v, bool log_nodes) {
    int lo = 0, hi = n - 1;  // largest k in [0, n-2] with node(k) <= v (v is clamped into the grid)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const double node = log_nodes ? log10(grid[mid]) : grid[mid];
        if (node <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double vmr_from_table(const double* tab, double T, double P, const double* ktemp, int ntemp,
                                                 const double* kpress, int npress) {
    const double t = dmin(ktemp[ntemp - 1], dmax(ktemp[0], T));
    const double p = dmin(log10(kpress[npress - 1]), dmax(log10(kpress[0]), log10(P)));
    const int it = last_node_not_above(ktemp, ntemp, t, false), ip = last_node_not_above(kpress, npress, p, true);
    const double t0 = ktemp[it], t1 = ktemp[it + 1], p0 = log10(kpress[ip]), p1 = log10(kpress[ip + 1]);
    const double ft = (t - t0) / (t1 - t0), fp = (p - p0) / (p1 - p0);
    const double v00 = tab[ip + npress * it], v10 = tab[ip + npress * (it + 1)], v01 = tab[ip + 1 + npress * it],
                 v11 = tab[ip + 1 + npress * (it + 1)];
    return v00 * (1 - ft) * (1 - fp) + v10 * ft * (1 - fp) + v01 * (1 - ft) * fp + v11 * ft * fp;
}

struct MixArgs {
    int X, Y, L, I, C, S, ntemp, npress, nabs;
    int carry_on;          // 0: the mix starts from zero; 1: from what opac_wg_* holds -- the launch folds in the NEXT block of at most
                           // MIX_MAX_ABSORBERS absorbers of a longer species list (round 6)
    const SpeciesDev* sp;  // [S]
    const int* abs_list;   // [nabs] indices of the absorbing species of this launch, ascending
    const double *T_lay, *T_int, *p_lay, *p_int;  // column strides L+1, I, L, I
    const double *vmr_lay, *vmr_int;              // [C][S][I]
    const double *ktemp, *kpress, *gauss_w, *gauss_y, *wave;
    double *mmm_lay, *mmm_int;          // [C][I]
    TPIndex *tp_lay, *tp_int;           // [C][I]
    double *fac_lay, *fac_int;          // [C][I][S]
    double *opac_wg_lay, *opac_wg_int;  // [C][Y X I]
    double *scat_lay, *scat_int;        // [C][X I]
    const int* done;
    unsigned long long* diag;
};

constexpr int MIX_MAX_ABSORBERS = 48;  // LDS images of the species list: 1 KB next to the mixing images; a longer list takes
                                       // one launch per block of 48 (MixArgs::carry_on)

// The launches of k_rt_mix_species over the absorbers `abs_list[0 .. nabs_all)` of `m`, block by block (rt_fused.hip, where
// the kernel lives).  csrc/premix.hip hands it node records of its own: a pseudo-column of L = 0 layers and I = nodes interfaces.
// `any_ro`: one of the absorbers mixes by random overlap (SpeciesDev::ro) -- it selects the kernel when Y != 20.
int launch_mix_species(hx_context* ctx, MixArgs m, const int* abs_list, int nabs_all, bool any_ro);

#ifndef HX_SPECIES_DECLARATIONS_ONLY  // (premix.hip: the structures and vmr_from_table, not a second copy of the kernels)
// Level i of a column at (T, P): the mixing ratios of the species that come with a (T, P) table follow the temperatures, on
// the device (calculate_vmr_for_all_species, host_functions.py:874-901; `vmr` is the column's [S][I] block), then the mean
// molecular mass of the level (host_functions.py:927-959), which is returned
__device__ __forceinline__ double level_vmr_and_mmm(const SpeciesDev* __restrict__ sp, int S, double* vmr, int I, int i, int col,
                                                    double T, double P, const double* ktemp, int ntemp, const double* kpress,
                                                    int npress) {
    for (int s = 0; s < S; s++)
        if (sp[s].vmr_tab)
            vmr[(size_t)s * I + i] = vmr_from_table(sp[s].vmr_tab + (size_t)col * ntemp * npress, T, P, ktemp, ntemp, kpress, npress);
    double num = 0.0, tot = 0.0;
    for (int s = 0; s < S; s++)
        if (sp[s].in_mu) {
            num += vmr[(size_t)s * I + i] * sp[s].weight;
            tot += vmr[(size_t)s * I + i];
        }
    return num / tot * HX_AMU;
}

__global__ void k_rt_species_prep(MixArgs a) {
    const int col = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.I || a.done[col]) return;
    for (int pass = 0; pass < 2; pass++) {
        const bool lay = pass == 0;
        if (lay && i >= a.L) continue;
        double* vmr = const_cast<double*>(lay ? a.vmr_lay : a.vmr_int) + (size_t)col * a.S * a.I;
        const double T = lay ? a.T_lay[(size_t)col * (a.L + 1) + i] : a.T_int[(size_t)col * a.I + i];
        const double P = lay ? a.p_lay[(size_t)col * a.L + i] : a.p_int[(size_t)col * a.I + i];
        const double mmm = level_vmr_and_mmm(a.sp, a.S, vmr, a.I, i, col, T, P, a.ktemp, a.ntemp, a.kpress, a.npress);
        (lay ? a.mmm_lay : a.mmm_int)[(size_t)col * a.I + i] = mmm;
        (lay ? a.tp_lay : a.tp_int)[(size_t)col * a.I + i] = locate_tp(T, P, a.ktemp, a.ntemp, a.kpress, a.npress, false, false);
        double* fac = (lay ? a.fac_lay : a.fac_int) + ((size_t)col * a.I + i) * a.S;
        for (int s = 0; s < a.S; s++) {
            const double mass = a.sp[s].weight * HX_AMU;
            fac[s] = vmr[(size_t)s * a.I + i] * mass / mmm;  // (vmr * mass) / mu, then times kappa (:3293)
        }
    }
}

// mean molecular mass of the layers only (the convection loop refreshes it ahead of the adjustment, computation.py:1030-1036),
// of finished columns too (the mixing ratios of tabulated species are brought up to the present layer temperatures first, :1035)
__global__ void k_rt_mmm_from_vmr(const SpeciesDev* __restrict__ sp, int S, double* __restrict__ vmr_lay,
                                  double* __restrict__ mmm_lay, int L, int I, const double* __restrict__ T_lay,
                                  const double* __restrict__ p_lay, const double* __restrict__ ktemp, int ntemp,
                                  const double* __restrict__ kpress, int npress) {
    const int col = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    mmm_lay[(size_t)col * I + i] = level_vmr_and_mmm(sp, S, vmr_lay + (size_t)col * S * I, I, i, col, T_lay[(size_t)col * (L + 1) + i],
                                                     p_lay[(size_t)col * L + i], ktemp, ntemp, kpress, npress);
}

// ro::mix keeps this kernel within 7.9 KB of LDS and 96 VGPRs: five wavefronts per SIMD (tests/test_abi.py)
#define RT_MIX_KERNEL k_rt_mix_species
#define RT_MIX_ATTR __attribute__((amdgpu_waves_per_eu(5)))
#define RT_MIX_INIT(sh, lane, a) ro::init(sh, lane, a.gauss_w, a.gauss_y)
#define RT_MIX ro::mix
#include "rt_mix_species_kernel.inc"
#undef RT_MIX_KERNEL
#undef RT_MIX_ATTR
#undef RT_MIX_INIT
#undef RT_MIX

// the same loop with the general mixer (random_overlap_ny.h): random overlap at 2 ... 19 Gauss points, selected by the host
#define RT_MIX_KERNEL k_rt_species_mix_ny
#define RT_MIX_ATTR
#define RT_MIX_INIT(sh, lane, a) ro::init_ny(sh, lane, a.Y, a.gauss_w, a.gauss_y)
#define RT_MIX ro::mix_ny
#include "rt_mix_species_kernel.inc"
#undef RT_MIX_KERNEL
#undef RT_MIX_ATTR
#undef RT_MIX_INIT
#undef RT_MIX

__global__ void __launch_bounds__(256) k_rt_scat_species(MixArgs a) {
    const int col = blockIdx.z, lev = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.X || a.done[col]) return;
    const bool lay = lev < a.L;
    const int i = lay ? lev : lev - a.L;
    const double* vmr = (lay ? a.vmr_lay : a.vmr_int) + (size_t)col * a.S * a.I;
    const double T = lay ? a.T_lay[(size_t)col * (a.L + 1) + i] : a.T_int[(size_t)col * a.I + i];
    const double P = lay ? a.p_lay[(size_t)col * a.L + i] : a.p_int[(size_t)col * a.I + i];
    double sum = 0.0;
    for (int s = 0; s < a.S; s++) {
        if (!a.sp[s].scattering) continue;
        const double f = vmr[(size_t)s * a.I + i];
        const double sigma = a.sp[s].is_h2o ? h2o_rayleigh_cross(T, P, f, a.wave[x], a.sp[s].weight * HX_AMU)
                                            : a.sp[s].scat_cross[x];
        sum += f * sigma;
    }
    (lay ? a.scat_lay : a.scat_int)[(size_t)col * a.X * a.I + x + (size_t)a.X * i] = sum;
}

#endif  // HX_SPECIES_DECLARATIONS_ONLY

}  // namespace hx
