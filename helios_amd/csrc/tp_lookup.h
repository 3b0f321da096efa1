// The bilinear look-up on a uniform (T, log10 P) grid (reference source/kernels.cu:524-610, :649-699, :3209-3259): index, blend,
// the gather of the four corners, and the launches of the two kernels (stage_interp.hip) that serve the stage API with one column
// and the device loop with all of a batch.  rt_coef_kernel.inc and rt_mix_species_kernel.inc apply locate_tp / blend_tp themselves.
#pragma once
#include "hx_common.h"

namespace hx {

// fractional table index on a uniform (T, log10 P) grid; margin 0.001 (premixed, :545-559) or 0 (per-species tables, :3228-3241)
struct TPIndex {
    double t, p;
    int tdown, tup, pdown, pup;
};

__device__ __forceinline__ TPIndex locate_tp(double temp, double press, const double* tgrid, int ntemp, const double* pgrid,
                                             int npress, bool margin, bool log_t) {  // (fmin, fmax: two_stream.h's dmin, dmax)
    TPIndex k;
    double t;
    if (log_t) {
        const double dt = (log10(tgrid[ntemp - 1]) - log10(tgrid[0])) / (ntemp - 1.0);
        t = (log10(temp) - log10(tgrid[0])) / dt;
    } else {
        const double dt = (tgrid[ntemp - 1] - tgrid[0]) / (ntemp - 1.0);
        t = (temp - tgrid[0]) / dt;
    }
    const double dp = (log10(pgrid[npress - 1]) - log10(pgrid[0])) / (npress - 1.0);
    double p = (log10(press) - log10(pgrid[0])) / dp;
    if (margin) {
        t = fmin(ntemp - 1.001, fmax(0.001, t));
        p = fmin(npress - 1.001, fmax(0.001, p));
    } else {
        t = fmin(ntemp - 1.0, fmax(0.0, t));
        p = fmin(npress - 1.0, fmax(0.0, p));
    }
    k.t = t;
    k.p = p;
    k.tdown = (int)floor(t);
    k.tup = (int)ceil(t);
    k.pdown = (int)floor(p);
    k.pup = (int)ceil(p);
    return k;
}

// four-case bilinear blend (:561-608); `species` selects the term order of :637-640
__device__ __forceinline__ double blend_tp(double dd, double ud, double du, double uu, const TPIndex& k, bool species) {
    if (k.pdown != k.pup && k.tdown != k.tup)
        return dd * (k.pup - k.p) * (k.tup - k.t) + ud * (k.p - k.pdown) * (k.tup - k.t) +
               du * (k.pup - k.p) * (k.t - k.tdown) + uu * (k.p - k.pdown) * (k.t - k.tdown);
    if (k.tdown == k.tup && k.pdown != k.pup) return dd * (k.pup - k.p) + ud * (k.p - k.pdown);
    if (k.pdown == k.pup && k.tdown != k.tup)
        return species ? du * (k.t - k.tdown) + dd * (k.tup - k.t) : dd * (k.tup - k.t) + du * (k.t - k.tdown);
    return dd;
}

// entry `c` of a table laid out [t][p][c] (sp, st: elements per pressure and per temperature node) at index k
__device__ __forceinline__ double gather_tp(const double* tab, size_t c, size_t sp, size_t st, const TPIndex& k, bool species) {
    return blend_tp(tab[c + sp * k.pdown + st * k.tdown], tab[c + sp * k.pup + st * k.tdown],
                    tab[c + sp * k.pdown + st * k.tup], tab[c + sp * k.pup + st * k.tup], k, species);
}

// ---- where a level's index comes from (Src): at(col, set, i) for up to two level sets (layers, interfaces), skip(col) ------
// the levels themselves: temperatures and pressures [column][level], a stride per array, and the grid they are located on
struct TPLevels {
    const double *temp[2], *press[2];
    size_t temp_col[2], press_col[2];
    const double *tgrid, *pgrid;
    int ntemp, npress;
    const hx_rt_column* time_stepped;  // non-null: only the columns with a physical time step of their own
};
template <bool MARGIN, bool LOG_T>
struct TPLocate {  // computed from the levels
    TPLevels v;
    __device__ bool skip(int col) const { return v.time_stepped && v.time_stepped[col].physical_tstep == 0; }
    __device__ TPIndex at(int col, int set, int i) const {
        return locate_tp(v.temp[set][col * v.temp_col[set] + i], v.press[set][col * v.press_col[set] + i], v.tgrid, v.ntemp,
                         v.pgrid, v.npress, MARGIN, LOG_T);
    }
};
struct TPStored {  // read from the arrays k_rt_tp_index left behind, [column][tp_col]; a finished column is skipped
    const TPIndex* tp[2];
    size_t tp_col;
    const int* done;
    __device__ bool skip(int col) const { return done[col] != 0; }
    __device__ TPIndex at(int col, int set, int i) const { return tp[set][col * tp_col + i]; }
};

// a table per column (Tab): of(col).  One table for all columns here; rt_fused.hip has the member of the device's TableSet array
struct OneTable {
    const double* t;
    __device__ const double* of(int) const { return t; }
};

// One look-up launch: nlev[s] levels in set s, which writes out[s] + col * out_col for column col
template <class Tab>
struct TPLaunch {
    Tab tab;
    double* out[2];
    size_t out_col, nc;  // nc: entries per level of a spectral table
    int npress, nlev[2], ncol;
};
// a second table [t][p][x], x < nx, looked up in the same spectral launch (the Rayleigh cross-sections of hx_opac_interpol)
struct TPSecond {
    const double* tab;
    double* out[2];
    size_t out_col;
    int nx;
};

// scalar table [t][p]: level i -> out[i] (mean molecular mass :649, kappa :703, c_p :761); grid (levels / 64, columns)
template <class Src, class Tab>
__global__ void k_tp_scalar(Src src, TPLaunch<Tab> q) {
    const int col = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (src.skip(col)) return;
    const double* __restrict__ table = q.tab.of(col);
    for (int set = 0; set < 2; set++)
        if (i < q.nlev[set]) q.out[set][col * q.out_col + i] = gather_tp(table, 0, 1, q.npress, src.at(col, set, i), false);
}

// spectral table [t][p][c], c < nc: (level i, c) -> out[c + nc * i] (premixed: kernels.cu:524-610, per species: :3209-3259).
// One thread per (c = y + ny*x, level): the four corners and the output are contiguous in c.  Grid (chunks of c, levels, columns)
template <bool SPECIES, bool SECOND, class Src, class Tab>
__global__ void __launch_bounds__(256) k_tp_spectral(Src src, TPLaunch<Tab> q, TPSecond x) {
    const int col = blockIdx.z, i = blockIdx.y;
    if (src.skip(col)) return;
    const double* __restrict__ table = q.tab.of(col);
    for (int set = 0; set < 2; set++) {
        if (i >= q.nlev[set]) continue;
        const TPIndex k = src.at(col, set, i);
        double* out = q.out[set] + col * q.out_col + q.nc * i;
        for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < q.nc; c += (size_t)gridDim.x * blockDim.x) {
            out[c] = gather_tp(table, c, q.nc, q.nc * q.npress, k, SPECIES);
            if (SECOND && c < (size_t)x.nx)
                x.out[set][col * x.out_col + c + (size_t)x.nx * i] = gather_tp(x.tab, c, x.nx, (size_t)x.nx * q.npress, k, false);
        }
    }
}

template <class Src, class Tab>
int launch_tp_scalar(hx_context* ctx, const Src& src, const TPLaunch<Tab>& q) {
    k_tp_scalar<<<dim3(hx_cdiv(q.nlev[0] > q.nlev[1] ? q.nlev[0] : q.nlev[1], 64), q.ncol), 64, 0, ctx->stream>>>(src, q);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

template <bool SPECIES, bool SECOND, class Src, class Tab>
int launch_tp_spectral(hx_context* ctx, const Src& src, const TPLaunch<Tab>& q, const TPSecond& x = TPSecond{}) {
    const long long chunks = hx_cdiv((long long)q.nc, 256);
    const dim3 grid((unsigned)(chunks < 4096 ? chunks : 4096), q.nlev[0] > q.nlev[1] ? q.nlev[0] : q.nlev[1], q.ncol);
    k_tp_spectral<SPECIES, SECOND><<<grid, 256, 0, ctx->stream>>>(src, q, x);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

// a scalar table for all columns at computed levels (with the margin): instantiated once, in stage_interp.hip, for the stage
// API and for the kappa / c_p refresh of the batch
int launch_scalar_table(hx_context* ctx, const TPLevels& levels, bool log_t, const TPLaunch<OneTable>& q);

}  // namespace hx
