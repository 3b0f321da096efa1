// Premixed k-tables from the on-the-fly species set (include/helios_hip.h section 5).
//
// Where every species' mixing ratio is a constant or a (T, P) table, the mix of a level is a function of (T, P) alone.  This
// unit evaluates it on a grid of (T, P) nodes with the refresh's own species loop and stores what a premixed run reads:
//
//   k_premix_nodes        per output node: every species' mixing ratio at the node's (T, P), mu over the in_mu species, the
//                         fractional indices into the species tables and the factors vmr * mass / mu -- the records
//                         k_rt_species_prep writes per level (rt_species.h)
//   k_rt_mix_species      unchanged (hx::launch_mix_species, rt_fused.hip): the table layout [t][p][x][y] is the layout it writes
//                         for a pseudo-column of L = 0 layers and I = nodes interfaces (out_level = nc * i, off = ny * x + y)
//   k_premix_scat         weighted Rayleigh table [t][p][x] (water vapour through h2o_rayleigh_cross at the node) and the mean
//                         molecular mass per node in amu
//   k_premix_cell_error   per output cell: the mix evaluated at the cell's centre (a second mixing launch with the centres as
//                         levels) against the bilinear value the premixed look-up returns there from the four corner nodes;
//                         max and mean over (x, y) of |k_table - k_otf| / k_otf
//
// The table is built in slabs of temperature rows, so that a refined table of any size fits next to the species tables; the
// finished rows go to host memory.
//
// k_premix_nodes repeats the dozen lines of k_rt_species_prep's level body instead of sharing a __device__ helper with it:
// the existing kernel's code object was to stay as it is, and both sides call the same vmr_from_table and locate_tp.
#define HX_SPECIES_DECLARATIONS_ONLY
#include "rt_species.h"
#include "hx_tool.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace hx;

struct hx_premix {
    hx_context* ctx = nullptr;
    int X = 0, Y = 0, ntemp = 0, npress = 0, S = 0, rt = 1, rp = 1, ck = 0;
    int NT = 0, NP = 0;  // output nodes
    int slab_rows = 0;   // cell rows per slab; 0: as many as fit
    bool have_grid = false, ran = false, ran_error = false;
    double *wave = nullptr, *gauss_y = nullptr, *gauss_w = nullptr, *ktemp = nullptr, *kpress = nullptr;
    struct Sp {
        double *pretab = nullptr, *scat_cross = nullptr, *vmr_tab = nullptr;
        double vmr_const = 0.0, weight = 0.0;
        int absorbing = 0, scattering = 0, is_h2o = 0, is_cia = 0, in_mu = 0;
        bool set = false;
    };
    std::vector<Sp> sp;
    std::vector<double> h_ktemp, h_kpress, outT, outP, cenT, cenP;  // output nodes and cell centres along each axis
    std::vector<double> kpoints, scat, mmm, err_max, err_mean;      // results (host)
    double timing[4] = {0, 0, 0, 0};
    hx_owned owned;
};

namespace {

struct NodeArgs {
    int n, S, ntemp, npress;
    const SpeciesDev* sp;
    const double* vmr_const;  // [S]
    const double *T, *P;      // [n]
    const double *ktemp, *kpress;
    double* vmr;  // [n][S]
    TPIndex* tp;  // [n]
    double* fac;  // [n][S]
};

__global__ void __launch_bounds__(64) k_premix_nodes(NodeArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double T = a.T[i], P = a.P[i];
    double* vmr = a.vmr + (size_t)i * a.S;
    for (int s = 0; s < a.S; s++)
        vmr[s] = a.sp[s].vmr_tab ? vmr_from_table(a.sp[s].vmr_tab, T, P, a.ktemp, a.ntemp, a.kpress, a.npress) : a.vmr_const[s];
    double num = 0.0, tot = 0.0;  // as k_rt_species_prep (host_functions.py:927-959)
    for (int s = 0; s < a.S; s++)
        if (a.sp[s].in_mu) {
            num += vmr[s] * a.sp[s].weight;
            tot += vmr[s];
        }
    const double mmm = num / tot * HX_AMU;
    a.tp[i] = locate_tp(T, P, a.ktemp, a.ntemp, a.kpress, a.npress, false, false);
    double* fac = a.fac + (size_t)i * a.S;
    for (int s = 0; s < a.S; s++) {
        const double mass = a.sp[s].weight * HX_AMU;
        fac[s] = vmr[s] * mass / mmm;
    }
}

// one thread per (node, bin); the thread of bin 0 also writes the node's mean molecular mass in amu
__global__ void __launch_bounds__(256) k_premix_scat(const SpeciesDev* __restrict__ sp, int S, int X, int n,
                                                     const double* __restrict__ T, const double* __restrict__ P,
                                                     const double* __restrict__ vmr, const double* __restrict__ wave,
                                                     double* __restrict__ scat, double* __restrict__ mmm_amu) {
    const int x = blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (x >= X || i >= n) return;
    const double* v = vmr + (size_t)i * S;
    double sum = 0.0;  // as k_rt_scat_species (add_to_mixed_scat)
    for (int s = 0; s < S; s++) {
        if (!sp[s].scattering) continue;
        const double f = v[s];
        const double sigma = sp[s].is_h2o ? h2o_rayleigh_cross(T[i], P[i], f, wave[x], sp[s].weight * HX_AMU) : sp[s].scat_cross[x];
        sum += f * sigma;
    }
    scat[(size_t)i * X + x] = sum;
    if (x == 0) {
        double num = 0.0, tot = 0.0;
        for (int s = 0; s < S; s++)
            if (sp[s].in_mu) {
                num += v[s] * sp[s].weight;
                tot += v[s];
            }
        mmm_amu[i] = num / tot;
    }
}

// One wavefront per (cell, chunk of the nc = ny * nbin entries of a node): lane l reads entries c0 + l, c0 + l + 64, ... of
// the four corner nodes and of the centre -- each load of the wavefront one 512-byte segment.  The corner blend is the premixed
// look-up's (kernels.cu:561-567, blend_tp) at the fractional indices of the centre, (t + 1/2, p + 1/2).  Partial results:
// (max, sum) per (cell, chunk), combined over the lanes by a fixed tree; k_premix_cell_error_final adds the chunks in order.
constexpr int ERR_CHUNK = 64 * 32;  // entries per wavefront

__global__ void __launch_bounds__(64) k_premix_cell_error(const double* __restrict__ nodes, const double* __restrict__ centres,
                                                          int nc, int NP, int ncell, int nchunk, double* __restrict__ part) {
    const int cell = blockIdx.x, chunk = blockIdx.y, lane = threadIdx.x;
    if (cell >= ncell || chunk >= nchunk) return;
    const int tr = cell / (NP - 1), p = cell - tr * (NP - 1);  // cell (tr, p) of the slab: corners at rows tr, tr + 1
    const double* dd = nodes + (size_t)nc * ((size_t)tr * NP + p);
    const double* ud = dd + nc;                // (t, p + 1)
    const double* du = dd + (size_t)nc * NP;   // (t + 1, p)
    const double* uu = du + nc;
    const double* ce = centres + (size_t)nc * cell;
    TPIndex k;
    k.tdown = 0; k.tup = 1; k.pdown = 0; k.pup = 1; k.t = 0.5; k.p = 0.5;
    double mx = 0.0, sm = 0.0;
    const int e1 = min(nc, (chunk + 1) * ERR_CHUNK);
    for (int e = chunk * ERR_CHUNK + lane; e < e1; e += 64) {
        const double tab = blend_tp(dd[e], ud[e], du[e], uu[e], k, false);
        const double otf = ce[e];
        const double d = fabs(tab - otf);
        const double rel = d == 0.0 ? 0.0 : d / otf;
        mx = dmax(mx, rel);
        sm += rel;
    }
    for (int d = 32; d > 0; d >>= 1) {
        mx = dmax(mx, __shfl_down(mx, d));
        sm += __shfl_down(sm, d);
    }
    if (lane == 0) {
        part[2 * ((size_t)cell * nchunk + chunk)] = mx;
        part[2 * ((size_t)cell * nchunk + chunk) + 1] = sm;
    }
}

__global__ void __launch_bounds__(64) k_premix_cell_error_final(const double* __restrict__ part, int ncell, int nchunk, int nc,
                                                                double* __restrict__ err_max, double* __restrict__ err_mean) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= ncell) return;
    double mx = 0.0, sm = 0.0;
    for (int c = 0; c < nchunk; c++) {
        mx = dmax(mx, part[2 * ((size_t)cell * nchunk + c)]);
        sm += part[2 * ((size_t)cell * nchunk + c) + 1];
    }
    err_max[cell] = mx;
    err_mean[cell] = sm / nc;
}

__global__ void __launch_bounds__(256) k_premix_table_outer(double* __restrict__ out, const double* __restrict__ kxy,
                                                            const double* __restrict__ ftp, size_t nc, size_t ntp) {
    const size_t n = nc * ntp;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x)
        out[k] = kxy[k % nc] * ftp[k / nc];
}

#define PM_ALLOC(ptr, count)                                                 \
    do {                                                                     \
        int rc_ = hx_owned_alloc(pm->ctx, pm->owned, (size_t)(count) * sizeof(*(ptr)), &(ptr)); \
        if (rc_) return rc_;                                                 \
    } while (0)

// nodes of one axis: node k * r + m lies at base[k] + (base[k + 1] - base[k]) * (m / r), in T or in log10 P; the species'
// own nodes (m = 0) are taken over as they are.  The centres of the output cells are the odd nodes of the same formula at 2 r,
// so that the centre of a cell IS the node a table refined twice as finely holds there, to the bit.
std::vector<double> axis_nodes(const std::vector<double>& base, int r, bool log_axis) {
    const int n = (int)base.size();
    std::vector<double> out((size_t)(n - 1) * r + 1);
    for (int k = 0; k < n; k++) {
        out[(size_t)k * r] = base[k];
        if (k == n - 1) break;
        for (int m = 1; m < r; m++) {
            const double f = (double)m / r;
            if (log_axis) {
                const double a = std::log10(base[k]), b = std::log10(base[k + 1]);
                out[(size_t)k * r + m] = std::pow(10.0, a + (b - a) * f);
            } else {
                out[(size_t)k * r + m] = base[k] + (base[k + 1] - base[k]) * f;
            }
        }
    }
    return out;
}

struct Timer {
    hx_context* ctx;
    double* acc;
    Timer(hx_context* c, double* a) : ctx(c), acc(a) { (void)hx_timer_start(ctx); }
    ~Timer() {
        double ms = 0.0;
        if (hx_timer_stop_ms(ctx, &ms) == 0) *acc += ms;
    }
};

}  // namespace

extern "C" {

int hx_premix_create(hx_context* ctx, int nbin, int ny, int ntemp, int npress, int nspecies, int refine_t, int refine_p,
                     int correlated_k, hx_premix** out_pm) {
    if (!ctx || !out_pm) return HX_E_ARG;
    *out_pm = nullptr;
    HX_REQUIRE(ctx, nbin >= 1 && ny >= 1 && ntemp >= 2 && npress >= 2 && nspecies >= 1, HX_E_ARG,
               "needs nbin, ny, nspecies >= 1 and at least two nodes in T and in P");
    HX_REQUIRE(ctx, refine_t >= 1 && refine_p >= 1, HX_E_ARG, "refinement factors are integers >= 1");
    HX_REQUIRE(ctx, ny <= ro::NY, HX_E_UNSUPPORTED, "on-the-fly mixing holds at most 20 Gauss points");
    const long long NT = (long long)(ntemp - 1) * refine_t + 1, NP = (long long)(npress - 1) * refine_p + 1;
    HX_REQUIRE(ctx, NT * NP < (1ll << 24) && (long long)nbin * ny < (1ll << 30), HX_E_ARG, "table too large");
    hx_premix* pm = new hx_premix();
    pm->ctx = ctx;
    pm->X = nbin; pm->Y = ny; pm->ntemp = ntemp; pm->npress = npress; pm->S = nspecies;
    pm->rt = refine_t; pm->rp = refine_p; pm->ck = correlated_k ? 1 : 0;
    pm->NT = (int)NT; pm->NP = (int)NP;
    pm->sp.resize(nspecies);
    *out_pm = pm;
    return 0;
}

int hx_premix_destroy(hx_premix* pm) {
    if (!pm) return 0;
    (void)hx_sync(pm->ctx);
    hx_owned_free_all(pm->ctx, pm->owned);
    delete pm;
    return 0;
}

int hx_premix_set_grid(hx_premix* pm, const double* wave, const double* gauss_y, const double* gauss_w, const double* ktemp,
                       const double* kpress) {
    if (!pm) return HX_E_ARG;
    hx_context* ctx = pm->ctx;
    HX_REQUIRE(ctx, wave && gauss_y && gauss_w && ktemp && kpress, HX_E_ARG, "null grid array");
    // the premixed look-up (and locate_tp here) takes the nodes as uniform in T and in log10 P
    for (int k = 0; k < pm->ntemp; k++) {
        const double want = ktemp[0] + (ktemp[pm->ntemp - 1] - ktemp[0]) * k / (pm->ntemp - 1.0);
        HX_REQUIRE(ctx, std::fabs(ktemp[k] - want) <= 1e-9 * std::fabs(want), HX_E_ARG, "temperature nodes are not uniform");
    }
    for (int k = 0; k < pm->npress; k++) {
        HX_REQUIRE(ctx, kpress[k] > 0.0, HX_E_ARG, "pressure nodes must be positive");
        const double l0 = std::log10(kpress[0]), l1 = std::log10(kpress[pm->npress - 1]);
        const double want = l0 + (l1 - l0) * k / (pm->npress - 1.0);
        HX_REQUIRE(ctx, std::fabs(std::log10(kpress[k]) - want) <= 1e-9 * std::max(1.0, std::fabs(want)), HX_E_ARG,
                   "pressure nodes are not uniform in log10 P");
    }
    if (!pm->wave) {
        PM_ALLOC(pm->wave, pm->X); PM_ALLOC(pm->gauss_y, pm->Y); PM_ALLOC(pm->gauss_w, pm->Y);
        PM_ALLOC(pm->ktemp, pm->ntemp); PM_ALLOC(pm->kpress, pm->npress);
    }
    int rc = hx_h2d(ctx, pm->wave, wave, pm->X * 8);
    if (!rc) rc = hx_h2d(ctx, pm->gauss_y, gauss_y, pm->Y * 8);
    if (!rc) rc = hx_h2d(ctx, pm->gauss_w, gauss_w, pm->Y * 8);
    if (!rc) rc = hx_h2d(ctx, pm->ktemp, ktemp, pm->ntemp * 8);
    if (!rc) rc = hx_h2d(ctx, pm->kpress, kpress, pm->npress * 8);
    if (rc) return rc;
    pm->h_ktemp.assign(ktemp, ktemp + pm->ntemp);
    pm->h_kpress.assign(kpress, kpress + pm->npress);
    pm->outT = axis_nodes(pm->h_ktemp, pm->rt, false);
    pm->outP = axis_nodes(pm->h_kpress, pm->rp, true);
    const std::vector<double> t2 = axis_nodes(pm->h_ktemp, 2 * pm->rt, false), p2 = axis_nodes(pm->h_kpress, 2 * pm->rp, true);
    pm->cenT.resize(pm->NT - 1);
    pm->cenP.resize(pm->NP - 1);
    for (int k = 0; k + 1 < pm->NT; k++) pm->cenT[k] = t2[2 * k + 1];
    for (int k = 0; k + 1 < pm->NP; k++) pm->cenP[k] = p2[2 * k + 1];
    pm->have_grid = true;
    pm->ran = false;
    return 0;
}

int hx_premix_set_species_vmr(hx_premix* pm, int s, const double* vmr_table, double vmr_const) {
    if (!pm) return HX_E_ARG;
    HX_REQUIRE(pm->ctx, s >= 0 && s < pm->S, HX_E_ARG, "species index out of range");
    hx_premix::Sp& sp = pm->sp[s];
    const size_t ntp = (size_t)pm->ntemp * pm->npress;
    if (vmr_table) {
        if (!sp.vmr_tab) PM_ALLOC(sp.vmr_tab, ntp);
        int rc = hx_h2d(pm->ctx, sp.vmr_tab, vmr_table, ntp * 8);
        if (rc) return rc;
    } else if (sp.vmr_tab) {
        int rc = hx_owned_free(pm->ctx, pm->owned, sp.vmr_tab);
        if (rc) return rc;
        sp.vmr_tab = nullptr;
    }
    sp.vmr_const = vmr_const;
    pm->ran = false;
    return 0;
}

int hx_premix_set_species(hx_premix* pm, int s, const double* pretab, const double* scat_cross, const double* vmr_table,
                          double vmr_const, double weight, int absorbing, int scattering, int is_h2o, int is_cia, int in_mu) {
    if (!pm) return HX_E_ARG;
    hx_context* ctx = pm->ctx;
    HX_REQUIRE(ctx, s >= 0 && s < pm->S, HX_E_ARG, "species index out of range");
    HX_REQUIRE(ctx, !scattering || is_h2o || scat_cross, HX_E_ARG, "a scattering species other than H2O needs its cross-sections");
    hx_premix::Sp& sp = pm->sp[s];
    const size_t n = (size_t)pm->ntemp * pm->npress * pm->X * pm->Y;
    if (pretab) {
        if (!sp.pretab) PM_ALLOC(sp.pretab, n);
        int rc = hx_h2d(ctx, sp.pretab, pretab, n * 8);
        if (rc) return rc;
    }
    if (scat_cross) {
        if (!sp.scat_cross) PM_ALLOC(sp.scat_cross, pm->X);
        int rc = hx_h2d(ctx, sp.scat_cross, scat_cross, pm->X * 8);
        if (rc) return rc;
    }
    sp.weight = weight;
    sp.absorbing = absorbing ? 1 : 0; sp.scattering = scattering ? 1 : 0;
    sp.is_h2o = is_h2o ? 1 : 0; sp.is_cia = is_cia ? 1 : 0; sp.in_mu = in_mu ? 1 : 0;
    sp.set = true;
    return hx_premix_set_species_vmr(pm, s, vmr_table, vmr_const);
}

int hx_premix_set_species_separable(hx_premix* pm, int s, const double* kxy, const double* ftp) {
    if (!pm) return HX_E_ARG;
    hx_context* ctx = pm->ctx;
    HX_REQUIRE(ctx, s >= 0 && s < pm->S && kxy && ftp, HX_E_ARG, "species index out of range or null factor");
    hx_premix::Sp& sp = pm->sp[s];
    const size_t nc = (size_t)pm->X * pm->Y, ntp = (size_t)pm->ntemp * pm->npress;
    if (!sp.pretab) PM_ALLOC(sp.pretab, nc * ntp);
    double *d_kxy = nullptr, *d_ftp = nullptr;
    int rc = hx_alloc(ctx, nc * 8, (void**)&d_kxy);
    if (!rc) rc = hx_alloc(ctx, ntp * 8, (void**)&d_ftp);
    if (!rc) rc = hx_h2d(ctx, d_kxy, kxy, nc * 8);
    if (!rc) rc = hx_h2d(ctx, d_ftp, ftp, ntp * 8);
    if (!rc) {
        const int grid = (int)std::min<size_t>((nc * ntp + 255) / 256, 65536);
        k_premix_table_outer<<<grid, 256, 0, ctx->stream>>>(sp.pretab, d_kxy, d_ftp, nc, ntp);
        rc = hipGetLastError() == hipSuccess ? 0 : hx_fail(ctx, HX_E_ARG, "k_premix_table_outer launch failed");
    }
    (void)hx_free(ctx, d_kxy);  // (waits for the stream)
    (void)hx_free(ctx, d_ftp);
    pm->ran = false;
    return rc;
}

int hx_premix_set_slab_rows(hx_premix* pm, int rows) {
    if (!pm || rows < 0) return HX_E_ARG;
    pm->slab_rows = rows;
    return 0;
}

int hx_premix_run(hx_premix* pm, int cell_error) {
    if (!pm) return HX_E_ARG;
    hx_context* ctx = pm->ctx;
    HX_REQUIRE(ctx, pm->have_grid, HX_E_STATE, "set the grid first");
    const int X = pm->X, Y = pm->Y, S = pm->S, NT = pm->NT, NP = pm->NP;
    const size_t nc = (size_t)X * Y;
    std::vector<SpeciesDev> sd(S);
    std::vector<double> vconst(S);
    std::vector<int> abs;
    bool any_ro = false;
    for (int s = 0; s < S; s++) {
        const hx_premix::Sp& sp = pm->sp[s];
        HX_REQUIRE(ctx, sp.set, HX_E_STATE, "a species was not set");
        HX_REQUIRE(ctx, !sp.absorbing || sp.pretab, HX_E_STATE, "an absorbing species has no opacity table");
        // random overlap unless CIA or one Gauss point per bin, as the refresh chooses it (rt_fused.hip, upload_species_table)
        const int ro_flag = (!pm->ck && !sp.is_cia && Y != 1) ? 1 : 0;
        sd[s] = SpeciesDev{sp.absorbing ? sp.pretab : nullptr, sp.scat_cross, sp.vmr_tab, sp.weight, sp.absorbing, sp.scattering,
                           sp.is_h2o, ro_flag, sp.in_mu, 0};
        vconst[s] = sp.vmr_const;
        if (sp.absorbing) {
            abs.push_back(s);
            any_ro = any_ro || ro_flag;
        }
    }
    HX_REQUIRE(ctx, !abs.empty() && abs[0] == 0, HX_E_ARG, "the first species must absorb (it starts the mix)");
    if (any_ro && Y > ro::NY) return hx_fail(ctx, HX_E_RO_NY, "random-overlap mixing needs ny == 20 or 1 (got %d)", Y);

    // slabs: R cell rows = R + 1 rows of nodes, next to R rows of cell centres when the error map is asked for
    const size_t row_bytes = (size_t)NP * nc * 8, cen_row_bytes = cell_error ? (size_t)(NP - 1) * nc * 8 : 0;
    int R = pm->slab_rows;
    if (R <= 0) {
        size_t free_b = 0, total_b = 0;
        int rc = hx_mem_info(ctx, &free_b, &total_b);
        if (rc) return rc;
        const size_t budget = std::min<size_t>(free_b / 2, (size_t)8 << 30);
        HX_REQUIRE(ctx, budget >= 2 * row_bytes + cen_row_bytes, HX_E_UNSUPPORTED,
                   "no device memory for two rows of nodes next to the species tables");
        R = (int)std::min<size_t>((budget - row_bytes) / (row_bytes + cen_row_bytes), (size_t)NT - 1);
    }
    R = std::max(1, std::min(R, NT - 1));
    const int slab_nodes = (R + 1) * NP, slab_cells = R * (NP - 1);
    const int nrec = std::max(slab_nodes, slab_cells);
    const int nchunk = (int)((nc + ERR_CHUNK - 1) / ERR_CHUNK);

    SpeciesDev* d_sp = nullptr;
    int *d_abs = nullptr, *d_done = nullptr;
    double *d_vconst = nullptr, *d_T = nullptr, *d_P = nullptr, *d_vmr = nullptr, *d_fac = nullptr, *d_nodes = nullptr,
           *d_cen = nullptr, *d_scat = nullptr, *d_mmm = nullptr, *d_part = nullptr, *d_emax = nullptr, *d_emean = nullptr;
    TPIndex* d_tp = nullptr;
    std::vector<void*> tmp;
    auto grab = [&](void** p, size_t bytes) {
        int rc = hx_alloc(ctx, bytes, p);
        if (!rc) tmp.push_back(*p);
        return rc;
    };
    auto release = [&]() {
        (void)hx_sync(ctx);
        for (void* p : tmp) (void)hipFree(p);
        tmp.clear();
    };
    int rc = 0;
#define PM_TRY(expr)          \
    do {                      \
        rc = (expr);          \
        if (rc) {             \
            release();        \
            return rc;        \
        }                     \
    } while (0)
    PM_TRY(grab((void**)&d_sp, S * sizeof(SpeciesDev)));
    PM_TRY(grab((void**)&d_abs, abs.size() * sizeof(int)));
    PM_TRY(grab((void**)&d_done, sizeof(int)));
    PM_TRY(grab((void**)&d_vconst, S * 8));
    PM_TRY(grab((void**)&d_T, (size_t)nrec * 8));
    PM_TRY(grab((void**)&d_P, (size_t)nrec * 8));
    PM_TRY(grab((void**)&d_vmr, (size_t)nrec * S * 8));
    PM_TRY(grab((void**)&d_fac, (size_t)nrec * S * 8));
    PM_TRY(grab((void**)&d_tp, (size_t)nrec * sizeof(TPIndex)));
    PM_TRY(grab((void**)&d_nodes, (size_t)slab_nodes * nc * 8));
    PM_TRY(grab((void**)&d_scat, (size_t)slab_nodes * X * 8));
    PM_TRY(grab((void**)&d_mmm, (size_t)slab_nodes * 8));
    if (cell_error) {
        PM_TRY(grab((void**)&d_cen, (size_t)slab_cells * nc * 8));
        PM_TRY(grab((void**)&d_part, (size_t)slab_cells * nchunk * 16));
        PM_TRY(grab((void**)&d_emax, (size_t)slab_cells * 8));
        PM_TRY(grab((void**)&d_emean, (size_t)slab_cells * 8));
    }
    PM_TRY(hx_h2d(ctx, d_sp, sd.data(), S * sizeof(SpeciesDev)));
    PM_TRY(hx_h2d(ctx, d_abs, abs.data(), abs.size() * sizeof(int)));
    PM_TRY(hx_h2d(ctx, d_vconst, vconst.data(), S * 8));
    PM_TRY(hx_memset0(ctx, d_done, sizeof(int)));

    try {
        pm->kpoints.assign((size_t)NT * NP * nc, 0.0);
        pm->scat.assign((size_t)NT * NP * X, 0.0);
        pm->mmm.assign((size_t)NT * NP, 0.0);
        pm->err_max.assign(cell_error ? (size_t)(NT - 1) * (NP - 1) : 0, 0.0);
        pm->err_mean.assign(pm->err_max.size(), 0.0);
    } catch (...) {
        release();
        return hx_fail(ctx, HX_E_ARG, "no host memory for the table");
    }
    for (double& t : pm->timing) t = 0.0;

    // records + species loop of n points (T, P) into `out` ([n][nc]); node records stay in d_vmr for the Rayleigh table
    std::vector<double> hT(nrec), hP(nrec);
    auto mix_points = [&](int n, double* out, double* t_nodes, double* t_mix) -> int {
        int r = hx_h2d(ctx, d_T, hT.data(), (size_t)n * 8);
        if (!r) r = hx_h2d(ctx, d_P, hP.data(), (size_t)n * 8);
        if (r) return r;
        {
            Timer tm(ctx, t_nodes);
            NodeArgs na{n, S, pm->ntemp, pm->npress, d_sp, d_vconst, d_T, d_P, pm->ktemp, pm->kpress, d_vmr, d_tp, d_fac};
            k_premix_nodes<<<hx_cdiv(n, 64), 64, 0, ctx->stream>>>(na);
            HX_LAUNCH_CHECK(ctx);
        }
        MixArgs m = {};
        m.X = X; m.Y = Y; m.L = 0; m.I = n; m.C = 1; m.S = S;
        m.ntemp = pm->ntemp; m.npress = pm->npress;
        m.sp = d_sp;
        m.ktemp = pm->ktemp; m.kpress = pm->kpress; m.gauss_w = pm->gauss_w; m.gauss_y = pm->gauss_y; m.wave = pm->wave;
        m.tp_lay = d_tp; m.tp_int = d_tp; m.fac_lay = d_fac; m.fac_int = d_fac;
        m.opac_wg_lay = out; m.opac_wg_int = out;
        m.done = d_done; m.diag = ctx->diag;
        Timer tm(ctx, t_mix);
        return launch_mix_species(ctx, m, d_abs, (int)abs.size(), any_ro);
    };

    for (int r0 = 0; r0 < NT - 1; r0 += R) {
        const int Rc = std::min(R, NT - 1 - r0);   // cell rows of this slab; node rows r0 .. r0 + Rc
        const int first = r0 == 0 ? 0 : 1;         // the slab's first row of nodes is the last one of the slab before
        if (first) PM_TRY(hx_d2d(ctx, d_nodes, d_nodes + (size_t)R * NP * nc, row_bytes));
        const int nrows = Rc + 1 - first, n = nrows * NP;
        for (int k = 0; k < n; k++) {
            hT[k] = pm->outT[r0 + first + k / NP];
            hP[k] = pm->outP[k % NP];
        }
        double* out = d_nodes + (size_t)first * NP * nc;
        PM_TRY(mix_points(n, out, &pm->timing[0], &pm->timing[1]));
        {
            Timer tm(ctx, &pm->timing[2]);
            k_premix_scat<<<dim3(n, hx_cdiv(X, 256)), 256, 0, ctx->stream>>>(d_sp, S, X, n, d_T, d_P, d_vmr, pm->wave, d_scat, d_mmm);
            if (hipGetLastError() != hipSuccess) PM_TRY(hx_fail(ctx, HX_E_ARG, "k_premix_scat launch failed"));
        }
        const size_t node0 = (size_t)(r0 + first) * NP;
        PM_TRY(hx_d2h(ctx, pm->kpoints.data() + node0 * nc, out, (size_t)n * nc * 8));
        PM_TRY(hx_d2h(ctx, pm->scat.data() + node0 * X, d_scat, (size_t)n * X * 8));
        PM_TRY(hx_d2h(ctx, pm->mmm.data() + node0, d_mmm, (size_t)n * 8));
        if (cell_error) {
            const int ncell = Rc * (NP - 1);
            for (int k = 0; k < ncell; k++) {
                hT[k] = pm->cenT[r0 + k / (NP - 1)];
                hP[k] = pm->cenP[k % (NP - 1)];
            }
            PM_TRY(mix_points(ncell, d_cen, &pm->timing[3], &pm->timing[3]));
            {
                Timer tm(ctx, &pm->timing[3]);
                k_premix_cell_error<<<dim3(ncell, nchunk), 64, 0, ctx->stream>>>(d_nodes, d_cen, (int)nc, NP, ncell, nchunk, d_part);
                k_premix_cell_error_final<<<hx_cdiv(ncell, 64), 64, 0, ctx->stream>>>(d_part, ncell, nchunk, (int)nc, d_emax, d_emean);
                if (hipGetLastError() != hipSuccess) PM_TRY(hx_fail(ctx, HX_E_ARG, "k_premix_cell_error launch failed"));
            }
            PM_TRY(hx_d2h(ctx, pm->err_max.data() + (size_t)r0 * (NP - 1), d_emax, (size_t)ncell * 8));
            PM_TRY(hx_d2h(ctx, pm->err_mean.data() + (size_t)r0 * (NP - 1), d_emean, (size_t)ncell * 8));
        }
    }
#undef PM_TRY
    release();
    pm->ran = true;
    pm->ran_error = cell_error != 0;
    return 0;
}

int hx_premix_get(hx_premix* pm, const char* name, void* out, size_t out_bytes) {
    if (!pm || !name || !out) return HX_E_ARG;
    hx_context* ctx = pm->ctx;
    const int32_t dims[2] = {pm->NT, pm->NP};
    const char* first = "set the grid and run the premix first";
    const char *no_grid = pm->have_grid ? nullptr : first, *no_run = pm->ran ? nullptr : first;
    const char* no_error = no_run ? no_run : pm->ran_error ? nullptr : "the last run did not build the cell-error map";
    const hx_result rows[] = {
        {"dims", dims, sizeof dims, false, nullptr},
        {"timing_ms", pm->timing, sizeof pm->timing, false, no_grid},
        {"temperatures", pm->outT.data(), pm->outT.size() * 8, false, no_grid},
        {"pressures", pm->outP.data(), pm->outP.size() * 8, false, no_grid},
        {"kpoints", pm->kpoints.data(), pm->kpoints.size() * 8, false, no_run},
        {"scat_cross", pm->scat.data(), pm->scat.size() * 8, false, no_run},
        {"meanmolmass", pm->mmm.data(), pm->mmm.size() * 8, false, no_run},
        {"cell_error_max", pm->err_max.data(), pm->err_max.size() * 8, false, no_error},
        {"cell_error_mean", pm->err_mean.data(), pm->err_mean.size() * 8, false, no_error},
    };
    return hx_get_result(ctx, __func__, rows, sizeof rows / sizeof rows[0], name, out, out_bytes);
}

}  // extern "C"
