// Cloud decks built on the device (include/helios_hip.h section 4, hx_rt_add_mie_table / hx_rt_set_column_cloud_decks).
//
// Counterpart of the host's Cloud.cloud_pre_processing (helios_amd/clouds.py; reference source/clouds.py:84-253) for the
// columns of a batch:
//   k_cloud_deck_spectra  one (column, deck): the size-distribution-weighted sums over the radii of a resident Mie table at
//                         every tabulated wavelength, re-binned onto the batch's bins under the contract of
//                         tools.convert_spectrum with int_lambda = opac_interwave -- absorption and scattering in log mode,
//                         the third spectrum (the scattering-weighted sum again, the reference's sic) in linear mode
//   k_cloud_planes        every level and bin of one column: the decks' spectra times their mixing-ratio profiles, summed in
//                         deck order, and the normalised asymmetry parameter -- stored straight into the six planes
//                         hx_rt_set_column_clouds fills
// The unit is compiled with -ffp-contract=off like the rest of the library: products and sums round separately, so the planes
// are the bits numpy's np.outer accumulation gives from the same spectra.
#include "rt_fused.h"

#include <cmath>
#include <cstdint>

using namespace hx;

namespace {

// Mie wavelengths one workgroup stages per pass: CL_CHUNK intervals, i.e. CL_CHUNK + 1 points, the last one shared with the
// next pass so that every interval between two tabulated wavelengths lies inside exactly one pass
constexpr int CL_CHUNK = 1024;
constexpr int CL_BINS = 256;       // bins per workgroup, one per thread
constexpr int CL_MAX_TABLES = 256;

// first index j in [0, n) with a[j] >= v, n if there is none: np.searchsorted(a, v, side="left")
__device__ __forceinline__ int lower_bound(const double* __restrict__ a, int n, double v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// interpolant at an interface lam between the tabulated points p (at lam_p) and p + 1 (at lam_q): linear in the value, and
// linear in its logarithm.  d_hi = 0 -- the interface lies ON point p + 1 -- takes point p out: the host's f_p * 0 and f_p ** 0.
struct EdgeValue { double lin, log_a, log_s; };

__device__ __forceinline__ EdgeValue edge_value(double lam, double lam_p, double lam_q, double s_p, double s_q, double la_p,
                                                double la_q, double ls_p, double ls_q) {
    const double d_hi = lam_q - lam, d_lo = lam - lam_p, width = lam_q - lam_p;
    EdgeValue e;
    e.lin = ((d_hi == 0.0 ? 0.0 : s_p * d_hi) + s_q * d_lo) / width;
    e.log_a = ((d_hi == 0.0 ? 0.0 : d_hi * la_p) + d_lo * la_q) / width;
    e.log_s = ((d_hi == 0.0 ? 0.0 : d_hi * ls_p) + d_lo * ls_q) / width;
    return e;
}

// grid (ceil(nbin / CL_BINS), ndecks); out[deck][3][nbin] = absorption, scattering, scattering-weighted third spectrum
__global__ void __launch_bounds__(CL_BINS) k_cloud_deck_spectra(const MieTable* __restrict__ tabs, const int* __restrict__ mie_index,
                                                                const double* __restrict__ weight, int nr,
                                                                const double* __restrict__ inter, int X,
                                                                double* __restrict__ out) {
    __shared__ double s_s[CL_CHUNK + 1], s_la[CL_CHUNK + 1], s_ls[CL_CHUNK + 1];
    const int d = blockIdx.y;
    const MieTable t = tabs[mie_index[d]];
    const double* __restrict__ lam = t.lam;
    const double* __restrict__ w = weight + (size_t)d * nr;
    const int nw = t.nw;
    const int xb0 = blockIdx.x * CL_BINS, xb1 = min(X, xb0 + CL_BINS);
    const int x = xb0 + threadIdx.x;
    // the tabulated points this workgroup's bins can touch: from the one below its first interface to the first one at or
    // above its last interface
    const int jlo = max(0, lower_bound(lam, nw, inter[xb0]) - 1);
    const int jhi = min(nw - 1, lower_bound(lam, nw, inter[xb1]));

    double lo = 0.0, hi = 0.0;
    int first = 0, last = 0;
    bool inside = false;       // both interfaces within the table: everything else is 0 (the host's interface value 0)
    if (x < X) {
        lo = inter[x];
        hi = inter[x + 1];
        inside = lo >= lam[0] && hi <= lam[nw - 1];
        if (inside) {
            first = lower_bound(lam, nw, lo);    // first tabulated point >= lo
            last = lower_bound(lam, nw, hi);     // first tabulated point >= hi
        }
    }
    bool have_lo = false, finished = false;
    EdgeValue e_lo = {0.0, 0.0, 0.0};
    int next = first;                            // next tabulated point inside the bin to take in
    double prev_x = 0.0, prev_s = 0.0, prev_la = 0.0, prev_ls = 0.0;
    double acc_g = 0.0, acc_a = 0.0, acc_s = 0.0;
    double res_a = 0.0, res_s = 0.0, res_g = 0.0;

    for (int g0 = jlo; g0 < jhi; g0 += CL_CHUNK) {
        const int g1 = min(g0 + CL_CHUNK, jhi);  // last staged point
        __syncthreads();
        for (int j = threadIdx.x; j <= g1 - g0; j += CL_BINS) {
            double a = 0.0, s = 0.0;
            for (int r = 0; r < nr; r++) {       // radii in order, products and sums rounded separately
                const double wr = w[r];
                a = a + t.absorb[(size_t)r * nw + g0 + j] * wr;
                s = s + t.scat[(size_t)r * nw + g0 + j] * wr;
            }
            s_s[j] = s;
            s_la[j] = log(a);
            s_ls[j] = log(s);
        }
        __syncthreads();
        if (!inside || finished) continue;
        if (!have_lo) {
            // the lower interface between points first - 1 and first.  first = 0: the interface lies on the first tabulated
            // point and the host's index -1 wraps to the LAST point, whose value its d_hi = 0 takes out again
            const bool ready = first == 0 ? g0 == 0 : (g0 <= first - 1 && first <= g1);
            if (ready) {
                const int q = first - g0, p = first == 0 ? q : q - 1;
                e_lo = edge_value(lo, first == 0 ? lam[nw - 1] : lam[first - 1], lam[first], s_s[p], s_s[q], s_la[p], s_la[q],
                                  s_ls[p], s_ls[q]);
                have_lo = true;
                prev_x = lo; prev_s = e_lo.lin; prev_la = e_lo.log_a; prev_ls = e_lo.log_s;
            }
        }
        if (!have_lo) continue;
        // the tabulated points in [lo, hi), in order: one trapezoid each, in the value and in its logarithm
        while (next < last && next >= g0 && next <= g1) {
            const int q = next - g0;
            const double xq = lam[next], dx = xq - prev_x;
            acc_g = acc_g + (prev_s + s_s[q]) / 2.0 * dx;
            if (dx != 0.0) {                      // (a factor (y y') ** 0 of the host's product)
                acc_a = acc_a + (0.5 * dx) * (prev_la + s_la[q]);
                acc_s = acc_s + (0.5 * dx) * (prev_ls + s_ls[q]);
            }
            prev_x = xq; prev_s = s_s[q]; prev_la = s_la[q]; prev_ls = s_ls[q];
            next++;
        }
        if (next == last && g0 <= last - 1 && last <= g1) {
            const int q = last - g0, p = q - 1;
            const EdgeValue e_hi = edge_value(hi, lam[last - 1], lam[last], s_s[p], s_s[q], s_la[p], s_la[q], s_ls[p], s_ls[q]);
            if (first == last) {
                // no tabulated point inside the bin: the mean of the two interface values, geometric in log mode
                res_g = (e_lo.lin + e_hi.lin) / 2.0;
                res_a = exp(0.5 * (e_lo.log_a + e_hi.log_a));
                res_s = exp(0.5 * (e_lo.log_s + e_hi.log_s));
            } else {
                const double dx = hi - prev_x;
                acc_g = acc_g + (prev_s + e_hi.lin) / 2.0 * dx;
                if (dx != 0.0) {
                    acc_a = acc_a + (0.5 * dx) * (prev_la + e_hi.log_a);
                    acc_s = acc_s + (0.5 * dx) * (prev_ls + e_hi.log_s);
                }
                res_g = acc_g / (hi - lo);
                res_a = exp(acc_a / (hi - lo));
                res_s = exp(acc_s / (hi - lo));
            }
            if (e_lo.lin == 0.0 || e_hi.lin == 0.0) res_g = 0.0;      // an interface value 0 marks "outside" on the host
            finished = true;
        }
    }
    if (x < X) {
        double* o = out + (size_t)d * 3 * X;
        o[x] = finished ? res_a : 0.0;
        o[(size_t)X + x] = finished ? res_s : 0.0;
        o[2 * (size_t)X + x] = finished ? res_g : 0.0;
    }
}

struct PlaneSet { double *abs_lay, *sc_lay, *g0_lay, *abs_int, *sc_int, *g0_int; };

// grid (ceil((nbin + 1) / 512), nlayer [+ ninterface]); a thread owns two neighbouring bins of one level, paired so that
// their 16-byte store is aligned whatever the parity of the row's start (rows are nbin doubles apart); the level is uniform
// per workgroup, so the decks' mixing ratios arrive by scalar loads
__global__ void __launch_bounds__(256) k_cloud_planes(const double* __restrict__ spec, const double* __restrict__ f_lay,
                                                      const double* __restrict__ f_int, int nd, int X, int L, int I,
                                                      PlaneSet pl) {
    const int level = blockIdx.y;
    const bool lay = level < L;
    const int lv = lay ? level : level - L;
    const double* __restrict__ f = (lay ? f_lay : f_int) + lv;
    const int fstride = lay ? L : I;
    double* pa = (lay ? pl.abs_lay : pl.abs_int) + (size_t)lv * X;
    double* ps = (lay ? pl.sc_lay : pl.sc_int) + (size_t)lv * X;
    double* pg = (lay ? pl.g0_lay : pl.g0_int) + (size_t)lv * X;
    const int par = (int)(((uintptr_t)pa >> 3) & 1);      // the six planes share their alignment (same offset in each)
    const int x0 = 2 * (int)(blockIdx.x * blockDim.x + threadIdx.x) - par;
    if (x0 >= X) return;
    const bool v0 = x0 >= 0, v1 = x0 + 1 < X;
    const int i0 = v0 ? x0 : 0, i1 = v1 ? x0 + 1 : X - 1;
    double a0 = 0.0, a1 = 0.0, s0 = 0.0, s1 = 0.0, g0 = 0.0, g1 = 0.0;
    for (int d = 0; d < nd; d++) {        // decks in order; f * a, f * s and f * (g * s) as np.outer forms them
        const double fd = f[(size_t)d * fstride];
        const double* __restrict__ sa = spec + (size_t)d * 3 * X;
        const double* __restrict__ ss = sa + X;
        const double* __restrict__ sg = ss + X;
        a0 = a0 + fd * sa[i0];
        a1 = a1 + fd * sa[i1];
        s0 = s0 + fd * ss[i0];
        s1 = s1 + fd * ss[i1];
        g0 = g0 + fd * (sg[i0] * ss[i0]);
        g1 = g1 + fd * (sg[i1] * ss[i1]);
    }
    if (s0 > 0.0) g0 = g0 / s0;
    if (s1 > 0.0) g1 = g1 / s1;
    if (v0 && v1) {
        *reinterpret_cast<double2*>(pa + x0) = make_double2(a0, a1);
        *reinterpret_cast<double2*>(ps + x0) = make_double2(s0, s1);
        *reinterpret_cast<double2*>(pg + x0) = make_double2(g0, g1);
    } else if (v0) {
        pa[x0] = a0; ps[x0] = s0; pg[x0] = g0;
    } else if (v1) {
        pa[x0 + 1] = a1; ps[x0 + 1] = s1; pg[x0 + 1] = g1;
    }
}

template <class T>
int cl_alloc(hx_rt* rt, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess)
        return hx_fail(rt->ctx, -(int)e, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    rt->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

// events around one launch while hx_rt_profile is on; hx_rt_profile_read collects them under the kernel's name
struct CloudProf {
    hx_rt* rt;
    const char* name;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CloudProf(hx_rt* r, const char* n) : rt(r), name(n) {
        if (!rt->profiling) return;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, rt->ctx->stream);
    }
    ~CloudProf() {
        if (!rt->profiling) return;
        (void)hipEventRecord(e1, rt->ctx->stream);
        rt->prof.push_back({name, e0, e1});
    }
};

}  // namespace

extern "C" {

int hx_rt_add_mie_table(hx_rt* rt, const double* lamda_mie, int nw, const double* scat, const double* absorb, int nr,
                        int* out_index) {
    if (!rt) return HX_E_ARG;  // e.g. a call after hx_rt_destroy
    const int ntab = (int)rt->mie.size();
    if (rt->f.clouds != 1)
        return hx_fail(rt->ctx, HX_E_STATE, "hx_rt_add_mie_table: object was created with clouds = %d; it takes no Mie table",
                       rt->f.clouds);
    HX_REQUIRE(rt->ctx, lamda_mie && scat && absorb && out_index, HX_E_ARG, "null table");
    if (nw < 2 || nr < 1)
        return hx_fail(rt->ctx, HX_E_ARG, "hx_rt_add_mie_table: a table of %d wavelengths x %d radii; at least 2 x 1 are needed",
                       nw, nr);
    for (int j = 1; j < nw; j++)
        if (!(lamda_mie[j] > lamda_mie[j - 1]))
            return hx_fail(rt->ctx, HX_E_ARG, "hx_rt_add_mie_table: wavelengths are not ascending: lamda_mie[%d] = %.17g after "
                           "lamda_mie[%d] = %.17g", j, lamda_mie[j], j - 1, lamda_mie[j - 1]);
    if (ntab >= CL_MAX_TABLES)
        return hx_fail(rt->ctx, HX_E_ARG, "hx_rt_add_mie_table: the batch holds %d Mie tables already, its limit", ntab);
    if (!rt->mie_dev) {
        int rc = cl_alloc(rt, &rt->mie_dev, (size_t)CL_MAX_TABLES);
        if (rc) return rc;
    }
    MieTable t = {nullptr, nullptr, nullptr, nw, nr};
    double *lam = nullptr, *sc = nullptr, *ab = nullptr;
    int rc = cl_alloc(rt, &lam, (size_t)nw);
    if (!rc) rc = cl_alloc(rt, &sc, (size_t)nw * nr);
    if (!rc) rc = cl_alloc(rt, &ab, (size_t)nw * nr);
    if (rc) return rc;       // (what was allocated stays in rt->allocs: hx_rt_destroy frees it)
    rc |= hx_h2d(rt->ctx, lam, lamda_mie, (size_t)nw * 8);
    rc |= hx_h2d(rt->ctx, sc, scat, (size_t)nw * nr * 8);
    rc |= hx_h2d(rt->ctx, ab, absorb, (size_t)nw * nr * 8);
    if (rc) return rc;
    t.lam = lam; t.scat = sc; t.absorb = ab;
    rc = hx_h2d(rt->ctx, rt->mie_dev + ntab, &t, sizeof(t));
    if (rc) return rc;
    rt->mie.push_back(t);
    *out_index = ntab;
    return 0;
}

int hx_rt_set_column_cloud_decks(hx_rt* rt, int col, int ndecks, const int* mie_index, const double* radius_weight, int nr,
                                 const double* f_lay, const double* f_int) {
    if (!rt) return HX_E_ARG;  // e.g. a call after hx_rt_destroy
    hx_context* ctx = rt->ctx;
    const int ntab = (int)rt->mie.size();
    if (rt->f.clouds != 1)
        return hx_fail(ctx, HX_E_STATE, "hx_rt_set_column_cloud_decks: object was created with clouds = %d; it has no cloud "
                       "planes to fill", rt->f.clouds);
    HX_REQUIRE(ctx, rt->have_grid, HX_E_STATE, "the wavelength bins come first (hx_rt_set_grid)");
    if (col >= rt->C) return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: column index %d out of range, the batch has "
                                     "%d column(s)", col, rt->C);
    if (ndecks < 1) return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: %d decks; at least one is needed", ndecks);
    if (rt->cloud_ndecks && ndecks != rt->cloud_ndecks)
        return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: %d decks, but the batch was set up for %d; the number of "
                       "decks is fixed per batch", ndecks, rt->cloud_ndecks);
    HX_REQUIRE(ctx, mie_index && radius_weight && f_lay, HX_E_ARG, "null deck description");
    if (!rt->f.iso && !f_int)
        return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: f_int is NULL but the batch has iso = 0 and interface planes");
    for (int d = 0; d < ndecks; d++) {
        if (mie_index[d] < 0 || mie_index[d] >= ntab)
            return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: Mie table index %d of deck %d out of range, the batch "
                           "holds %d Mie table(s)", mie_index[d], d, ntab);
        if (rt->mie[mie_index[d]].nr != nr)
            return hx_fail(ctx, HX_E_ARG, "hx_rt_set_column_cloud_decks: %d radius weights for deck %d, but Mie table %d has %d "
                           "radii", nr, d, mie_index[d], rt->mie[mie_index[d]].nr);
    }
    const size_t X = rt->X, L = rt->L, I = rt->I, nd = ndecks;
    const bool with_int = !rt->f.iso;
    if (!rt->cloud_ndecks) {
        // deck spectra of every column, and the staging of one call: table indices, radius weights, the two profiles
        int rc = cl_alloc(rt, &rt->cloud_spec, (size_t)rt->C * nd * 3 * X);
        if (!rc) rc = cl_alloc(rt, &rt->cloud_stage, nd * ((size_t)nr + L + I));
        if (!rc) rc = cl_alloc(rt, &rt->cloud_stage_index, nd);
        if (rc) return rc;
        HX_HIP(ctx, hipMemsetAsync(rt->cloud_spec, 0, (size_t)rt->C * nd * 3 * X * 8, ctx->stream));
        rt->cloud_ndecks = ndecks;
        rt->cloud_stage_nr = nr;
    } else if (nr > rt->cloud_stage_nr) {
        int rc = cl_alloc(rt, &rt->cloud_stage, nd * ((size_t)nr + L + I));
        if (rc) return rc;
        rt->cloud_stage_nr = nr;
    }
    rt->graph_gen++;       // as every setter: captured graphs and re-created flux tiles are of before this call
    rt->solve_serial++;
    double* d_w = rt->cloud_stage;
    double* d_flay = d_w + nd * nr;
    double* d_fint = d_flay + nd * L;
    int rc = hx_h2d(ctx, rt->cloud_stage_index, mie_index, nd * sizeof(int));
    rc |= hx_h2d(ctx, d_w, radius_weight, nd * nr * 8);
    rc |= hx_h2d(ctx, d_flay, f_lay, nd * L * 8);
    if (with_int) rc |= hx_h2d(ctx, d_fint, f_int, nd * I * 8);
    if (rc) return rc;
    const int c0 = col < 0 ? 0 : col, c1 = col < 0 ? rt->C : col + 1;
    for (int c = c0; c < c1; c++) {
        double* spec = rt->cloud_spec + (size_t)c * nd * 3 * X;
        {
            CloudProf p(rt, "k_cloud_deck_spectra");
            k_cloud_deck_spectra<<<dim3(hx_cdiv(X, CL_BINS), ndecks), CL_BINS, 0, ctx->stream>>>(
                rt->mie_dev, rt->cloud_stage_index, d_w, nr, rt->interwave, (int)X, spec);
        }
        HX_LAUNCH_CHECK(ctx);
        const size_t XI = X * I;
        PlaneSet pl = {rt->cl_abs_lay + c * XI, rt->cl_sc_lay + c * XI, rt->cl_g0_lay + c * XI,
                       rt->cl_abs_int + c * XI, rt->cl_sc_int + c * XI, rt->cl_g0_int + c * XI};
        {
            CloudProf p(rt, "k_cloud_planes");
            k_cloud_planes<<<dim3(hx_cdiv(X + 1, 512), (unsigned)(L + (with_int ? I : 0))), 256, 0, ctx->stream>>>(
                spec, d_flay, d_fint, ndecks, (int)X, (int)L, (int)I, pl);
        }
        HX_LAUNCH_CHECK(ctx);
    }
    // (the staging is reused by the next call: its copies are ordered behind these launches on the stream)
    return 0;
}

}  // extern "C"
