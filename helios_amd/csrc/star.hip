// Stellar spectra from model grids, re-binned onto the opacity grid (include/helios_hip.h section 8; the contract and the host
// side are helios_amd/star.py).
//
//   k_star_blend        S stars at once: the weighted sum of up to eight resident fp32 corner spectra, fp64, in the term order
//                       the host hands over (the reference's branch for that star)
//   k_star_planck_bins  pi x the 199-term analytic Planck integral over every bin, per star temperature, every term without
//                       the cancellation of its closed form at small limits
//   k_star_rebin_*      interface interpolants and the trapezoids of the points inside a bin: bins of up to ST_NARROW points one
//                       thread each in the reference's own order, longer ones one workgroup each in chunks staged through LDS and
//                       summed by a tree whose shape the chunk length fixes
#include "hx_tool.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_PER_THREAD = 4;       // consecutive points of one thread in k_star_blend: one 16-byte load per corner
constexpr int ST_NARROW = 16;          // bins of up to this many points are summed by one thread
constexpr int ST_MIN_CHUNK = 64, ST_MAX_CHUNK = 2048;
constexpr int ST_TERMS = 199;
constexpr double ST_GAMMA_SPLIT = 2.0;    // star.py: GAMMA_SPLIT, GAMMA_TERMS
constexpr int ST_GAMMA_TERMS = 26;
constexpr int ST_MAX_CORNERS = 8;

struct StStar {
    int nterms;                        // 0: the flux was put as it is (hx_star_put_flux)
    int slot[ST_MAX_CORNERS];
    int pad_;
    double w[ST_MAX_CORNERS][3];       // a term is ((f * w0) * w1) * w2; factors its branch does not have are 1
    double div;
};

struct StGrid {
    const double* lam;                 // [N] ascending
    const double* inter;               // [nbin + 1]
    const int* pbot;                   // [nbin + 1] number of tabulated wavelengths below the interface, less one
    const int* state;                  // [nbin + 1] 0: outside the table, the interface value stays 0
    const double* flux;                // [S][npad]
    const double* planck;              // [S][nbin]
    double* out;                       // [S][nbin]
    size_t npad;
    int N, nbin;
};

__global__ __launch_bounds__(ST_THREADS) void k_star_blend(const float* __restrict__ corners, const StStar* __restrict__ stars,
                                                           double* __restrict__ flux, size_t npad) {
    const StStar& d = stars[blockIdx.y];
    const int nterms = d.nterms;
    if (nterms == 0) return;
    const size_t i = ((size_t)blockIdx.x * ST_THREADS + threadIdx.x) * ST_PER_THREAD;
    if (i >= npad) return;             // npad is a multiple of ST_PER_THREAD: a thread's four points are inside or outside
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int k = 0; k < nterms; k++) {
        const float4 v = *reinterpret_cast<const float4*>(corners + (size_t)d.slot[k] * npad + i);
        const double w0 = d.w[k][0], w1 = d.w[k][1], w2 = d.w[k][2];
        const double t0 = (double)v.x * w0 * w1 * w2, t1 = (double)v.y * w0 * w1 * w2;
        const double t2 = (double)v.z * w0 * w1 * w2, t3 = (double)v.w * w0 * w1 * w2;
        if (k == 0) { a0 = t0; a1 = t1; a2 = t2; a3 = t3; }
        else { a0 += t0; a1 += t1; a2 += t2; a3 += t3; }
    }
    const double div = d.div;
    double2* o = reinterpret_cast<double2*>(flux + (size_t)blockIdx.y * npad + i);
    o[0] = make_double2(a0 / div, a1 / div);
    o[1] = make_double2(a2 / div, a3 / div);
}

// int_0^x t^3 e^-t dt for x <= ST_GAMMA_SPLIT by x^4 e^-x sum_k x^k / (4 * 5 * ... * (4 + k)): positive terms only
__device__ __forceinline__ double st_lower_gamma4(double x) {
    double s = 1.0;
#pragma unroll
    for (int k = ST_GAMMA_TERMS; k >= 1; k--) s = 1.0 + x / (4.0 + (double)k) * s;
    const double x2 = x * x;
    return x2 * x2 * exp(-x) * (s / 4.0);
}

// int_x^inf t^3 e^-t dt in the reference's closed form, or 6 less the integral from 0 below the split
__device__ __forceinline__ double st_upper_gamma4(double x) {
    if (x < ST_GAMMA_SPLIT) return 6.0 - st_lower_gamma4(x);
    return exp(-x) * (x * x * x + 3.0 * (x * x) + 6.0 * x + 6.0);
}

// Term n of the reference's series is int t^3 e^-t dt between n y_top and n y_bot, over n^4.  The reference takes the closed
// form at both limits; for small limits both are 6 less a little and the difference keeps few digits, so limits below the
// split go through the lower incomplete gamma function here (helios_amd/star.py, planck_term: the same arithmetic).
// temp_d[2 s] the temperature (0: no extrapolation, the values are 0), temp_d[2 s + 1] the prefactor 2 (k/h)^3 k T^4 / c^2 as the
// host forms it; hc and kb are the host's constants
__global__ __launch_bounds__(ST_THREADS) void k_star_planck_bins(const double* __restrict__ inter, const double* __restrict__ temp_d,
                                                                 double* __restrict__ planck, int nbin, double hc, double kb) {
    const int x = blockIdx.x * ST_THREADS + threadIdx.x, s = blockIdx.y;
    if (x >= nbin) return;
    const double T = temp_d[2 * s], d = temp_d[2 * s + 1];
    if (!(T > 0.0)) { planck[(size_t)s * nbin + x] = 0.0; return; }
    const double lo = inter[x], hi = inter[x + 1];
    const double yt = hc / (hi * kb * T), yb = hc / (lo * kb * T);
    double result = 0.0;
    for (int n = 1; n <= ST_TERMS; n++) {
        const double n1 = (double)n, n2 = n1 * n1, n4 = n2 * n2;      // exact: 199^4 < 2^53
        const double a = n1 * yt, b = n1 * yb;
        const double term = (a < ST_GAMMA_SPLIT && b < ST_GAMMA_SPLIT) ? st_lower_gamma4(b) - st_lower_gamma4(a)
                                                                       : st_upper_gamma4(a) - st_upper_gamma4(b);
        result += term / n4;
    }
    result *= d / (hi - lo);
    planck[(size_t)s * nbin + x] = HX_PI * result;
}

// the linear interpolant at interface i; the index -1 of an interface on the first tabulated wavelength wraps to the last point
__device__ __forceinline__ double st_interface(const StGrid& G, const double* __restrict__ f, int i) {
    if (!G.state[i]) return 0.0;
    const int pb = G.pbot[i];
    const int a = pb < 0 ? pb + G.N : pb, b = pb + 1;
    const double x = G.inter[i];
    const double v = f[a] * (G.lam[b] - x) + f[b] * (x - G.lam[a]);
    return v / (G.lam[b] - G.lam[a]);
}

__global__ __launch_bounds__(ST_THREADS) void k_star_rebin_narrow(StGrid G) {
    const int x = blockIdx.x * ST_THREADS + threadIdx.x, s = blockIdx.y;
    if (x >= G.nbin) return;
    if (G.state[x] && G.state[x + 1] && G.pbot[x + 1] - G.pbot[x] > ST_NARROW) return;      // k_star_rebin_wide's
    const double* __restrict__ f = G.flux + (size_t)s * G.npad;
    const double* __restrict__ l = G.lam;
    const size_t o = (size_t)s * G.nbin + x;
    const double Fi = st_interface(G, f, x), Fj = st_interface(G, f, x + 1);
    if (Fi == 0.0 || Fj == 0.0) { G.out[o] = G.planck[o]; return; }
    const int ps = G.pbot[x] + 1, pe = G.pbot[x + 1] + 1, n = pe - ps;
    if (n <= 0) { G.out[o] = (Fi + Fj) / 2.0; return; }
    const double xi = G.inter[x], xj = G.inter[x + 1];
    double acc = (Fi + f[ps]) / 2.0 * (l[ps] - xi);
    for (int p = ps + 1; p < pe; p++) acc += (f[p - 1] + f[p]) / 2.0 * (l[p] - l[p - 1]);
    acc += (f[pe - 1] + Fj) / 2.0 * (xj - l[pe - 1]);
    G.out[o] = acc / (xj - xi);
}

// one workgroup per (bin of more than ST_NARROW points, star).  Node 0 is the lower interface, nodes 1 .. n the points inside, node
// n + 1 the upper interface; term j is the trapezoid between nodes j and j + 1.  `chunk` terms at a time: their nodes go to LDS, the
// terms to a zero-padded array of `chunk` slots that a tree halves down to one; the chunks' sums add up in order
__global__ __launch_bounds__(ST_THREADS) void k_star_rebin_wide(StGrid G, const int* __restrict__ wide, int chunk) {
    extern __shared__ double st_lds[];
    double* sL = st_lds;                       // [chunk + 1]
    double* sF = st_lds + (chunk + 1);         // [chunk + 1]
    double* sT = st_lds + 2 * (chunk + 1);     // [chunk]
    const int x = wide[blockIdx.x], s = blockIdx.y, tid = threadIdx.x;
    const double* __restrict__ f = G.flux + (size_t)s * G.npad;
    const double* __restrict__ l = G.lam;
    const size_t o = (size_t)s * G.nbin + x;
    const double Fi = st_interface(G, f, x), Fj = st_interface(G, f, x + 1);
    if (Fi == 0.0 || Fj == 0.0) {              // the same in every thread
        if (tid == 0) G.out[o] = G.planck[o];
        return;
    }
    const int ps = G.pbot[x] + 1, n = G.pbot[x + 1] + 1 - ps, nterms = n + 1;
    const double xi = G.inter[x], xj = G.inter[x + 1];
    double total = 0.0;
    for (int base = 0; base < nterms; base += chunk) {
        const int cnt = min(chunk, nterms - base);
        for (int k = tid; k <= cnt; k += ST_THREADS) {
            const int node = base + k;
            double lv, fv;
            if (node == 0) { lv = xi; fv = Fi; }
            else if (node == n + 1) { lv = xj; fv = Fj; }
            else { lv = l[ps + node - 1]; fv = f[ps + node - 1]; }
            sL[k] = lv; sF[k] = fv;
        }
        __syncthreads();
        for (int k = tid; k < chunk; k += ST_THREADS)
            sT[k] = k < cnt ? (sF[k] + sF[k + 1]) / 2.0 * (sL[k + 1] - sL[k]) : 0.0;
        __syncthreads();
        for (int stride = chunk >> 1; stride >= 1; stride >>= 1) {
            for (int k = tid; k < stride; k += ST_THREADS) sT[k] += sT[k + stride];
            __syncthreads();
        }
        total += sT[0];
        __syncthreads();
    }
    if (tid == 0) G.out[o] = total / (xj - xi);
}

}  // namespace

struct hx_star {
    hx_context* ctx;
    int N, ncorner, nstar, nbin, chunk, nwide, nnarrow;
    size_t npad;
    float* corners;
    double *lam, *inter, *flux, *planck, *out, *temp_d;
    int *pbot, *state, *wide;
    StStar* stars;
    std::vector<StStar> h_stars;
    std::vector<char> have_corner, have_star;
    bool have_grid;
    hx_owned owned;
    hx_stream_timer timer[3];          // around the blend, the Planck values and the re-binning of the last run
    double timing[4];      // ms in k_star_blend, in k_star_planck_bins, in the re-binning kernels; runs
};

static int st_settle(hx_star* st) {
    int rc = 0;
    for (int k = 0; k < 3 && !rc; k++) rc = hx_stream_timer_settle(st->ctx, st->timer[k], &st->timing[k]);
    return rc;
}

extern "C" {

int hx_star_create(hx_context* ctx, int n_points, int n_corners, int n_stars, int n_bins, int chunk, hx_star** out_st) {
    if (!ctx || !out_st) return HX_E_ARG;
    HX_REQUIRE(ctx, n_points >= 2 && n_points <= (1 << 28), HX_E_ARG, "2 ... 2^28 tabulated wavelengths");
    HX_REQUIRE(ctx, n_corners >= 0 && n_corners <= 65535, HX_E_ARG, "0 ... 65535 corner spectra");
    HX_REQUIRE(ctx, n_stars >= 1 && n_stars <= 65535 && n_bins >= 1, HX_E_ARG, "1 ... 65535 stars, at least one bin");
    HX_REQUIRE(ctx, chunk >= ST_MIN_CHUNK && chunk <= ST_MAX_CHUNK && (chunk & (chunk - 1)) == 0, HX_E_ARG,
               "the staging chunk is a power of two of 64 ... 2048 trapezoids");
    hx_star* st = new (std::nothrow) hx_star();
    if (!st) return hx_fail(ctx, HX_E_ARG, "no host memory");
    st->ctx = ctx;
    st->N = n_points; st->ncorner = n_corners; st->nstar = n_stars; st->nbin = n_bins; st->chunk = chunk;
    st->npad = ((size_t)n_points + ST_PER_THREAD - 1) / ST_PER_THREAD * ST_PER_THREAD;
    st->h_stars.assign(n_stars, StStar());
    st->have_corner.assign(n_corners, 0);
    st->have_star.assign(n_stars, 0);
    const size_t nb = (size_t)n_bins, ns = (size_t)n_stars;
    int rc = hx_owned_alloc(ctx, st->owned, st->npad * 8, &st->lam);
    if (!rc && n_corners) rc = hx_owned_alloc(ctx, st->owned, (size_t)n_corners * st->npad * 4, &st->corners);
    if (!rc && n_corners) rc = hx_memset0(ctx, st->corners, (size_t)n_corners * st->npad * 4);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, ns * st->npad * 8, &st->flux);
    if (!rc) rc = hx_memset0(ctx, st->flux, ns * st->npad * 8);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, (nb + 1) * 8, &st->inter);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, (nb + 1) * 4, &st->pbot);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, (nb + 1) * 4, &st->state);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, nb * 4, &st->wide);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, ns * nb * 8, &st->planck);
    if (!rc) rc = hx_memset0(ctx, st->planck, ns * nb * 8);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, ns * nb * 8, &st->out);
    if (!rc) rc = hx_memset0(ctx, st->out, ns * nb * 8);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, ns * 16, &st->temp_d);
    if (!rc) rc = hx_owned_alloc(ctx, st->owned, ns * sizeof(StStar), &st->stars);
    for (int k = 0; k < 3 && !rc; k++) rc = hx_stream_timer_create(ctx, st->timer[k]);
    if (rc) {
        hx_star_destroy(st);
        return rc;
    }
    *out_st = st;
    return 0;
}

int hx_star_destroy(hx_star* st) {
    if (!st) return HX_E_ARG;
    (void)hx_sync(st->ctx);
    hx_owned_free_all(st->ctx, st->owned);
    for (hx_stream_timer& t : st->timer) hx_stream_timer_destroy(t);
    delete st;
    return 0;
}

int hx_star_add_corner(hx_star* st, int slot, const void* flux_f32) {
    if (!st) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    HX_REQUIRE(ctx, flux_f32 && slot >= 0 && slot < st->ncorner, HX_E_ARG, "the corner's slot lies outside 0 ... n_corners - 1");
    int rc = st_settle(st);
    if (!rc) rc = hx_h2d(ctx, st->corners + (size_t)slot * st->npad, flux_f32, (size_t)st->N * 4);
    if (rc) return rc;
    st->have_corner[slot] = 1;
    return 0;
}

int hx_star_set_grid(hx_star* st, const double* lamda, const double* interfaces, const int* p_bot, const int* state) {
    if (!st) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    HX_REQUIRE(ctx, lamda && interfaces && p_bot && state, HX_E_ARG, "null array");
    for (int p = 1; p < st->N; p++) HX_REQUIRE(ctx, lamda[p - 1] < lamda[p], HX_E_ARG, "tabulated wavelengths do not ascend");
    std::vector<int> wide;
    int narrow = 0;
    for (int i = 0; i <= st->nbin; i++) {
        HX_REQUIRE(ctx, i == 0 || interfaces[i - 1] < interfaces[i], HX_E_ARG, "interfaces are not ascending");
        if (!state[i]) continue;
        // an evaluated interface reads the points p_bot (or, at -1, the last one) and p_bot + 1
        HX_REQUIRE(ctx, p_bot[i] >= -1 && p_bot[i] <= st->N - 2, HX_E_ARG, "an interface's index lies outside the table");
        if (i > 0 && state[i - 1]) {
            HX_REQUIRE(ctx, p_bot[i] >= p_bot[i - 1], HX_E_ARG, "the interfaces' indices do not ascend");
            if (p_bot[i] - p_bot[i - 1] > ST_NARROW) wide.push_back(i - 1);
            else narrow++;
        }
    }
    int rc = st_settle(st);
    if (!rc) rc = hx_h2d(ctx, st->lam, lamda, (size_t)st->N * 8);
    if (!rc) rc = hx_h2d(ctx, st->inter, interfaces, (size_t)(st->nbin + 1) * 8);
    if (!rc) rc = hx_h2d(ctx, st->pbot, p_bot, (size_t)(st->nbin + 1) * 4);
    if (!rc) rc = hx_h2d(ctx, st->state, state, (size_t)(st->nbin + 1) * 4);
    if (!rc && !wide.empty()) rc = hx_h2d(ctx, st->wide, wide.data(), wide.size() * 4);
    if (rc) return rc;
    st->nwide = (int)wide.size();
    st->nnarrow = narrow;
    st->have_grid = true;
    return 0;
}

int hx_star_set_star(hx_star* st, int s, int n_terms, const int* slots, const double* weights, double divisor) {
    if (!st) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    HX_REQUIRE(ctx, s >= 0 && s < st->nstar, HX_E_ARG, "the star's index lies outside 0 ... n_stars - 1");
    HX_REQUIRE(ctx, slots && weights && (n_terms == 1 || n_terms == 2 || n_terms == 4 || n_terms == 8), HX_E_ARG,
               "a blend has 1, 2, 4 or 8 terms");
    StStar d = StStar();
    d.nterms = n_terms;
    d.div = divisor;
    for (int k = 0; k < n_terms; k++) {
        HX_REQUIRE(ctx, slots[k] >= 0 && slots[k] < st->ncorner && st->have_corner[slots[k]], HX_E_ARG,
                   "a term names a corner that was not added");
        d.slot[k] = slots[k];
        for (int j = 0; j < 3; j++) d.w[k][j] = weights[3 * k + j];
    }
    st->h_stars[s] = d;
    st->have_star[s] = 1;
    return 0;
}

int hx_star_put_flux(hx_star* st, int s, const double* flux) {
    if (!st) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    HX_REQUIRE(ctx, flux && s >= 0 && s < st->nstar, HX_E_ARG, "the star's index lies outside 0 ... n_stars - 1");
    int rc = st_settle(st);
    if (!rc) rc = hx_h2d(ctx, st->flux + (size_t)s * st->npad, flux, (size_t)st->N * 8);
    if (rc) return rc;
    st->h_stars[s] = StStar();
    st->have_star[s] = 1;
    return 0;
}

int hx_star_run(hx_star* st, int n_stars, const double* bb_temp, const double* bb_prefactor, double hc, double kb, int stages) {
    if (!st) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    HX_REQUIRE(ctx, n_stars >= 1 && n_stars <= st->nstar, HX_E_ARG, "1 ... n_stars stars per run");
    HX_REQUIRE(ctx, stages >= 1 && stages <= 7, HX_E_ARG, "stages: 1 blend, 2 Planck values, 4 re-binning, or their sum");
    HX_REQUIRE(ctx, !(stages & 6) || st->have_grid, HX_E_STATE, "set the grid first");
    HX_REQUIRE(ctx, !(stages & 2) || (bb_temp && bb_prefactor), HX_E_ARG, "null array");
    for (int s = 0; s < n_stars; s++) {
        HX_REQUIRE(ctx, st->have_star[s], HX_E_STATE, "a star of the run was not set");
        HX_REQUIRE(ctx, !(stages & 2) || bb_temp[s] >= 0.0, HX_E_ARG, "the extrapolation temperature cannot be negative");
    }
    int rc = st_settle(st);
    if (rc) return rc;
    if (stages & 1) {
        rc = hx_h2d(ctx, st->stars, st->h_stars.data(), (size_t)n_stars * sizeof(StStar));
        if (!rc) rc = hx_stream_timer_start(ctx, st->timer[0]);
        if (rc) return rc;
        const dim3 grid(hx_cdiv((long long)(st->npad / ST_PER_THREAD), ST_THREADS), n_stars);
        k_star_blend<<<grid, ST_THREADS, 0, ctx->stream>>>(st->corners, st->stars, st->flux, st->npad);
        HX_LAUNCH_CHECK(ctx);
        rc = hx_stream_timer_stop(ctx, st->timer[0]);
        if (rc) return rc;
    }
    if (stages & 2) {
        std::vector<double> td(2 * (size_t)n_stars);
        for (int s = 0; s < n_stars; s++) { td[2 * s] = bb_temp[s]; td[2 * s + 1] = bb_prefactor[s]; }
        rc = hx_h2d(ctx, st->temp_d, td.data(), td.size() * 8);
        if (!rc) rc = hx_stream_timer_start(ctx, st->timer[1]);
        if (rc) return rc;
        k_star_planck_bins<<<dim3(hx_cdiv(st->nbin, ST_THREADS), n_stars), ST_THREADS, 0, ctx->stream>>>(
            st->inter, st->temp_d, st->planck, st->nbin, hc, kb);
        HX_LAUNCH_CHECK(ctx);
        rc = hx_stream_timer_stop(ctx, st->timer[1]);
        if (rc) return rc;
    }
    if (stages & 4) {
        StGrid G;
        G.lam = st->lam; G.inter = st->inter; G.pbot = st->pbot; G.state = st->state; G.flux = st->flux; G.planck = st->planck;
        G.out = st->out; G.npad = st->npad; G.N = st->N; G.nbin = st->nbin;
        rc = hx_stream_timer_start(ctx, st->timer[2]);
        if (rc) return rc;
        // bins with an interface outside the table or of few points; the kernel leaves the long ones alone
        k_star_rebin_narrow<<<dim3(hx_cdiv(st->nbin, ST_THREADS), n_stars), ST_THREADS, 0, ctx->stream>>>(G);
        HX_LAUNCH_CHECK(ctx);
        if (st->nwide) {
            const size_t lds = (size_t)(3 * st->chunk + 2) * sizeof(double);
            k_star_rebin_wide<<<dim3(st->nwide, n_stars), ST_THREADS, lds, ctx->stream>>>(G, st->wide, st->chunk);
            HX_LAUNCH_CHECK(ctx);
        }
        rc = hx_stream_timer_stop(ctx, st->timer[2]);
        if (rc) return rc;
    }
    st->timing[3] += 1.0;
    return 0;
}

int hx_star_get(hx_star* st, const char* name, void* out, size_t out_bytes) {
    if (!st || !name || !out) return HX_E_ARG;
    hx_context* ctx = st->ctx;
    int rc = st_settle(st);
    if (rc) return rc;
    const size_t ns = (size_t)st->nstar;
    if (!strcmp(name, "flux")) {       // [s][n_points], without the padding of the device rows
        if (out_bytes != ns * st->N * 8) return hx_fail(ctx, HX_E_ARG, "hx_star_get(flux): %zu bytes expected", ns * st->N * 8);
        for (size_t s = 0; s < ns && !rc; s++)
            rc = hx_d2h(ctx, (char*)out + s * st->N * 8, st->flux + s * st->npad, (size_t)st->N * 8);
        return rc;
    }
    const hx_result rows[] = {
        {"timing_ms", st->timing, sizeof st->timing, false, nullptr},
        {"converted", st->out, ns * st->nbin * 8, true, nullptr},
        {"planck", st->planck, ns * st->nbin * 8, true, nullptr},
    };
    return hx_get_result(ctx, __func__, rows, 3, name, out, out_bytes);
}

}  // extern "C"
