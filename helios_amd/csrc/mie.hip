// Lorenz-Mie series per (size parameter, refractive index) pair (include/helios_hip.h section 10; the contract and the host side
// are helios_amd/mie.py, the statements one pair at a time tests/mie_reference.py).
//
//   k_mie   one thread per pair.  The pairs of a wavefront are consecutive entries of the caller's `order` (sorted by their number
//           of terms N, descending, so that the 64 loops are of nearly equal length and the longest start first).  D_n(m x) is
//           started at n = N from Lentz's continued fraction, taken downward, and kept in the D buffer laid out [n][lane] per
//           wavefront -- one 16-byte entry per lane and n, so that a wavefront's stores and loads coalesce -- because the sums
//           run upward.  The buffer is bounded; the host packs wavefronts into it and launches as often as needed, and a
//           wavefront that would not fit with 64 lanes gets fewer.
//
// All arithmetic is fp64 without contraction, complex division is written out, and no function of the complex m x is taken.
#include "hx_tool.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

constexpr int MIE_LANES = 64;
constexpr double MIE_X_SMALL = 0.5;          // mie.py: X_SMALL, SERIES_TERMS, LENTZ_TOL_EPS, TINY
constexpr int MIE_SERIES_TERMS = 10;
constexpr double MIE_LENTZ_TOL = 16.0 * 2.220446049250313e-16;
constexpr double MIE_TINY = 1e-30;
constexpr int MIE_MAX_TERMS = 1 << 26;       // of one pair: x < 6.7e7
constexpr unsigned long long MIE_GUARD = 0x7ff8dead0badbeefULL;

struct MieWave {
    int first, count;                  // the wavefront's pairs are order[first ... first + count - 1]; count is the lane stride
    long long off;                     // of its D region, in entries
};

__device__ __forceinline__ void mie_crec(double br, double bi, double& r, double& i) {
    const double d = br * br + bi * bi;
    r = br / d;
    i = -bi / d;
}

__device__ __forceinline__ void mie_cdiv(double ar, double ai, double br, double bi, double& r, double& i) {
    const double d = br * br + bi * bi;
    r = (ar * br + ai * bi) / d;
    i = (ai * br - ar * bi) / d;
}

// psi_n(x) = x^(n+1) / (2n+1)!! (1 - x^2 / (2 (2n+3)) + ...): no cancellation for x < MIE_X_SMALL
__device__ __forceinline__ double mie_psi_series(int n, double x) {
    double s = 1.0;
    const double x2 = x * x;
    for (int k = MIE_SERIES_TERMS; k >= 1; k--) s = 1.0 - x2 / (double)(2 * k * (2 * n + 2 * k + 1)) * s;
    double pref = x;
    for (int j = 1; j <= n; j++) pref = pref * x / (double)(2 * j + 1);
    return pref * s;
}

// (D u + n/x) psi_n - psi_{n-1} over the same with xi = psi - i chi, where (ur, ui) is D / m or m D
__device__ __forceinline__ void mie_coef(double ur, double ui, double nx, double psi1, double psi0, double chi1, double chi0,
                                         double& r, double& i) {
    ur = ur + nx;
    mie_cdiv(ur * psi1 - psi0, ui * psi1, ur * psi1 + ui * chi1 - psi0, ui * psi1 - ur * chi1 + chi0, r, i);
}

__global__ __launch_bounds__(MIE_LANES) void k_mie(const MieWave* __restrict__ waves, const double* __restrict__ xs,
                                                   const double* __restrict__ m_re, const double* __restrict__ m_im,
                                                   const int* __restrict__ nterms, const int* __restrict__ cap,
                                                   const int* __restrict__ order, double2* __restrict__ dbuf,
                                                   double* __restrict__ q_ext, double* __restrict__ q_sca, double* __restrict__ g) {
    const MieWave w = waves[blockIdx.x];
    const int lane = threadIdx.x;
    if (lane >= w.count) return;
    const int pair = order[w.first + lane];
    const double x = xs[pair], mr = m_re[pair], mi = m_im[pair];
    const int N = nterms[pair], kcap = cap[pair];
    double2* __restrict__ D = dbuf + w.off + lane;           // entry n at D[n * stride], n = 1 ... N
    const size_t stride = (size_t)w.count;

    double zinv_r, zinv_i, minv_r, minv_i;
    mie_crec(mr * x, mi * x, zinv_r, zinv_i);
    mie_crec(mr, mi, minv_r, minv_i);

    // D_N(z): J_{nu-1}(z) / J_nu(z) = a_1 + 1 / (a_2 + 1 / (a_3 + ...)), nu = N + 1/2, a_k = (-1)^(k+1) (2 N + 2 k - 1) / z
    double dnr, dni;
    {
        double c = (double)(2 * N + 1);
        double fr = c * zinv_r, fi = c * zinv_i;
        if (fr == 0.0 && fi == 0.0) fr = MIE_TINY;
        double Cr = fr, Ci = fi, Dr = 0.0, Di = 0.0;
        int sign = -1;
        for (int k = 2;; k++, sign = -sign) {
            c = (double)(sign * (2 * N + 2 * k - 1));
            const double ar = c * zinv_r, ai = c * zinv_i;
            Dr = ar + Dr; Di = ai + Di;
            if (Dr == 0.0 && Di == 0.0) Dr = MIE_TINY;
            mie_crec(Dr, Di, Dr, Di);
            double tr, ti;
            mie_crec(Cr, Ci, tr, ti);
            Cr = ar + tr; Ci = ai + ti;
            if (Cr == 0.0 && Ci == 0.0) Cr = MIE_TINY;
            const double dr = Cr * Dr - Ci * Di, di = Cr * Di + Ci * Dr;
            const double nr = fr * dr - fi * di, ni = fr * di + fi * dr;
            fr = nr; fi = ni;
            if (fabs(dr - 1.0) + fabs(di) < MIE_LENTZ_TOL || k >= kcap) break;
        }
        c = (double)N;
        dnr = fr - c * zinv_r; dni = fi - c * zinv_i;
    }
    D[(size_t)N * stride] = make_double2(dnr, dni);
    for (int n = N; n >= 2; n--) {
        const double c = (double)n;
        const double tr = c * zinv_r, ti = c * zinv_i;
        double ir, ii;
        mie_crec(dnr + tr, dni + ti, ir, ii);
        dnr = tr - ir; dni = ti - ii;
        D[(size_t)(n - 1) * stride] = make_double2(dnr, dni);
    }

    const bool small = x < MIE_X_SMALL;
    const double sx = sin(x), cx = cos(x);
    double psi0 = sx, chi0 = cx;
    double psi1 = small ? mie_psi_series(1, x) : sx / x - cx;
    double chi1 = cx / x + sx;
    double s_ext = 0.0, s_sca = 0.0, s_g = 0.0;
    double a_pr = 0.0, a_pi = 0.0, b_pr = 0.0, b_pi = 0.0;
    for (int n = 1; n <= N; n++) {
        if (n >= 2) {
            const double c = (double)(2 * n - 1) / x;
            const double psi = small ? mie_psi_series(n, x) : c * psi1 - psi0;
            const double chi = c * chi1 - chi0;
            psi0 = psi1; psi1 = psi; chi0 = chi1; chi1 = chi;
        }
        const double nx = (double)n / x;
        const double2 d = D[(size_t)n * stride];
        double ar, ai, br, bi;
        mie_coef(d.x * minv_r - d.y * minv_i, d.x * minv_i + d.y * minv_r, nx, psi1, psi0, chi1, chi0, ar, ai);
        mie_coef(mr * d.x - mi * d.y, mr * d.y + mi * d.x, nx, psi1, psi0, chi1, chi0, br, bi);
        const double f = (double)(2 * n + 1);
        s_ext = s_ext + f * (ar + br);
        s_sca = s_sca + f * ((ar * ar + ai * ai) + (br * br + bi * bi));
        if (n >= 2)
            s_g = s_g + ((double)(n - 1) * (double)(n + 1)) / (double)n * ((a_pr * ar + a_pi * ai) + (b_pr * br + b_pi * bi));
        s_g = s_g + f / ((double)n * (double)(n + 1)) * (ar * br + ai * bi);
        a_pr = ar; a_pi = ai; b_pr = br; b_pi = bi;
    }
    const double q = 2.0 / (x * x);
    q_ext[pair] = q * s_ext;
    q_sca[pair] = q * s_sca;
    g[pair] = 2.0 * s_g / s_sca;
}

}  // namespace

struct hx_mie {
    hx_context* ctx;
    int nmax;
    size_t cap_entries;                // of the D buffer
    double *x, *m_re, *m_im, *q_ext, *q_sca, *g;       // the result arrays hold nmax + 1: the last is the guard
    int *nterms, *cap, *order;
    double2* dbuf;                     // cap_entries + 1
    MieWave* waves;                    // nmax: a wavefront holds at least one pair
    hx_owned owned;
    hx_stream_timer timer;
    double timing[2];                  // ms in k_mie and launches, of the last run
};

static int mie_terms(double x) { return (int)floor(x + 4.05 * pow(x, 1.0 / 3.0) + 2.0); }

extern "C" {

int hx_mie_create(hx_context* ctx, int n_pairs_max, size_t scratch_bytes, hx_mie** out_mie) {
    if (!ctx || !out_mie) return HX_E_ARG;
    HX_REQUIRE(ctx, n_pairs_max >= 1 && n_pairs_max <= (1 << 28), HX_E_ARG, "1 ... 2^28 pairs");
    HX_REQUIRE(ctx, scratch_bytes >= 64 && scratch_bytes <= ((size_t)1 << 36), HX_E_ARG, "the D buffer holds 64 bytes ... 64 GiB");
    hx_mie* h = new (std::nothrow) hx_mie();
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->nmax = n_pairs_max;
    h->cap_entries = scratch_bytes / sizeof(double2);
    const size_t n = (size_t)n_pairs_max;
    int rc = hx_owned_alloc(ctx, h->owned, n * 8, &h->x);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * 8, &h->m_re);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * 8, &h->m_im);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (n + 1) * 8, &h->q_ext);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (n + 1) * 8, &h->q_sca);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (n + 1) * 8, &h->g);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * 4, &h->nterms);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * 4, &h->cap);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * 4, &h->order);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, n * sizeof(MieWave), &h->waves);
    if (!rc) {
        rc = hx_owned_alloc(ctx, h->owned, (h->cap_entries + 1) * sizeof(double2), &h->dbuf);
        if (rc) rc = hx_fail(ctx, rc, "hx_mie_create: no device memory for a D buffer of %zu bytes", scratch_bytes);
    }
    if (!rc) rc = hx_memset0(ctx, h->q_ext, n * 8);
    if (!rc) rc = hx_memset0(ctx, h->q_sca, n * 8);
    if (!rc) rc = hx_memset0(ctx, h->g, n * 8);
    if (!rc) {
        const unsigned long long gd[2] = {MIE_GUARD, MIE_GUARD};
        rc = hx_h2d(ctx, h->q_ext + n, gd, 8);
        if (!rc) rc = hx_h2d(ctx, h->q_sca + n, gd, 8);
        if (!rc) rc = hx_h2d(ctx, h->g + n, gd, 8);
        if (!rc) rc = hx_h2d(ctx, h->dbuf + h->cap_entries, gd, 16);
    }
    if (!rc) rc = hx_stream_timer_create(ctx, h->timer);
    if (rc) {
        hx_mie_destroy(h);
        return rc;
    }
    *out_mie = h;
    return 0;
}

int hx_mie_destroy(hx_mie* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->timer);
    delete h;
    return 0;
}

int hx_mie_run(hx_mie* h, int n_pairs, const double* x, const double* m_re, const double* m_im, const int* order) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, x && m_re && m_im && order, HX_E_ARG, "null array");
    if (n_pairs < 1 || n_pairs > h->nmax)
        return hx_fail(ctx, HX_E_ARG, "hx_mie_run: %d pairs, the handle holds 1 ... %d", n_pairs, h->nmax);
    std::vector<int> nt(n_pairs), cap(n_pairs);
    std::vector<char> seen(n_pairs, 0);
    for (int p = 0; p < n_pairs; p++) {
        if (!(x[p] > 0.0) || !std::isfinite(x[p]))
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d: x = %g is not a finite number > 0", p, x[p]);
        if (!(m_re[p] > 0.0) || !std::isfinite(m_re[p]))
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d: m_re = %g is not a finite number > 0", p, m_re[p]);
        if (!(m_im[p] >= 0.0) || !std::isfinite(m_im[p]))
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d: m_im = %g is not a finite number >= 0", p, m_im[p]);
        const double terms = floor(x[p] + 4.05 * pow(x[p], 1.0 / 3.0) + 2.0);
        if (terms > (double)MIE_MAX_TERMS)
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d: x = %g needs more than 2^26 terms", p, x[p]);
        nt[p] = mie_terms(x[p]);
        const size_t bytes = ((size_t)nt[p] + 1) * sizeof(double2);
        if ((size_t)nt[p] + 1 > h->cap_entries)
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d (x = %.17g, m = %.17g + %.17g i, %d terms) needs %zu bytes for its "
                           "D_n, the buffer holds %zu", p, x[p], m_re[p], m_im[p], nt[p], bytes, h->cap_entries * sizeof(double2));
        const double zabs = sqrt(m_re[p] * m_re[p] + m_im[p] * m_im[p]) * x[p];
        const double c = zabs + 4.05 * pow(zabs, 1.0 / 3.0);
        if (!(c < (double)MIE_MAX_TERMS))
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: pair %d: |m| x = %g needs more than 2^26 steps of the continued fraction", p, zabs);
        cap[p] = (int)c + 100;
    }
    for (int p = 0; p < n_pairs; p++) {
        if (order[p] < 0 || order[p] >= n_pairs || seen[order[p]])
            return hx_fail(ctx, HX_E_ARG, "hx_mie_run: order[%d] = %d: order is not a permutation of 0 ... %d", p, order[p],
                           n_pairs - 1);
        seen[order[p]] = 1;
    }
    // wavefronts of up to 64 consecutive pairs of `order`, packed into the D buffer; a launch per filling.  Entry n of lane l
    // lies at off + n * count + l, n = 0 ... depth - 1 with depth = 1 + the wavefront's largest N
    std::vector<MieWave> waves;
    std::vector<int> launch_first;      // index into waves
    int p = 0;
    while (p < n_pairs) {
        launch_first.push_back((int)waves.size());
        size_t used = 0;
        while (p < n_pairs) {
            int cnt = 0;
            size_t depth = 0;
            while (cnt < MIE_LANES && p + cnt < n_pairs) {
                const size_t d = std::max(depth, (size_t)nt[order[p + cnt]] + 1);
                if (used + d * (size_t)(cnt + 1) > h->cap_entries) break;
                depth = d;
                cnt++;
            }
            if (cnt == 0) break;        // the buffer is full (an empty one takes any single pair: checked above)
            MieWave w;
            w.first = p; w.count = cnt; w.off = (long long)used;
            waves.push_back(w);
            used += depth * (size_t)cnt;
            p += cnt;
        }
    }
    launch_first.push_back((int)waves.size());
    int rc = hx_h2d(ctx, h->x, x, (size_t)n_pairs * 8);
    if (!rc) rc = hx_h2d(ctx, h->m_re, m_re, (size_t)n_pairs * 8);
    if (!rc) rc = hx_h2d(ctx, h->m_im, m_im, (size_t)n_pairs * 8);
    if (!rc) rc = hx_h2d(ctx, h->nterms, nt.data(), (size_t)n_pairs * 4);
    if (!rc) rc = hx_h2d(ctx, h->cap, cap.data(), (size_t)n_pairs * 4);
    if (!rc) rc = hx_h2d(ctx, h->order, order, (size_t)n_pairs * 4);
    if (!rc) rc = hx_h2d(ctx, h->waves, waves.data(), waves.size() * sizeof(MieWave));
    if (!rc) rc = hx_stream_timer_start(ctx, h->timer);
    if (rc) return rc;
    const int launches = (int)launch_first.size() - 1;
    for (int l = 0; l < launches; l++) {
        const int w0 = launch_first[l], nw = launch_first[l + 1] - w0;
        k_mie<<<nw, MIE_LANES, 0, ctx->stream>>>(h->waves + w0, h->x, h->m_re, h->m_im, h->nterms, h->cap, h->order, h->dbuf,
                                                 h->q_ext, h->q_sca, h->g);
        HX_LAUNCH_CHECK(ctx);
    }
    h->timing[0] = 0.0;                 // of this run alone, and it has ended when the call returns
    h->timing[1] = launches;
    rc = hx_stream_timer_stop(ctx, h->timer);
    if (!rc) rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    return rc;
}

int hx_mie_get(hx_mie* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (!strcmp(name, "guard")) {       // behind q_ext, q_sca, g, and the two doubles behind the D buffer
        if (out_bytes != 40) return hx_fail(ctx, HX_E_ARG, "hx_mie_get(guard): 40 bytes expected");
        int rc = hx_d2h(ctx, out, h->q_ext + h->nmax, 8);
        if (!rc) rc = hx_d2h(ctx, (char*)out + 8, h->q_sca + h->nmax, 8);
        if (!rc) rc = hx_d2h(ctx, (char*)out + 16, h->g + h->nmax, 8);
        if (!rc) rc = hx_d2h(ctx, (char*)out + 24, h->dbuf + h->cap_entries, 16);
        return rc;
    }
    const double* src = !strcmp(name, "q_ext") ? h->q_ext : !strcmp(name, "q_sca") ? h->q_sca : !strcmp(name, "g") ? h->g : nullptr;
    if (src) {                          // the first out_bytes: a run may hold fewer pairs than the handle
        if (out_bytes == 0 || out_bytes % 8 || out_bytes > (size_t)h->nmax * 8)
            return hx_fail(ctx, HX_E_ARG, "hx_mie_get(%s): 8 ... %zu bytes expected, got %zu", name, (size_t)h->nmax * 8, out_bytes);
        return hx_d2h(ctx, out, src, out_bytes);
    }
    const hx_result row = {"timing_ms", h->timing, sizeof h->timing, false, nullptr};
    return hx_get_result(ctx, __func__, &row, 1, name, out, out_bytes);
}

}  // extern "C"
