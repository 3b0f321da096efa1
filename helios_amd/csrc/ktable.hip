// Per-species k-tables from HELIOS-K opacities (include/helios_hip.h section 6; the host logic is helios_amd/ktable.py).
//
// k_ktable_bins: one workgroup per (wavelength bin, (T, P) point).  Every point of the bin becomes a 64-bit key -- high word:
// the bits of the floored fp32 opacity (positive, so bit order is value order; 0 stands for the floor 1e-15, below every fp32
// above it), low word: the point's place in ascending weight w -- the keys are sorted by a bitonic network, in LDS where the
// bin fits and through a global scratch of 8 B per point where it does not, w is recomputed from the low word, the
// mid-point sums are scanned in fp64 (a sequential run per thread, a tree over the runs), and every Gauss abscissa is
// placed by a binary search over the runs and a walk through one.  The output has the layout of `kpoints`.
//
// The network is the ascending-only form of the bitonic sort (the first step of a merge compares i with its mirror in the
// block, the others i with i + j): every comparator leaves the larger key at the higher index, so padding of +inf behind the
// n keys would never move, and comparators that reach beyond n are skipped instead of padded for.
#include <algorithm>
#include <vector>

#include "hx_tool.h"

namespace {

constexpr int KT_THREADS = 1024;
constexpr int KT_LANES = 64;
constexpr int KT_MAX_LDS_POINTS = 16384;      // 128 KiB of keys next to 16 KiB of scan records: 144 of the CU's 160 KiB
constexpr double KT_FLOOR = 1e-15;
typedef unsigned long long kt_key;

struct KtArgs {
    const double* lam;        // [N] ascending wavelength
    const int* bstart;        // [nbin]
    const int* bend;          // [nbin]
    const double* inter;      // [nbin + 1]
    const double* yg;         // [ng]
    const float* opac;        // [ntp of this launch][N], ascending wavenumber
    kt_key* scratch;          // [ntp of this launch][N], or null when no bin exceeds cap
    double* out;              // kpoints of the launch's first (T, P) point
    int N, nbin, ng, cap;
};

struct KtBin {
    const double* lb;         // wavelengths of the bin's points
    double lo, hi, width;
    int n;
};

__device__ __forceinline__ double kt_weight(const KtBin& b, int i) {
    double w;
    if (i == 0) w = (b.lb[0] - b.lo) + (b.lb[1] - b.lb[0]) / 2;
    else if (i == b.n - 1) w = (b.hi - b.lb[b.n - 1]) + (b.lb[b.n - 1] - b.lb[b.n - 2]) / 2;
    else w = (b.lb[i + 1] - b.lb[i - 1]) / 2;
    return w / b.width;
}

// number of interior points (1 .. n-2, whose w rises with the index) that weigh less than `w`
__device__ int kt_interior_below(const KtBin& b, double w) {
    int lo = 1, hi = b.n - 1;            // first interior index with weight >= w, n - 1 if none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kt_weight(b, mid) < w) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ unsigned kt_high(float k) {
    return ((double)k > KT_FLOOR) ? __float_as_uint(k) : 0u;      // NaN, zero and negative values land on the floor
}

__device__ __forceinline__ int kt_index(kt_key key, int n) {
    const unsigned low = (unsigned)key;
    return (low & 7u) == 0u ? (int)(low >> 3) : ((low & 1u) ? n - 1 : 0);
}

__device__ __forceinline__ double kt_floored(kt_key key) {
    const unsigned h = (unsigned)(key >> 32);
    return h == 0u ? KT_FLOOR : (double)__uint_as_float(h);
}

__device__ __forceinline__ void kt_cmpx(kt_key* a, int i, int j) {
    const kt_key x = a[i], y = a[j];
    if (x > y) { a[i] = y; a[j] = x; }
}

// one step over the m keys of `a`: flip = the first step of the merge of blocks of k, otherwise stride j
__device__ __forceinline__ void kt_step(kt_key* a, int m, int k, int j, bool flip) {
    for (int p = threadIdx.x; ; p += KT_THREADS) {
        int lo, hi;
        if (flip) {
            const int h = k >> 1, blk = p / h, w = p - blk * h;
            lo = blk * k + w;
            hi = blk * k + k - 1 - w;
        } else {
            const int blk = p / j, w = p - blk * j;
            lo = blk * 2 * j + w;
            hi = lo + j;
        }
        if (lo >= m) break;              // lo rises with p
        if (hi < m) kt_cmpx(a, lo, hi);
    }
}

// the merges of block sizes 2 .. k_last over the m keys of `a` (LDS)
__device__ void kt_sort_lds(kt_key* a, int m, int k_last) {
    for (int k = 2; k <= k_last && (k >> 1) < m; k <<= 1) {
        __syncthreads();
        kt_step(a, m, k, 0, true);
        for (int j = k >> 2; j > 0; j >>= 1) {
            __syncthreads();
            kt_step(a, m, k, j, false);
        }
    }
    __syncthreads();
}

__launch_bounds__(KT_THREADS) __global__ void k_ktable_bins(KtArgs A) {
    extern __shared__ kt_key sk[];                 // cap keys
    __shared__ double run_sum[KT_THREADS];         // per run of the scan: its sum, then the sum of the runs before it
    __shared__ double run_first[KT_THREADS];       // y of the run's first point
    const int x = blockIdx.x, tp = blockIdx.y, tid = threadIdx.x;
    const int s = A.bstart[x], n = A.bend[x] - s;
    double* out = A.out + ((size_t)tp * A.nbin + x) * A.ng;
    const float* opac = A.opac + (size_t)tp * A.N;           // point j of the wavelength axis is opac[N - 1 - j]
    if (n < 2) {
        double v = KT_FLOOR;
        if (n == 1) {
            const float k = opac[A.N - 1 - s];
            v = ((double)k > KT_FLOOR) ? (double)k : KT_FLOOR;
        }
        for (int g = tid; g < A.ng; g += KT_THREADS) out[g] = v;
        return;
    }
    KtBin b;
    b.lb = A.lam + s; b.lo = A.inter[x]; b.hi = A.inter[x + 1]; b.width = b.hi - b.lo; b.n = n;

    // low words of the bin's two ends: placed among the interior points by their actual weights
    __shared__ unsigned end_low[2];
    if (tid < 2) {
        const double w0 = kt_weight(b, 0), w1 = kt_weight(b, n - 1);
        const double mine = tid ? w1 : w0;
        const unsigned c = n > 2 ? (unsigned)kt_interior_below(b, mine) : 0u;
        const unsigned first_goes_first = w0 <= w1 ? 1u : 0u;
        const unsigned order = tid ? (first_goes_first ? 2u : 1u) : (first_goes_first ? 1u : 2u);
        end_low[tid] = 8u * c + 2u * order + (unsigned)tid;
    }
    __syncthreads();
    const bool in_lds = n <= A.cap;
    kt_key* keys = in_lds ? sk : A.scratch + (size_t)tp * A.N + s;
    for (int i = tid; i < n; i += KT_THREADS) {
        const unsigned low = i == 0 ? end_low[0] : (i == n - 1 ? end_low[1] : 8u * (unsigned)i);
        keys[i] = ((kt_key)kt_high(opac[A.N - 1 - (s + i)]) << 32) | low;
    }
    if (in_lds) {
        kt_sort_lds(sk, n, A.cap);
    } else {
        const int cap = A.cap;
        __syncthreads();
        // blocks of cap keys, each sorted in LDS
        for (int base = 0; base < n; base += cap) {
            const int m = min(cap, n - base);
            for (int i = tid; i < m; i += KT_THREADS) sk[i] = keys[base + i];
            kt_sort_lds(sk, m, cap);
            for (int i = tid; i < m; i += KT_THREADS) keys[base + i] = sk[i];
            __syncthreads();
        }
        // merges of larger blocks: strides of a block or more in the scratch, the rest of each merge block by block in LDS
        for (int k = 2 * cap; (k >> 1) < n; k <<= 1) {
            kt_step(keys, n, k, 0, true);
            __syncthreads();
            for (int j = k >> 2; j >= cap; j >>= 1) {
                kt_step(keys, n, k, j, false);
                __syncthreads();
            }
            for (int base = 0; base < n; base += cap) {
                const int m = min(cap, n - base);
                for (int i = tid; i < m; i += KT_THREADS) sk[i] = keys[base + i];
                for (int j = cap >> 1; j > 0; j >>= 1) {
                    __syncthreads();
                    kt_step(sk, m, 2 * j, j, false);
                }
                __syncthreads();
                for (int i = tid; i < m; i += KT_THREADS) keys[base + i] = sk[i];
                __syncthreads();
            }
        }
    }

    // scan of the mid-point sums: y_0 = w_0 / 2, y_i = y_{i-1} + (w_{i-1} + w_i) / 2.  Thread t runs over L points.
    const int L = (n + KT_THREADS - 1) / KT_THREADS;
    {
        const int i0 = tid * L, i1 = min(n, i0 + L);
        double sum = 0.0, first = 0.0;
        if (i0 < i1) {
            double wp = i0 > 0 ? kt_weight(b, kt_index(keys[i0 - 1], n)) : 0.0;
            for (int i = i0; i < i1; i++) {
                const double w = kt_weight(b, kt_index(keys[i], n));
                const double mid = i == 0 ? 0.5 * w : 0.5 * (wp + w);
                sum += mid;
                if (i == i0) first = mid;
                wp = w;
            }
        }
        run_sum[tid] = sum;
        run_first[tid] = first;
    }
    __syncthreads();
    if (tid < KT_LANES) {          // the first wavefront: 16 runs per lane, a tree over the lanes
        constexpr int PER = KT_THREADS / KT_LANES;
        double v[PER], lane_sum = 0.0;
#pragma unroll
        for (int q = 0; q < PER; q++) { v[q] = run_sum[tid * PER + q]; lane_sum += v[q]; }
        double incl = lane_sum;
#pragma unroll
        for (int d = 1; d < KT_LANES; d <<= 1) {
            const double up = __shfl_up(incl, d, KT_LANES);
            if (tid >= d) incl = up + incl;
        }
        const double prev = __shfl_up(incl, 1, KT_LANES);
        double before = tid == 0 ? 0.0 : prev;
#pragma unroll
        for (int q = 0; q < PER; q++) { run_sum[tid * PER + q] = before; before += v[q]; }
    }
    __syncthreads();
    run_first[tid] += run_sum[tid];
    __syncthreads();

    // the Gauss abscissae: linear in y between the two points around each, the end values outside
    const int nrun = (n + L - 1) / L;
    for (int g = tid; g < A.ng; g += KT_THREADS) {
        const double xg = A.yg[g];
        double v;
        if (!(run_first[0] < xg)) {
            v = log10(kt_floored(keys[0]));                  // at or below y_0
        } else {
            int lo = 0, hi = nrun - 1;                       // last run whose first y is below xg
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (run_first[mid] < xg) lo = mid; else hi = mid - 1;
            }
            const int i0 = lo * L, i1 = min(n, i0 + L);
            const double off = run_sum[lo];
            double sum = 0.0, wp = i0 > 0 ? kt_weight(b, kt_index(keys[i0 - 1], n)) : 0.0;
            double y_lo = 0.0, y_hi = 0.0;
            int at = -1;                                     // first point of the run with y >= xg (never its first)
            for (int i = i0; i < i1; i++) {
                const double w = kt_weight(b, kt_index(keys[i], n));
                sum += i == 0 ? 0.5 * w : 0.5 * (wp + w);
                wp = w;
                const double y = off + sum;
                if (i > i0 && y >= xg) { at = i; y_hi = y; break; }
                y_lo = y;
            }
            if (at < 0 && lo + 1 < nrun) { at = i1; y_hi = run_first[lo + 1]; }
            if (at < 0) {
                v = log10(kt_floored(keys[n - 1]));          // above y_{n-1}
            } else {
                const double k_lo = log10(kt_floored(keys[at - 1])), k_hi = log10(kt_floored(keys[at]));
                const double slope = (k_hi - k_lo) / (y_hi - y_lo);
                v = slope * (xg - y_lo) + k_lo;
            }
        }
        out[g] = pow(10.0, v);
    }
}

struct KtRegrid {
    const double* k_old; double* k_new;
    const int *t_left, *t_red, *p_left, *p_red;
    const double *T, *lp, *Tn, *lpn;
    int nc, np_old, np_new;
    size_t total;
};

// bilinear in T and log10 P, the source's edge value outside its nodes; the four branches and their term order are the
// reference's (ktable/source_ktable/combination.py, interpolate_opacity_to_final_grid)
__global__ void k_ktable_regrid(KtRegrid R) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < R.total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx % R.nc);
        const size_t node = idx / R.nc;
        const int j = (int)(node % R.np_new), i = (int)(node / R.np_new);
        const int t0 = R.t_left[i], p0 = R.p_left[j];
        const bool rt = R.t_red[i] != 0, rp = R.p_red[j] != 0;
        auto K = [&](int t, int p) { return R.k_old[((size_t)t * R.np_old + p) * R.nc + e]; };
        double v;
        if (rt && rp) {
            v = K(t0, p0);
        } else if (rt) {
            const double c = R.lpn[j] - R.lp[p0], d = R.lp[p0 + 1] - R.lpn[j];
            v = (K(t0, p0 + 1) * c + K(t0, p0) * d) / (R.lp[p0 + 1] - R.lp[p0]);
        } else if (rp) {
            const double a = R.Tn[i] - R.T[t0], b = R.T[t0 + 1] - R.Tn[i];
            v = (K(t0 + 1, p0) * a + K(t0, p0) * b) / (R.T[t0 + 1] - R.T[t0]);
        } else {
            const double a = R.Tn[i] - R.T[t0], b = R.T[t0 + 1] - R.Tn[i];
            const double c = R.lpn[j] - R.lp[p0], d = R.lp[p0 + 1] - R.lpn[j];
            v = (K(t0 + 1, p0 + 1) * a * c + K(t0 + 1, p0) * a * d + K(t0, p0 + 1) * b * c + K(t0, p0) * b * d) /
                ((R.T[t0 + 1] - R.T[t0]) * (R.lp[p0 + 1] - R.lp[p0]));
        }
        R.k_new[idx] = v;
    }
}

}  // namespace

struct hx_ktable {
    hx_context* ctx;
    int N, nbin, ng, ntp, maxtp, cap;
    double *lam, *inter, *yg, *out, *ip;
    int *bstart, *bend;
    float* opac;
    kt_key* scratch;
    size_t ip_nodes;
    bool have_grid;
    hx_owned owned;
    hx_stream_timer timer;     // around the last launch of k_ktable_bins; settled by the next call
    double timing[4];          // kernel ms of k_ktable_bins, launches, ms of the re-gridding, (T, P) points done
};

static int kt_settle(hx_ktable* kt) { return hx_stream_timer_settle(kt->ctx, kt->timer, &kt->timing[0]); }

extern "C" {

// the one re-gridding of the library: hx_ktable_regrid and hx_ktmix_set_species_native (ktable_mix.hip) both end here
int hx_internal_regrid_check(hx_context* ctx, const char* fn, const hx_regrid_plan* P) {
#define RG_REQUIRE(cond, msg)                                                 \
    do {                                                                      \
        if (!(cond)) return hx_fail(ctx, HX_E_ARG, "%s: %s", fn, (msg));      \
    } while (0)
    RG_REQUIRE(P->nt_new >= 1 && P->np_new >= 1, "an empty target grid");
    RG_REQUIRE(P->t_left && P->t_reduced && P->p_left && P->p_reduced && P->temp_old && P->logp_old && P->temp_new && P->logp_new,
               "null array");
    // a node that is not clamped reads its left neighbour and the one after it
    for (int i = 0; i < P->nt_new; i++)
        RG_REQUIRE(P->t_left[i] >= 0 && P->t_left[i] + (P->t_reduced[i] ? 0 : 1) < P->nt_old, "temperature plan out of range");
    for (int j = 0; j < P->np_new; j++)
        RG_REQUIRE(P->p_left[j] >= 0 && P->p_left[j] + (P->p_reduced[j] ? 0 : 1) < P->np_old, "pressure plan out of range");
#undef RG_REQUIRE
    return 0;
}

int hx_internal_regrid(hx_context* ctx, const char* fn, const hx_regrid_plan* P, const double* k_old, double* k_new, size_t nc,
                       double* ms) {
    int rc = hx_internal_regrid_check(ctx, fn, P);
    if (rc) return rc;
    const int nt_old = P->nt_old, np_old = P->np_old, nt_new = P->nt_new, np_new = P->np_new;
    const size_t ni = (size_t)2 * (nt_new + np_new), nd = (size_t)nt_old + np_old + nt_new + np_new;
    int* d_i = nullptr;
    double* d_d = nullptr;
    std::vector<int> hi;
    std::vector<double> hd;
    hi.insert(hi.end(), P->t_left, P->t_left + nt_new); hi.insert(hi.end(), P->t_reduced, P->t_reduced + nt_new);
    hi.insert(hi.end(), P->p_left, P->p_left + np_new); hi.insert(hi.end(), P->p_reduced, P->p_reduced + np_new);
    hd.insert(hd.end(), P->temp_old, P->temp_old + nt_old); hd.insert(hd.end(), P->logp_old, P->logp_old + np_old);
    hd.insert(hd.end(), P->temp_new, P->temp_new + nt_new); hd.insert(hd.end(), P->logp_new, P->logp_new + np_new);
    rc = hx_alloc(ctx, ni * 4, (void**)&d_i);
    if (!rc) rc = hx_alloc(ctx, nd * 8, (void**)&d_d);
    if (!rc) rc = hx_h2d(ctx, d_i, hi.data(), ni * 4);
    if (!rc) rc = hx_h2d(ctx, d_d, hd.data(), nd * 8);
    double took = 0.0;
    if (!rc) {
        KtRegrid R;
        R.k_old = k_old; R.k_new = k_new;
        R.t_left = d_i; R.t_red = d_i + nt_new; R.p_left = d_i + 2 * nt_new; R.p_red = d_i + 2 * nt_new + np_new;
        R.T = d_d; R.lp = d_d + nt_old; R.Tn = d_d + nt_old + np_old; R.lpn = d_d + nt_old + np_old + nt_new;
        R.nc = (int)nc; R.np_old = np_old; R.np_new = np_new; R.total = (size_t)nt_new * np_new * nc;
        const int grid = (int)std::min<size_t>((R.total + 255) / 256, 65536);
        rc = hx_timer_start(ctx);
        if (!rc) {
            k_ktable_regrid<<<grid, 256, 0, ctx->stream>>>(R);
            rc = hipGetLastError() == hipSuccess ? 0 : hx_fail(ctx, HX_E_ARG, "%s: k_ktable_regrid launch failed", fn);
        }
        if (!rc) rc = hx_timer_stop_ms(ctx, &took);
    }
    (void)hx_free(ctx, d_i);
    (void)hx_free(ctx, d_d);
    if (!rc) *ms += took;
    return rc;
}

int hx_ktable_create(hx_context* ctx, int n_points, int n_bins, int n_gauss, int n_tp, int max_tp_per_launch, int lds_points,
                     hx_ktable** out_kt) {
    if (!ctx || !out_kt) return HX_E_ARG;
    HX_REQUIRE(ctx, n_points >= 1 && n_points <= (1 << 28), HX_E_ARG, "1 ... 2^28 spectral points");
    HX_REQUIRE(ctx, n_bins >= 1 && n_gauss >= 1 && n_tp >= 1, HX_E_ARG, "bins, Gauss points and (T, P) points are >= 1");
    HX_REQUIRE(ctx, max_tp_per_launch >= 1 && max_tp_per_launch <= 65535, HX_E_ARG, "1 ... 65535 (T, P) points per launch");
    HX_REQUIRE(ctx, lds_points >= 2 && lds_points <= KT_MAX_LDS_POINTS && (lds_points & (lds_points - 1)) == 0, HX_E_ARG,
               "the LDS sort holds a power of two of 2 ... 16384 points");
    hx_ktable* kt = new (std::nothrow) hx_ktable();
    if (!kt) return hx_fail(ctx, HX_E_ARG, "no host memory");
    kt->ctx = ctx;
    kt->N = n_points; kt->nbin = n_bins; kt->ng = n_gauss; kt->ntp = n_tp;
    kt->maxtp = std::min(max_tp_per_launch, n_tp); kt->cap = lds_points;
    hx_owned& o = kt->owned;
    int rc = hx_owned_alloc(ctx, o, (size_t)n_points * 8, &kt->lam);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)(n_bins + 1) * 8, &kt->inter);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)n_gauss * 8, &kt->yg);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)n_bins * 4, &kt->bstart);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)n_bins * 4, &kt->bend);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)kt->maxtp * n_points * 4, &kt->opac);
    if (!rc) rc = hx_owned_alloc(ctx, o, (size_t)n_tp * n_bins * n_gauss * 8, &kt->out);
    if (!rc) rc = hx_stream_timer_create(ctx, kt->timer);
    if (!rc) rc = hipFuncSetAttribute((const void*)k_ktable_bins, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      KT_MAX_LDS_POINTS * (int)sizeof(kt_key)) == hipSuccess
                      ? 0 : hx_fail(ctx, HX_E_UNSUPPORTED, "k_ktable_bins: 128 KiB of dynamic LDS were refused");
    if (rc) {
        hx_ktable_destroy(kt);
        return rc;
    }
    *out_kt = kt;
    return 0;
}

int hx_ktable_destroy(hx_ktable* kt) {
    if (!kt) return HX_E_ARG;
    (void)hx_sync(kt->ctx);
    hx_owned_free_all(kt->ctx, kt->owned);
    hx_stream_timer_destroy(kt->timer);
    delete kt;
    return 0;
}

int hx_ktable_set_grid(hx_ktable* kt, const double* lamda, const int* bin_start, const int* bin_end, const double* interfaces,
                       const double* gauss_y) {
    if (!kt) return HX_E_ARG;
    hx_context* ctx = kt->ctx;
    HX_REQUIRE(ctx, lamda && bin_start && bin_end && interfaces && gauss_y, HX_E_ARG, "null array");
    int longest = 0;
    for (int x = 0; x < kt->nbin; x++) {
        HX_REQUIRE(ctx, 0 <= bin_start[x] && bin_start[x] <= bin_end[x] && bin_end[x] <= kt->N, HX_E_ARG,
                   "a bin's range lies outside the spectral axis");
        // two workgroups would sort the same stretch of the scratch at once
        HX_REQUIRE(ctx, x == 0 || bin_start[x] >= bin_end[x - 1], HX_E_ARG, "the bins' ranges overlap or do not ascend");
        HX_REQUIRE(ctx, interfaces[x] < interfaces[x + 1], HX_E_ARG, "interfaces are not ascending");
        longest = std::max(longest, bin_end[x] - bin_start[x]);
    }
    int rc = kt_settle(kt);
    if (!rc) rc = hx_h2d(ctx, kt->lam, lamda, (size_t)kt->N * 8);
    if (!rc) rc = hx_h2d(ctx, kt->bstart, bin_start, (size_t)kt->nbin * 4);
    if (!rc) rc = hx_h2d(ctx, kt->bend, bin_end, (size_t)kt->nbin * 4);
    if (!rc) rc = hx_h2d(ctx, kt->inter, interfaces, (size_t)(kt->nbin + 1) * 8);
    if (!rc) rc = hx_h2d(ctx, kt->yg, gauss_y, (size_t)kt->ng * 8);
    if (!rc && longest > kt->cap && !kt->scratch) rc = hx_owned_alloc(ctx, kt->owned, (size_t)kt->maxtp * kt->N * 8, &kt->scratch);
    if (rc) return rc;
    kt->have_grid = true;
    return 0;
}

// what hx_ktable_run and hx_kt_run_device share: the checks, then -- `upload`: the slabs into the table's own buffer first --
// one launch over the slabs where they then are
static int kt_run(hx_ktable* kt, const char* fn, const void* slabs, bool upload, int n_tp, int first_tp) {
    hx_context* ctx = kt->ctx;
#define KT_REQUIRE(cond, code, msg)                                           \
    do {                                                                      \
        if (!(cond)) return hx_fail(ctx, (code), "%s: %s", fn, (msg));        \
    } while (0)
    KT_REQUIRE(kt->have_grid, HX_E_STATE, "set the grid first");
    KT_REQUIRE(slabs && n_tp >= 1 && n_tp <= kt->maxtp, HX_E_ARG, "1 ... max_tp_per_launch slabs per call");
    KT_REQUIRE(first_tp >= 0 && first_tp <= kt->ntp - n_tp, HX_E_ARG, "the slabs reach beyond the table's (T, P) points");
#undef KT_REQUIRE
    int rc = kt_settle(kt);
    if (!rc && upload) rc = hx_h2d(ctx, kt->opac, slabs, (size_t)n_tp * kt->N * 4);
    if (rc) return rc;
    KtArgs A;
    A.lam = kt->lam; A.bstart = kt->bstart; A.bend = kt->bend; A.inter = kt->inter; A.yg = kt->yg;
    A.opac = upload ? kt->opac : (const float*)slabs; A.scratch = kt->scratch;
    A.out = kt->out + (size_t)first_tp * kt->nbin * kt->ng;
    A.N = kt->N; A.nbin = kt->nbin; A.ng = kt->ng; A.cap = kt->cap;
    rc = hx_stream_timer_start(ctx, kt->timer);
    if (rc) return rc;
    k_ktable_bins<<<dim3(kt->nbin, n_tp), KT_THREADS, (size_t)kt->cap * sizeof(kt_key), ctx->stream>>>(A);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, kt->timer);
    if (rc) return rc;
    kt->timing[1] += 1.0;
    kt->timing[3] += n_tp;
    return 0;
}

int hx_ktable_run(hx_ktable* kt, const void* opac_f32, int n_tp, int first_tp) {
    if (!kt) return HX_E_ARG;
    return kt_run(kt, __func__, opac_f32, true, n_tp, first_tp);
}

int hx_kt_run_device(hx_ktable* kt, const void* d_opac_f32, int n_tp, int first_tp) {
    if (!kt) return HX_E_ARG;
    if (!d_opac_f32) return hx_fail(kt->ctx, HX_E_ARG, "hx_kt_run_device: the device slabs are a null pointer");
    return kt_run(kt, __func__, d_opac_f32, false, n_tp, first_tp);
}

int hx_ktable_regrid(hx_ktable* kt, int nt_old, int np_old, int nt_new, int np_new, const int* t_left, const int* t_reduced,
                     const int* p_left, const int* p_reduced, const double* temp_old, const double* logp_old,
                     const double* temp_new, const double* logp_new) {
    if (!kt) return HX_E_ARG;
    hx_context* ctx = kt->ctx;
    HX_REQUIRE(ctx, nt_old >= 1 && np_old >= 1 && (long long)nt_old * np_old == kt->ntp, HX_E_ARG,
               "nt_old x np_old is not the table's number of (T, P) points");
    const hx_regrid_plan plan = {nt_old, np_old, nt_new, np_new, t_left, t_reduced, p_left, p_reduced,
                                 temp_old, logp_old, temp_new, logp_new};
    int rc = hx_internal_regrid_check(ctx, __func__, &plan);
    if (!rc) rc = kt_settle(kt);
    if (rc) return rc;
    const size_t nc = (size_t)kt->nbin * kt->ng, nodes = (size_t)nt_new * np_new;
    rc = hx_owned_free(ctx, kt->owned, kt->ip);      // a refused plan leaves the last result; a failure from here on leaves none
    kt->ip = nullptr; kt->ip_nodes = 0;
    if (!rc) rc = hx_owned_alloc(ctx, kt->owned, nodes * nc * 8, &kt->ip);
    if (!rc) rc = hx_internal_regrid(ctx, __func__, &plan, kt->out, kt->ip, nc, &kt->timing[2]);
    if (rc) return rc;
    kt->ip_nodes = nodes;
    return 0;
}

int hx_ktable_put(hx_ktable* kt, const double* kpoints) {
    if (!kt || !kpoints) return HX_E_ARG;
    int rc = kt_settle(kt);
    if (rc) return rc;
    return hx_h2d(kt->ctx, kt->out, kpoints, (size_t)kt->ntp * kt->nbin * kt->ng * 8);
}

int hx_ktable_get(hx_ktable* kt, const char* name, void* out, size_t out_bytes) {
    if (!kt || !name || !out) return HX_E_ARG;
    int rc = kt_settle(kt);
    if (rc) return rc;
    const size_t nc = (size_t)kt->nbin * kt->ng;
    const hx_result rows[] = {
        {"timing_ms", kt->timing, sizeof kt->timing, false, nullptr},
        {"kpoints", kt->out, (size_t)kt->ntp * nc * 8, true, nullptr},
        {"kpoints_ip", kt->ip, kt->ip_nodes * nc * 8, true, kt->ip ? nullptr : "re-grid first"},
    };
    return hx_get_result(kt->ctx, __func__, rows, 3, name, out, out_bytes);
}

}  // extern "C"

// ---- the analytic containers (include/helios_hip.h section 7; the contract is stated in helios_amd/continuum.py) -------------------
//
// k_ktable_continuum: a workgroup takes 256 consecutive bins of one (T, P) row.  Every thread evaluates the opacity of its bin
// once; the tile's 256 * ny values -- each repeated over y -- are contiguous in the container's [t][p][x][y] order and are written
// by the whole workgroup, consecutive lanes to consecutive addresses, as 16-byte stores (one 8-byte store in front or behind where
// the tile does not start or end on 16 bytes).  The kind's coefficients arrive as a device array and are staged in LDS.
namespace {

constexpr int KC_THREADS = 256;
constexpr int KC_MAX_COEF = 304;
constexpr int KC_HE_NT = 12, KC_HE_NX = 22;
constexpr int KC_COEF_BF = 9, KC_COEF_FF = 76, KC_COEF_HE = 4 + KC_HE_NT + KC_HE_NX + KC_HE_NT * KC_HE_NX;

struct KcArgs {
    const double *coef, *wave, *temp, *press;
    double* out;              // the slab: row first_row of the container is its row 0
    int kind, ncoef, nbin, ny, npress, first_row;
};

// H- bound-free: [mass, mu_min, mu_0, C_0 .. C_5]
__device__ double kc_hm_bf(const double* c, double mu) {
    if (mu < c[1] || mu > c[2]) return 0.0;
    const double x = (c[2] - mu) / (mu * c[2]), s = sqrt(x);        // 1/mu - 1/mu_0 without the cancellation
    double f = c[8];
    for (int k = 7; k >= 3; k--) f = f * s + c[k];
    return 1e-18 * (mu * mu * mu) * (x * s) * f / c[0];
}

// H- free-free: [mass, mu_min, mu_split, 5040, then per regime the sets A .. F of six].  Next to 0.3645 micron and at low T the
// terms of the fit cancel to one part in 1e3 ... 1e5, so the sums run in double-double (a value as an unevaluated hi + lo; the
// error of every product comes from an fma, of every sum from the two-sum): the result is rounded once from ~100 bits.
struct kc_dd { double hi, lo; };

__device__ __forceinline__ kc_dd kc_renorm(double s, double e) {
    kc_dd r;
    r.hi = s + e;
    r.lo = e - (r.hi - s);
    return r;
}

__device__ __forceinline__ kc_dd kc_add(kc_dd a, kc_dd b) {
    const double s = a.hi + b.hi, bb = s - a.hi;
    const double e = (a.hi - (s - bb)) + (b.hi - bb);
    return kc_renorm(s, e + (a.lo + b.lo));
}

__device__ __forceinline__ kc_dd kc_mul(kc_dd a, kc_dd b) {
    const double p = a.hi * b.hi;
    const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return kc_renorm(p, e);
}

__device__ __forceinline__ kc_dd kc_of(double v) { kc_dd r; r.hi = v; r.lo = 0.0; return r; }

__device__ __forceinline__ kc_dd kc_div(double a, double b) {          // a / b
    const double q = a / b;
    return kc_renorm(q, fma(-q, b, a) / b);
}

__device__ __forceinline__ kc_dd kc_sqrt(kc_dd a) {
    const double s = sqrt(a.hi);
    return kc_renorm(s, (fma(-s, s, a.hi) + a.lo) / (2.0 * s));
}

__device__ double kc_hm_ff(const double* c, double mu, double T, double P) {
    if (mu < c[1]) return 0.0;
    const double* s = c + 4 + (mu < c[2] ? 0 : 36);
    const kc_dd theta = kc_div(c[3], T), root = kc_sqrt(theta), u = kc_div(1.0, mu), mu2 = kc_mul(kc_of(mu), kc_of(mu));
    kc_dd total = kc_of(0.0);
    for (int n = 5; n >= 0; n--) {
        kc_dd g = kc_of(s[30 + n]);
        for (int term = 24; term >= 6; term -= 6) g = kc_add(kc_mul(g, u), kc_of(s[term + n]));
        g = kc_add(g, kc_mul(mu2, kc_of(s[n])));
        total = kc_add(kc_mul(total, root), g);
    }
    total = kc_mul(theta, total);
    return 1e-29 * (total.hi + total.lo) * P / c[0];
}

// He-: [mass, mu_lo, mu_hi, fill, T nodes, log10 mu nodes, log10 k [t][x]]
__device__ double kc_he(const double* c, double mu, double T, double P) {
    const double *tn = c + 4, *xn = tn + KC_HE_NT, *z = xn + KC_HE_NX;
    double v = c[3];
    if (T >= tn[0] && T <= tn[KC_HE_NT - 1] && mu >= c[1] && mu <= c[2]) {
        const double x = log10(mu);
        int i = 0, j = 0;
        while (i < KC_HE_NT - 2 && tn[i + 1] <= T) i++;
        while (j < KC_HE_NX - 2 && xn[j + 1] <= x) j++;
        const double ft = (T - tn[i]) / (tn[i + 1] - tn[i]), fx = (x - xn[j]) / (xn[j + 1] - xn[j]);
        const double* z0 = z + i * KC_HE_NX + j;
        v = (z0[0] * (1 - ft) + z0[KC_HE_NX] * ft) * (1 - fx) + (z0[1] * (1 - ft) + z0[KC_HE_NX + 1] * ft) * fx;
    }
    return pow(10.0, v) * P / c[0];
}

__launch_bounds__(KC_THREADS) __global__ void k_ktable_continuum(KcArgs A) {
    __shared__ double coef[KC_MAX_COEF];
    __shared__ double val[KC_THREADS];
    const int tid = threadIdx.x;
    for (int k = tid; k < A.ncoef; k += KC_THREADS) coef[k] = A.coef[k];
    __syncthreads();
    const int x0 = blockIdx.x * KC_THREADS, cnt = min(KC_THREADS, A.nbin - x0);
    const int row = A.first_row + blockIdx.y;
    if (tid < cnt) {
        const double T = A.temp[row / A.npress], P = A.press[row % A.npress];
        const double mu = A.wave[x0 + tid] * 1e4;                   // micron, rounded as the contract rounds it
        val[tid] = A.kind == 0 ? kc_hm_bf(coef, mu) : (A.kind == 1 ? kc_hm_ff(coef, mu, T, P) : kc_he(coef, mu, T, P));
    }
    __syncthreads();
    double* dst = A.out + ((size_t)blockIdx.y * A.nbin + x0) * A.ny;
    const int n = cnt * A.ny;
    const int head = ((size_t)dst & 15) ? 1 : 0;
    if (head && tid == 0) dst[0] = val[0];
    const int pairs = (n - head) >> 1;
    for (int q = tid; q < pairs; q += KC_THREADS) {
        const int e = head + 2 * q;
        double2 v;
        v.x = val[e / A.ny];
        v.y = val[(e + 1) / A.ny];
        *reinterpret_cast<double2*>(dst + e) = v;
    }
    if (((n - head) & 1) && tid == 0) dst[n - 1] = val[(n - 1) / A.ny];
}

}  // namespace

extern "C" int hx_continuum_table(hx_context* ctx, int kind, const double* coef, int ncoef, const double* wave, int nbin, int ny,
                                  const double* temp, int ntemp, const double* press, int npress, double* out, int first_row,
                                  int rows) {
    if (!ctx) return HX_E_ARG;
    HX_REQUIRE(ctx, kind >= 0 && kind <= 2, HX_E_ARG, "kind is 0 (H- bound-free), 1 (H- free-free) or 2 (He-)");
    HX_REQUIRE(ctx, ncoef == (kind == 0 ? KC_COEF_BF : (kind == 1 ? KC_COEF_FF : KC_COEF_HE)), HX_E_ARG,
               "the coefficient array has another length than this kind's");
    HX_REQUIRE(ctx, coef && wave && temp && press && out, HX_E_ARG, "null array");
    HX_REQUIRE(ctx, nbin >= 1 && nbin <= (1 << 24) && ny >= 1 && ny <= 65536, HX_E_ARG, "1 ... 2^24 bins, 1 ... 65536 Gauss points");
    HX_REQUIRE(ctx, ntemp >= 1 && npress >= 1 && (long long)ntemp * npress <= (1 << 30), HX_E_ARG, "an empty (T, P) grid");
    HX_REQUIRE(ctx, rows >= 1 && rows <= 65535, HX_E_ARG, "1 ... 65535 rows per call");
    HX_REQUIRE(ctx, first_row >= 0 && (long long)first_row + rows <= (long long)ntemp * npress, HX_E_ARG,
               "the rows reach beyond the (T, P) grid");
    HX_REQUIRE(ctx, ((size_t)out & 7) == 0, HX_E_ARG, "the output is not aligned to 8 bytes");
    KcArgs A;
    A.coef = coef; A.wave = wave; A.temp = temp; A.press = press; A.out = out;
    A.kind = kind; A.ncoef = ncoef; A.nbin = nbin; A.ny = ny; A.npress = npress; A.first_row = first_row;
    k_ktable_continuum<<<dim3((nbin + KC_THREADS - 1) / KC_THREADS, rows), KC_THREADS, 0, ctx->stream>>>(A);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}
