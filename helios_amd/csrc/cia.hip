// Collision-induced absorption: the blocks of a HITRAN CIA file interpolated onto a spectral grid, per (T, P) node
// (include/helios_hip.h section 12; the contract and the host side are helios_amd/cia.py, the statements one point at a time
// tests/cia_reference.py).
//
//   k_cia_nodes   blockIdx.y is the node, blockIdx.x a tile of CIA_TILE consecutive points, CIA_PPT per thread; point j of thread t
//                 is tile + j * CIA_THREADS + t, so a wavefront's stores are consecutive.  The workgroup decides on the tile's first
//                 and last nu which bands the tile meets.  None: it stores zeros.  One: its four wavefronts find, each by one search
//                 in global memory that takes 64 samples per step (cia_count_le_wave: three dependent loads for a block of 10 000
//                 points where a binary search takes fourteen), the index windows of the node's two blocks of that band that the
//                 tile's points can fall into; when both hold at most CIA_WINDOW entries they are staged through LDS and every
//                 thread searches its points inside them.  Windows that do not fit, and tiles that meet several bands, take
//                 cia_sigma_global: the same statements on the whole blocks in global memory.  A search decides on exact
//                 comparisons, so where and how it runs changes no bit.
//
// All arithmetic is fp64 without contraction; nothing here calls libm and nothing is accumulated, so there are no atomics.
#include "hx_tool.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

constexpr int CIA_THREADS = 256;             // cia.py: THREADS, POINTS_PER_THREAD, WINDOW
constexpr int CIA_PPT = 4;
constexpr int CIA_TILE = CIA_THREADS * CIA_PPT;
constexpr int CIA_WINDOW = 256;              // entries of one block's window that LDS holds
static_assert(CIA_THREADS == 4 * 64, "one wavefront per window end");

// phys_const.py
constexpr double CC_KB = 1.380649e-16, CC_NA = 6.02214076e23;

// the resident table: the blocks' nu and k one behind the other, and the bands' ranges band_numin[n] <= nu <= band_numax[n]; where
// a block stands and which band it belongs to is the host's knowledge, which the node records carry
struct CiaTable {
    const double *nu, *k;
    const double *band_numin, *band_numax;
    int n_bands;
};

// what a node takes of one band: sigma = w0 * (the block of n0 points at off0) + w1 * (the block of n1 points at off1), or the
// first block alone where off0 == off1
struct CiaNodeBand {
    int off0, n0, off1, n1;
    double w0, w1;
};

// how many of a[0 ... n - 1], ascending, are <= x
__device__ __forceinline__ int cia_count_le(const double* a, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the same count by a whole wavefront: every step the 64 lanes sample the ends of 64 chunks of the range that is left, and the
// chunk behind the last sample <= x is the next range
__device__ __forceinline__ int cia_count_le_wave(const double* a, int n, double x) {
    const int lane = threadIdx.x & 63;
    int lo = 0, len = n;
    while (len > 0) {
        const int step = (len + 63) >> 6;
        const int idx = lo + (lane + 1) * step - 1;
        const bool le = idx < lo + len && a[idx] <= x;
        const int chunks = __popcll(__ballot(le));       // ascending: the lanes with a sample <= x are the first ones
        const int end = lo + len;
        lo += chunks * step;
        len = min(step - 1, end - lo);
    }
    return lo;
}

// the block's value at x from the n >= 2 entries a, k that hold x's interval; 0 outside first ... last, the block's own ends
__device__ __forceinline__ double cia_block_value(const double* a, const double* k, int n, double first, double last, double x) {
    const int i = min(max(cia_count_le(a, n, x) - 1, 0), n - 2);
    const double d = a[i + 1] - a[i];
    const double u = (x - a[i]) / d, up = (a[i + 1] - x) / d;
    const double v = up * k[i] + u * k[i + 1];
    return (x >= first && x <= last) ? v : 0.0;
}

__device__ __forceinline__ double cia_block_global(const CiaTable& t, int off, int n, double x) {
    return cia_block_value(t.nu + off, t.k + off, n, t.nu[off], t.nu[off + n - 1], x);
}

// sigma at x by searches in global memory: the band that holds x, then the node's blocks of it
__device__ __forceinline__ double cia_sigma_global(const CiaTable& t, const CiaNodeBand* __restrict__ node_bands, double x) {
    for (int b = 0; b < t.n_bands; b++) {
        if (!(x >= t.band_numin[b] && x <= t.band_numax[b])) continue;
        const CiaNodeBand nb = node_bands[b];
        const double v0 = cia_block_global(t, nb.off0, nb.n0, x);
        if (nb.off0 == nb.off1) return v0;
        const double v1 = cia_block_global(t, nb.off1, nb.n1, x);
        return nb.w0 * v0 + nb.w1 * v1;
    }
    return 0.0;
}

// node_bands [node][n_bands], node_factor [node] = P / (K_B T); slabs32 and kappa64 [row][n_points], row = blockIdx.y
template <bool WITH_FP64>
__global__ __launch_bounds__(CIA_THREADS) void k_cia_nodes(CiaTable t, const CiaNodeBand* __restrict__ node_bands,
                                                           const double* __restrict__ node_factor, int first_node, int n_points,
                                                           double nu_first, double dnu, double partner_mass,
                                                           float* __restrict__ slabs32, double* __restrict__ kappa64) {
    __shared__ double s_nu[2][CIA_WINDOW], s_k[2][CIA_WINDOW];
    __shared__ int s_win[4];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x * CIA_TILE;
    const int node = first_node + blockIdx.y;
    const CiaNodeBand* bands = node_bands + (size_t)node * t.n_bands;
    const double factor = node_factor[node];
    float* out32 = slabs32 + (size_t)blockIdx.y * n_points;
    double* out64 = WITH_FP64 ? kappa64 + (size_t)blockIdx.y * n_points : nullptr;

    const double tile_lo = nu_first + (double)tile * dnu;
    const double tile_hi = nu_first + (double)(min(tile + CIA_TILE, n_points) - 1) * dnu;
    int band = 0, met = 0;
    for (int b = t.n_bands - 1; b >= 0; b--)
        if (t.band_numin[b] <= tile_hi && t.band_numax[b] >= tile_lo) {
            band = b;
            met++;
        }

    double nu[CIA_PPT], sigma[CIA_PPT];
#pragma unroll
    for (int j = 0; j < CIA_PPT; j++) {
        nu[j] = nu_first + (double)(tile + j * CIA_THREADS + tid) * dnu;
        sigma[j] = 0.0;
    }

    bool staged = false;
    if (met == 1) {
        const CiaNodeBand nb = bands[band];
        const int off0 = nb.off0, n0 = nb.n0, off1 = nb.off1, n1 = nb.n1;
        {                              // wavefront 0, 1: the first block at the tile's first and last nu; 2, 3: the second
            const int wave = tid >> 6;
            const int off = wave < 2 ? off0 : off1, n = wave < 2 ? n0 : n1;
            const int i = min(max(cia_count_le_wave(t.nu + off, n, (wave & 1) ? tile_hi : tile_lo) - 1, 0), n - 2);
            if ((tid & 63) == 0) s_win[wave] = i + (wave & 1);
        }
        __syncthreads();
        const int lo0 = s_win[0], len0 = s_win[1] - lo0 + 1, lo1 = s_win[2], len1 = s_win[3] - lo1 + 1;
        staged = len0 <= CIA_WINDOW && len1 <= CIA_WINDOW;
        if (staged) {
            const bool two = off0 != off1;
            for (int e = tid; e < len0; e += CIA_THREADS) {
                s_nu[0][e] = t.nu[off0 + lo0 + e];
                s_k[0][e] = t.k[off0 + lo0 + e];
            }
            if (two)
                for (int e = tid; e < len1; e += CIA_THREADS) {
                    s_nu[1][e] = t.nu[off1 + lo1 + e];
                    s_k[1][e] = t.k[off1 + lo1 + e];
                }
            __syncthreads();
            const double numin = t.band_numin[band], numax = t.band_numax[band];
            const double first0 = t.nu[off0], last0 = t.nu[off0 + n0 - 1];
            const double first1 = t.nu[off1], last1 = t.nu[off1 + n1 - 1];
#pragma unroll
            for (int j = 0; j < CIA_PPT; j++) {
                const double x = nu[j];
                if (!(x >= numin && x <= numax)) continue;
                const double v0 = cia_block_value(s_nu[0], s_k[0], len0, first0, last0, x);
                if (two) {
                    const double v1 = cia_block_value(s_nu[1], s_k[1], len1, first1, last1, x);
                    sigma[j] = nb.w0 * v0 + nb.w1 * v1;
                } else {
                    sigma[j] = v0;
                }
            }
        }
    }
    if (met >= 1 && !staged) {
#pragma unroll
        for (int j = 0; j < CIA_PPT; j++)
            if (tile + j * CIA_THREADS + tid < n_points) sigma[j] = cia_sigma_global(t, bands, nu[j]);
    }
#pragma unroll
    for (int j = 0; j < CIA_PPT; j++) {
        const int p = tile + j * CIA_THREADS + tid;
        if (p < n_points) {
            const double k = sigma[j] * factor * CC_NA / partner_mass;
            if (WITH_FP64) out64[p] = k;
            out32[p] = (float)k;
        }
    }
}

}  // namespace

struct hx_cia : hx_node_rows {
    hx_context* ctx;
    int values_max, blocks_max;
    int n_values, n_blocks, n_bands;                 // of the last set_blocks
    double *nu, *k;                                  // values_max
    double *band_numin, *band_numax;                 // blocks_max
    double* node_factor;                             // nodes_max
    CiaNodeBand* node_bands;                         // [n_nodes][n_bands], grown by set_nodes
    size_t node_bands_bytes;
    double common[3];                                // partner mass, nu_first, dnu of set_nodes
    std::vector<int> h_block_off, h_band_first;      // where the blocks stand and which a band holds: set_nodes finds a node's
    std::vector<double> h_block_temp;                // blocks in them
    hx_owned owned;
    hx_stream_timer timer;
    double timing[2];                                // ms in k_cia_nodes and its launches since set_nodes
};

extern "C" {

int hx_cia_create(hx_context* ctx, int n_values_max, int n_blocks_max, int n_points_max, int nodes_per_launch, int n_nodes_max,
                  int with_fp64, hx_cia** out_cia) {
    if (!ctx || !out_cia) return HX_E_ARG;
    HX_REQUIRE(ctx, n_values_max >= 2 && n_values_max <= (1 << 28), HX_E_ARG, "2 ... 2^28 tabulated values");
    HX_REQUIRE(ctx, n_blocks_max >= 1 && n_blocks_max <= n_values_max / 2, HX_E_ARG, "1 ... n_values_max / 2 blocks");
    hx_node_rows rows;
    int rc = hx_node_rows_init(ctx, __func__, rows, n_points_max, nodes_per_launch, n_nodes_max, with_fp64);
    if (rc) return rc;
    hx_cia* h = new (std::nothrow) hx_cia{rows};
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->values_max = n_values_max;
    h->blocks_max = n_blocks_max;
    const size_t nv = (size_t)n_values_max, nb = (size_t)n_blocks_max;
    rc = hx_owned_alloc(ctx, h->owned, nv * 8, &h->nu);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, nv * 8, &h->k);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, nb * 8, &h->band_numin);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, nb * 8, &h->band_numax);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)n_nodes_max * 8, &h->node_factor);
    if (!rc) rc = hx_node_rows_alloc(ctx, __func__, h->owned, *h);
    if (!rc) rc = hx_stream_timer_create(ctx, h->timer);
    if (rc) {
        (void)hipGetLastError();         // a refused hipMalloc is not the next launch's error
        hx_cia_destroy(h);
        return rc;
    }
    *out_cia = h;
    return 0;
}

int hx_cia_destroy(hx_cia* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->timer);
    delete h;
    return 0;
}

int hx_cia_set_blocks(hx_cia* h, int n_blocks, const int* block_off, const double* nu, const double* k, const double* block_temp,
                      int n_bands, const int* band_first, const double* band_numin, const double* band_numax) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, block_off && nu && k && block_temp && band_first && band_numin && band_numax, HX_E_ARG, "null array");
    if (n_blocks < 1 || n_blocks > h->blocks_max)
        return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: %d blocks, the handle holds 1 ... %d", n_blocks, h->blocks_max);
    if (n_bands < 1 || n_bands > n_blocks)
        return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: %d bands of %d blocks", n_bands, n_blocks);
    if (block_off[0] != 0) return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: block 0 starts at %d, not at 0", block_off[0]);
    for (int b = 0; b < n_blocks; b++) {
        const long long n = (long long)block_off[b + 1] - block_off[b];
        if (n < 2 || block_off[b + 1] > h->values_max)
            return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: block %d holds the values %d ... %d: a block has at least 2 points and "
                           "the handle holds %d values", b, block_off[b], block_off[b + 1] - 1, h->values_max);
        if (!(block_temp[b] > 0.0) || !std::isfinite(block_temp[b]))
            return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: block %d: T = %g is not a finite number > 0", b, block_temp[b]);
        for (int i = block_off[b]; i < block_off[b + 1]; i++) {
            if (!std::isfinite(nu[i]) || !std::isfinite(k[i]) || k[i] < 0.0)
                return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: block %d, point %d: nu = %g, k = %g are not finite numbers, k >= 0", b,
                               i - block_off[b], nu[i], k[i]);
            if (i > block_off[b] && !(nu[i] > nu[i - 1]))
                return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: block %d, point %d: nu = %.17g does not lie above %.17g", b,
                               i - block_off[b], nu[i], nu[i - 1]);
        }
    }
    if (band_first[0] != 0 || band_first[n_bands] != n_blocks)
        return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: the bands hold the blocks %d ... %d, not 0 ... %d", band_first[0],
                       band_first[n_bands] - 1, n_blocks - 1);
    for (int n = 0; n < n_bands; n++) {
        if (band_first[n + 1] <= band_first[n]) return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: band %d holds no block", n);
        if (!std::isfinite(band_numin[n]) || !std::isfinite(band_numax[n]) || band_numax[n] < band_numin[n])
            return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: band %d: %g ... %g is no range", n, band_numin[n], band_numax[n]);
        if (n > 0 && !(band_numin[n] > band_numax[n - 1]))
            return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: band %d starts at %.17g, band %d ends at %.17g: bands neither overlap nor "
                           "touch", n, band_numin[n], n - 1, band_numax[n - 1]);
        for (int b = band_first[n] + 1; b < band_first[n + 1]; b++)
            if (!(block_temp[b] > block_temp[b - 1]))
                return hx_fail(ctx, HX_E_ARG, "hx_cia_set_blocks: band %d: block %d at T = %.17g does not lie above %.17g", n, b,
                               block_temp[b], block_temp[b - 1]);
    }
    h->n_blocks = h->n_nodes = h->rows_run = 0;
    const size_t nv = (size_t)block_off[n_blocks];
    int rc = hx_h2d(ctx, h->nu, nu, nv * 8);
    if (!rc) rc = hx_h2d(ctx, h->k, k, nv * 8);
    if (!rc) rc = hx_h2d(ctx, h->band_numin, band_numin, (size_t)n_bands * 8);
    if (!rc) rc = hx_h2d(ctx, h->band_numax, band_numax, (size_t)n_bands * 8);
    if (rc) return rc;
    h->h_block_off.assign(block_off, block_off + n_blocks + 1);
    h->h_band_first.assign(band_first, band_first + n_bands + 1);
    h->h_block_temp.assign(block_temp, block_temp + n_blocks);
    h->n_values = (int)nv;
    h->n_blocks = n_blocks;
    h->n_bands = n_bands;
    return 0;
}

int hx_cia_set_nodes(hx_cia* h, int n_nodes, const double* temp, const double* press, double partner_mass, double nu_first,
                     double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_blocks < 1) return hx_fail(ctx, HX_E_STATE, "hx_cia_set_nodes: no blocks (hx_cia_set_blocks)");
    HX_REQUIRE(ctx, temp && press, HX_E_ARG, "null array");
    int rc = hx_node_rows_counts(ctx, __func__, *h, n_nodes, n_points);
    if (!rc) rc = hx_require_positive(ctx, __func__, -1, {{"M", partner_mass}, {"dnu", dnu}});
    if (rc) return rc;
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "hx_cia_set_nodes: nu of point 0 = %g is not finite", nu_first);
    for (int n = 0; n < n_nodes && !rc; n++) rc = hx_require_positive(ctx, __func__, n, {{"T", temp[n]}, {"P", press[n]}});
    if (rc) return rc;
    // per node and band: constant beyond the band's temperatures, else the two blocks around T with weights from differences
    std::vector<CiaNodeBand> bands((size_t)n_nodes * h->n_bands);
    std::vector<double> factor((size_t)n_nodes);
    for (int n = 0; n < n_nodes; n++) {
        const double T = temp[n];
        factor[n] = press[n] / (CC_KB * T);
        for (int b = 0; b < h->n_bands; b++) {
            const int first = h->h_band_first[b], last = h->h_band_first[b + 1] - 1;
            const double* bt = h->h_block_temp.data();
            CiaNodeBand& nb = bands[(size_t)n * h->n_bands + b];
            int j0, j1;
            nb.w0 = 1.0;
            nb.w1 = 0.0;
            if (T <= bt[first]) {
                j0 = j1 = first;
            } else if (T >= bt[last]) {
                j0 = j1 = last;
            } else {
                j0 = (int)(std::upper_bound(bt + first, bt + last + 1, T) - bt) - 1;
                j1 = j0 + 1;
                const double D = bt[j1] - bt[j0];
                nb.w0 = (bt[j1] - T) / D;
                nb.w1 = (T - bt[j0]) / D;
            }
            const int* off = h->h_block_off.data();
            nb.off0 = off[j0];
            nb.n0 = off[j0 + 1] - off[j0];
            nb.off1 = off[j1];
            nb.n1 = off[j1 + 1] - off[j1];
        }
    }
    h->n_nodes = h->rows_run = 0;        // until the new records are there
    rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    const size_t bytes = bands.size() * sizeof(CiaNodeBand);
    if (!rc && bytes > h->node_bands_bytes) {
        rc = hx_owned_free(ctx, h->owned, h->node_bands);
        h->node_bands = nullptr;
        h->node_bands_bytes = 0;
        if (!rc && hx_owned_alloc(ctx, h->owned, bytes, &h->node_bands)) {
            (void)hipGetLastError();
            return hx_fail(ctx, HX_E_ARG, "hx_cia_set_nodes: the records of %d nodes x %d bands need %zu bytes, which the device does "
                           "not give", n_nodes, h->n_bands, bytes);
        }
        if (!rc) h->node_bands_bytes = bytes;
    }
    // hx_h2d waits for the stream: node runs still queued have read the records they were queued with
    if (!rc) rc = hx_h2d(ctx, h->node_bands, bands.data(), bytes);
    if (!rc) rc = hx_h2d(ctx, h->node_factor, factor.data(), factor.size() * 8);
    if (rc) return rc;
    h->common[0] = partner_mass;
    h->common[1] = nu_first;
    h->common[2] = dnu;
    h->n_nodes = n_nodes;
    h->n_points = n_points;
    h->timing[0] = h->timing[1] = 0.0;
    return 0;
}

int hx_cia_run_nodes(hx_cia* h, int first_node, int n_nodes) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = hx_node_rows_check_run(ctx, __func__, "hx_cia_set_nodes", *h, first_node, n_nodes);
    if (!rc) rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    if (!rc) rc = hx_stream_timer_start(ctx, h->timer);
    if (rc) return rc;
    const CiaTable t = {h->nu, h->k, h->band_numin, h->band_numax, h->n_bands};
    const dim3 grid(hx_cdiv(h->n_points, CIA_TILE), n_nodes);
    if (h->want_fp64)
        k_cia_nodes<true><<<grid, CIA_THREADS, 0, ctx->stream>>>(t, h->node_bands, h->node_factor, first_node, h->n_points, h->common[1],
                                                                 h->common[2], h->common[0], h->slabs32, h->kappa64);
    else
        k_cia_nodes<false><<<grid, CIA_THREADS, 0, ctx->stream>>>(t, h->node_bands, h->node_factor, first_node, h->n_points, h->common[1],
                                                                  h->common[2], h->common[0], h->slabs32, nullptr);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->timer);
    if (rc) return rc;
    h->timing[1] += 1.0;
    h->rows_run = n_nodes;
    return 0;
}

int hx_cia_device_ptr(hx_cia* h, const char* name, void** out_dptr) {
    if (!h || !name || !out_dptr) return HX_E_ARG;
    return hx_node_rows_device_ptr(h->ctx, __func__, *h, name, out_dptr);
}

int hx_cia_get(hx_cia* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    if (rc) return rc;
    const char* no_run = h->rows_run ? nullptr : "no nodes have been run (hx_cia_run_nodes)";
    const hx_result rows[] = {hx_node_rows_slabs32(*h, no_run),
                              hx_node_rows_kappa64(*h, no_run, "the handle keeps no fp64 rows (hx_cia_create, with_fp64)"),
                              {"timing_ms", h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, rows, 3, name, out, out_bytes);
}

}  // extern "C"
