// Opacities from an ExoMol line list: a state table, transitions (upper, lower, A) and broadening per J'', cut by strength at
// the node's temperature and summed as csrc/lines.hip sums (include/helios_hip.h section 13; the contract and the host side are
// helios_amd/exomol.py, the statements one transition at a time tests/exomol_reference.py).
//
// Per launch of up to nodes_per_launch nodes, blockIdx.y the node, everything on the context's stream:
//   k_exomol_count    one thread per transition: gathers E'' and g' of its states, evaluates S(T) by the contract's statement and
//                     flags S >= S_min; a workgroup of EXO_B leaves the number of its flags.
//   k_exomol_scan     one workgroup per node walks the node's block counts, EXO_B at a time: an exclusive scan (shuffles inside a
//                     wavefront, LDS across the four, a carry from chunk to chunk) and the node's total.  No atomics: the
//                     offsets are the same in every run.
//   k_exomol_prepare  the same statement, so the same flag; a kept transition's position is its block's offset plus the number
//                     of kept lanes before it, and nu_0, s, a, y go to that position of the node's params [4][n_trans_max]: the
//                     kept transitions in list order.
//   k_exomol_ranges   one thread per tile: lower and upper bound of the tile's reach in the node's compacted nu_0 (ascending,
//                     there is no pressure shift), widened as lines_tile_ranges widens.
//   k_exomol_sum      lines_sum_tile (lines_device.h) over the node's own ranges: the bits of k_lines_sum for the same four numbers.
#include "lines_device.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

constexpr int EXO_B = 256;                   // exomol.py: COMPACT_BLOCK
constexpr int EXO_WAVES = EXO_B / 64;
constexpr double EXO_PI = 3.141592653589793;
constexpr double EXO_BAR = 1.0e6;            // dyne cm^-2: ExoMol's reference pressure
constexpr int EXO_JIDX_MAX = 1 << 20;

struct ExoNode {
    double temp, press, q_t;
};

struct ExoLists {
    const double *e, *g;               // per state
    const int* jidx;
    const int *up, *low;               // per transition, 0-based
    const double *a, *nu0;
};

struct ExoBroad {
    int n_b, n_j;
    const double* x;                   // [n_b]
    const double* table;               // [n_b][n_j][gamma, n]
};

__device__ __forceinline__ double exomol_strength(const ExoLists& in, int j, double temp, double q_t) {
    const double c2 = LC_H * LC_C / LC_KB;
    const double v = in.nu0[j];
    const double pre = in.g[in.up[j]] * in.a[j] / (8.0 * EXO_PI * LC_C * v * v);
    return pre * exp(-c2 * in.e[in.low[j]] / temp) * (-expm1(-c2 * v / temp)) / q_t;
}

__global__ __launch_bounds__(EXO_B) void k_exomol_count(int n, ExoLists in, const ExoNode* __restrict__ nodes, double s_min,
                                                        int n_blocks, int* __restrict__ counts) {
    __shared__ int s_w[EXO_WAVES];
    const int j = blockIdx.x * EXO_B + threadIdx.x;
    const ExoNode node = nodes[blockIdx.y];
    int keep = 0;
    if (j < n) keep = exomol_strength(in, j, node.temp, node.q_t) >= s_min;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < EXO_WAVES; w++) c += s_w[w];
        counts[(size_t)blockIdx.y * n_blocks + blockIdx.x] = c;
    }
}

// counts, offsets [node][n_blocks]; kept [node]
__global__ __launch_bounds__(EXO_B) void k_exomol_scan(int n_blocks, const int* __restrict__ counts, int* __restrict__ offsets,
                                                       int* __restrict__ kept) {
    __shared__ int s_w[EXO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* c = counts + (size_t)blockIdx.x * n_blocks;
    int* o = offsets + (size_t)blockIdx.x * n_blocks;
    int carry = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += EXO_B) {
        const int i = b0 + tid;
        const int v = i < n_blocks ? c[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < EXO_WAVES; w++) {
            const int t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < n_blocks) o[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();                                         // s_w is the next chunk's
    }
    if (tid == 0) kept[blockIdx.x] = carry;
}

__global__ __launch_bounds__(EXO_B) void k_exomol_prepare(int n, size_t stride, ExoLists in, ExoBroad br,
                                                          const ExoNode* __restrict__ nodes, double s_min, double molar_mass,
                                                          int n_blocks, const int* __restrict__ offsets,
                                                          double* __restrict__ params) {
    __shared__ int s_w[EXO_WAVES];
    const int j = blockIdx.x * EXO_B + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ExoNode node = nodes[blockIdx.y];
    double strength = 0.0;
    int keep = 0;
    if (j < n) {
        strength = exomol_strength(in, j, node.temp, node.q_t);
        keep = strength >= s_min;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int pos = offsets[(size_t)blockIdx.y * n_blocks + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < EXO_WAVES; w++)
        if (w < wave) pos += s_w[w];
    const double pbar = node.press / EXO_BAR;
    const double v = in.nu0[j];
    const int jx = in.jidx[in.low[j]];
    double sum = 0.0;
    for (int b = 0; b < br.n_b; b++) {
        const double* row = br.table + ((size_t)b * br.n_j + jx) * 2;
        sum = sum + br.x[b] * row[0] * pow(LC_TREF / node.temp, row[1]);
    }
    const double gamma = pbar * sum;
    const double alpha = (v / LC_C) * sqrt(2.0 * LC_LN2 * LC_NA * LC_KB * node.temp / molar_mass);
    const double a = sqrt(LC_LN2) / alpha;
    double* p = params + (size_t)blockIdx.y * 4 * stride;
    p[pos] = v;
    p[stride + pos] = strength * a * LC_INV_SQRT_PI;
    p[2 * stride + pos] = a;
    p[3 * stride + pos] = fmax(a * gamma, LC_YMIN);
}

// ranges [node][n_tiles]: the kept transitions whose nu_0 lies within `widen` of the tile's points
__global__ __launch_bounds__(256) void k_exomol_ranges(int n_tiles, int n_points, double nu_first, double dnu, double widen,
                                                       size_t stride, const double* __restrict__ params,
                                                       const int* __restrict__ kept, int2* __restrict__ ranges) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tiles) return;
    const double* nu = params + (size_t)blockIdx.y * 4 * stride;
    const int n = kept[blockIdx.y];
    const int first = t * LINES_TILE, last = min(first + LINES_TILE, n_points) - 1;
    const double lo = nu_first + (double)first * dnu - widen, hi = nu_first + (double)last * dnu + widen;
    int a = 0, b = n;                                            // the first index with nu >= lo
    while (a < b) {
        const int mid = a + (b - a) / 2;
        if (nu[mid] < lo) a = mid + 1; else b = mid;
    }
    int c = a, d = n;                                            // the first index with nu > hi
    while (c < d) {
        const int mid = c + (d - c) / 2;
        if (nu[mid] <= hi) c = mid + 1; else d = mid;
    }
    ranges[(size_t)blockIdx.y * n_tiles + t] = make_int2(a, c);
}

// ranges [node][n_tiles], params [node][4][stride], slabs32 and kappa64 [node][n_points].  Five waves per SIMD as k_lines_sum_nodes
__global__ __launch_bounds__(LINES_THREADS, 5) void k_exomol_sum(const int2* __restrict__ ranges, int n_tiles,
                                                              const double* __restrict__ params, size_t stride, int n_points,
                                                              double nu_first, double dnu, double cutoff, double molar_mass,
                                                              float* __restrict__ slabs32) {
    lines_sum_tile<false>(ranges + (size_t)blockIdx.y * n_tiles + blockIdx.x, params + (size_t)blockIdx.y * 4 * stride, stride,
                          n_points, nu_first, dnu, cutoff, molar_mass, nullptr, slabs32 + (size_t)blockIdx.y * n_points);
}

__global__ __launch_bounds__(LINES_THREADS) void k_exomol_sum_fp64(const int2* __restrict__ ranges, int n_tiles,
                                                                  const double* __restrict__ params, size_t stride, int n_points,
                                                                  double nu_first, double dnu, double cutoff, double molar_mass,
                                                                  double* __restrict__ kappa64, float* __restrict__ slabs32) {
    lines_sum_tile<true>(ranges + (size_t)blockIdx.y * n_tiles + blockIdx.x, params + (size_t)blockIdx.y * 4 * stride, stride,
                         n_points, nu_first, dnu, cutoff, molar_mass, kappa64 + (size_t)blockIdx.y * n_points,
                         slabs32 + (size_t)blockIdx.y * n_points);
}

}  // namespace

struct hx_exomol {
    hx_context* ctx;
    int states_max, trans_max, broad_max, points_max, per_launch, nodes_max, blocks_max, tiles_max;
    bool want_fp64;
    int n_states, max_jidx, n_trans, n_blocks, n_broad, n_jidx;
    int n_nodes, n_points, n_tiles, rows_run;
    double *e, *g;                     // states_max
    int* jidx;
    int *up, *low;                     // trans_max, sorted by (nu_0, position)
    double *a, *nu0;
    double* bx;                        // broad_max
    double* btable;                    // [n_broad][n_jidx][2], grown by set_broadening
    size_t btable_bytes;
    ExoNode* nodes;                    // nodes_max
    double* params;                    // [per_launch][4][trans_max]
    int *counts, *offsets;             // [per_launch][blocks_max]
    int* kept;                         // per_launch
    int2* ranges;                      // [per_launch][tiles_max], rows run with the stride n_tiles
    float* slabs32;                    // [per_launch][points_max], rows run with the stride n_points
    double* kappa64;                   // the same, want_fp64 only
    std::vector<double> host_e;        // set_transitions takes nu_0 = E[up] - E[low] from it
    double common[6];                  // molar_mass, cutoff, s_min, nu_first, dnu, widen of set_nodes
    hx_owned owned;
    hx_stream_timer t_prepare, t_sum;
    double timing[2];                  // ms in count + scan + prepare + ranges and in the sum since set_nodes
};

static int exomol_settle(hx_exomol* h) {
    int rc = hx_stream_timer_settle(h->ctx, h->t_prepare, &h->timing[0]);
    if (!rc) rc = hx_stream_timer_settle(h->ctx, h->t_sum, &h->timing[1]);
    return rc;
}

extern "C" {

int hx_exomol_create(hx_context* ctx, int n_states_max, int n_trans_max, int n_broadeners_max, int n_points_max,
                     int nodes_per_launch, int n_nodes_max, int want_fp64, hx_exomol** out_exomol) {
    if (!ctx || !out_exomol) return HX_E_ARG;
    HX_REQUIRE(ctx, n_states_max >= 1 && n_states_max <= (1 << 27), HX_E_ARG, "1 ... 2^27 states");
    HX_REQUIRE(ctx, n_trans_max >= 1 && n_trans_max <= (1 << 27), HX_E_ARG, "1 ... 2^27 transitions");
    HX_REQUIRE(ctx, n_broadeners_max >= 1 && n_broadeners_max <= 64, HX_E_ARG, "1 ... 64 broadeners");
    HX_REQUIRE(ctx, n_points_max >= 1 && n_points_max <= (1 << 30), HX_E_ARG, "1 ... 2^30 spectral points");
    HX_REQUIRE(ctx, nodes_per_launch >= 1 && nodes_per_launch <= 65535, HX_E_ARG, "1 ... 65535 nodes per launch");
    HX_REQUIRE(ctx, n_nodes_max >= 1 && n_nodes_max <= (1 << 24), HX_E_ARG, "1 ... 2^24 nodes");
    hx_exomol* h = new (std::nothrow) hx_exomol();
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->states_max = n_states_max;
    h->trans_max = n_trans_max;
    h->broad_max = n_broadeners_max;
    h->points_max = n_points_max;
    h->per_launch = nodes_per_launch;
    h->nodes_max = n_nodes_max;
    h->blocks_max = hx_cdiv(n_trans_max, EXO_B);
    h->tiles_max = hx_cdiv(n_points_max, LINES_TILE);
    h->want_fp64 = want_fp64 != 0;
    const size_t ns = (size_t)n_states_max, nt = (size_t)n_trans_max, np = (size_t)n_points_max, npl = (size_t)nodes_per_launch;
    const size_t nb = (size_t)h->blocks_max;
    const struct { const char* what; size_t bytes; void** where; } want[] = {
        {"state energies", ns * 8, (void**)&h->e}, {"state degeneracies", ns * 8, (void**)&h->g},
        {"state J indices", ns * 4, (void**)&h->jidx}, {"upper ids", nt * 4, (void**)&h->up}, {"lower ids", nt * 4, (void**)&h->low},
        {"Einstein coefficients", nt * 8, (void**)&h->a}, {"wavenumbers", nt * 8, (void**)&h->nu0},
        {"broadener fractions", (size_t)n_broadeners_max * 8, (void**)&h->bx},
        {"node records", (size_t)n_nodes_max * sizeof(ExoNode), (void**)&h->nodes},
        {"line parameters", npl * 4 * nt * 8, (void**)&h->params}, {"block counts", npl * nb * 4, (void**)&h->counts},
        {"block offsets", npl * nb * 4, (void**)&h->offsets}, {"kept counts", npl * 4, (void**)&h->kept},
        {"tile ranges", npl * (size_t)h->tiles_max * sizeof(int2), (void**)&h->ranges}, {"fp32 slabs", npl * np * 4, (void**)&h->slabs32},
        {"fp64 rows", h->want_fp64 ? npl * np * 8 : 0, (void**)&h->kappa64}};
    int rc = 0;
    for (const auto& w : want) {
        if (rc || !w.bytes) continue;
        if (hx_owned_alloc(ctx, h->owned, w.bytes, w.where))
            rc = hx_fail(ctx, HX_E_ARG, "hx_exomol_create: the %s of %d transitions, %d points and %d nodes per launch need %zu bytes, "
                         "which the device does not give", w.what, n_trans_max, n_points_max, nodes_per_launch, w.bytes);
    }
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_sum);
    if (rc) {
        (void)hipGetLastError();         // a refused hipMalloc is not the next launch's error
        hx_exomol_destroy(h);
        return rc;
    }
    *out_exomol = h;
    return 0;
}

int hx_exomol_destroy(hx_exomol* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->t_prepare);
    hx_stream_timer_destroy(h->t_sum);
    delete h;
    return 0;
}

int hx_exomol_set_states(hx_exomol* h, int n_states, const double* energy, const double* g, const int* jidx) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, energy && g && jidx, HX_E_ARG, "null array");
    if (n_states < 1 || n_states > h->states_max)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_states: %d states, the handle holds 1 ... %d", n_states, h->states_max);
    int max_jidx = 0;
    for (int k = 0; k < n_states; k++) {
        if (!std::isfinite(energy[k])) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_states: state %d: E = %g is not a finite number", k, energy[k]);
        if (!std::isfinite(g[k]) || g[k] < 0.0) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_states: state %d: g = %g is not a finite number >= 0", k, g[k]);
        if (jidx[k] < 0 || jidx[k] > EXO_JIDX_MAX)
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_states: state %d: 2 J = %d lies outside 0 ... %d", k, jidx[k], EXO_JIDX_MAX);
        max_jidx = std::max(max_jidx, jidx[k]);
    }
    h->n_states = h->n_trans = h->n_broad = h->n_nodes = h->rows_run = 0;      // the lists and the table were another table's
    int rc = hx_h2d(ctx, h->e, energy, (size_t)n_states * 8);
    if (!rc) rc = hx_h2d(ctx, h->g, g, (size_t)n_states * 8);
    if (!rc) rc = hx_h2d(ctx, h->jidx, jidx, (size_t)n_states * 4);
    if (rc) return rc;
    h->host_e.assign(energy, energy + n_states);
    h->n_states = n_states;
    h->max_jidx = max_jidx;
    return 0;
}

int hx_exomol_set_broadening(hx_exomol* h, int n_broadeners, int n_jidx, const double* fraction, const double* table) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, fraction && table, HX_E_ARG, "null array");
    if (h->n_states < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_broadening: no states (hx_exomol_set_states)");
    if (n_broadeners < 1 || n_broadeners > h->broad_max)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_broadening: %d broadeners, the handle holds 1 ... %d", n_broadeners, h->broad_max);
    if (n_jidx != h->max_jidx + 1)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_broadening: %d rows per broadener, the states' largest 2 J = %d needs %d", n_jidx,
                       h->max_jidx, h->max_jidx + 1);
    for (int b = 0; b < n_broadeners; b++) {
        if (!(fraction[b] > 0.0) || !std::isfinite(fraction[b]))
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_broadening: broadener %d: fraction = %g is not a finite number > 0", b, fraction[b]);
        for (int j = 0; j < n_jidx; j++) {
            const double gamma = table[((size_t)b * n_jidx + j) * 2], n = table[((size_t)b * n_jidx + j) * 2 + 1];
            if (!std::isfinite(gamma) || gamma < 0.0 || !std::isfinite(n))
                return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_broadening: broadener %d, 2 J = %d: gamma = %g, n = %g: gamma is a finite "
                               "number >= 0 and n is finite", b, j, gamma, n);
        }
    }
    h->n_broad = h->n_nodes = h->rows_run = 0;
    const size_t bytes = (size_t)n_broadeners * n_jidx * 2 * 8;
    int rc = 0;
    if (bytes > h->btable_bytes) {
        rc = hx_sync(ctx);               // launches still queued read the table they were queued with
        if (!rc) rc = hx_owned_free(ctx, h->owned, h->btable);
        h->btable = nullptr;
        h->btable_bytes = 0;
        if (!rc && hx_owned_alloc(ctx, h->owned, bytes, &h->btable)) {
            (void)hipGetLastError();
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_broadening: the table of %d broadeners x %d rows needs %zu bytes, which the "
                           "device does not give", n_broadeners, n_jidx, bytes);
        }
        if (!rc) h->btable_bytes = bytes;
    }
    if (!rc) rc = hx_h2d(ctx, h->bx, fraction, (size_t)n_broadeners * 8);
    if (!rc) rc = hx_h2d(ctx, h->btable, table, bytes);
    if (rc) return rc;
    h->n_broad = n_broadeners;
    h->n_jidx = n_jidx;
    return 0;
}

int hx_exomol_set_transitions(hx_exomol* h, int n_trans, const int* up, const int* low, const double* a) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, up && low && a, HX_E_ARG, "null array");
    if (h->n_states < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_transitions: no states (hx_exomol_set_states)");
    if (n_trans < 1 || n_trans > h->trans_max)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_transitions: %d transitions, the handle holds 1 ... %d", n_trans, h->trans_max);
    std::vector<double> nu0((size_t)n_trans);
    for (int j = 0; j < n_trans; j++) {
        if (up[j] < 0 || up[j] >= h->n_states || low[j] < 0 || low[j] >= h->n_states)
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_transitions: transition %d: states %d -> %d, the table holds 0 ... %d", j, up[j],
                           low[j], h->n_states - 1);
        if (!std::isfinite(a[j]) || a[j] < 0.0)
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_transitions: transition %d: A = %g is not a finite number >= 0", j, a[j]);
        nu0[j] = h->host_e[up[j]] - h->host_e[low[j]];
        if (!(nu0[j] > 0.0)) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_transitions: transition %d: nu_0 = %g is not > 0", j, nu0[j]);
        if (j > 0 && nu0[j] < nu0[j - 1])
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_transitions: transition %d: nu_0 = %.17g lies below transition %d's %.17g: the "
                           "list is sorted", j, nu0[j], j - 1, nu0[j - 1]);
    }
    h->n_trans = h->n_nodes = h->rows_run = 0;
    int rc = hx_h2d(ctx, h->up, up, (size_t)n_trans * 4);
    if (!rc) rc = hx_h2d(ctx, h->low, low, (size_t)n_trans * 4);
    if (!rc) rc = hx_h2d(ctx, h->a, a, (size_t)n_trans * 8);
    if (!rc) rc = hx_h2d(ctx, h->nu0, nu0.data(), (size_t)n_trans * 8);
    if (rc) return rc;
    h->n_trans = n_trans;
    h->n_blocks = hx_cdiv(n_trans, EXO_B);
    return 0;
}

int hx_exomol_set_nodes(hx_exomol* h, int n_nodes, const double* temp, const double* press, const double* q_t, double molar_mass,
                        double cutoff, double s_min, double nu_first, double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_trans < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_nodes: no transitions (hx_exomol_set_transitions)");
    if (h->n_broad < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_nodes: no broadening table (hx_exomol_set_broadening)");
    HX_REQUIRE(ctx, temp && press && q_t, HX_E_ARG, "null array");
    if (n_nodes < 1 || n_nodes > h->nodes_max)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: %d nodes, the handle holds 1 ... %d", n_nodes, h->nodes_max);
    if (n_points < 1 || n_points > h->points_max)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: %d spectral points, the handle holds 1 ... %d", n_points, h->points_max);
    const struct { const char* name; double v; } positive[] = {{"M", molar_mass}, {"cutoff", cutoff}, {"dnu", dnu}};
    for (const auto& p : positive)
        if (!(p.v > 0.0) || !std::isfinite(p.v))
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: %s = %g is not a finite number > 0", p.name, p.v);
    if (!(s_min >= 0.0) || !std::isfinite(s_min))
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: S_min = %g is not a finite number >= 0", s_min);
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: nu of point 0 = %g is not finite", nu_first);
    std::vector<ExoNode> nodes((size_t)n_nodes);
    for (int k = 0; k < n_nodes; k++) {
        const struct { const char* name; double v; } node[] = {{"T", temp[k]}, {"P", press[k]}, {"Q(T)", q_t[k]}};
        for (const auto& p : node)
            if (!(p.v > 0.0) || !std::isfinite(p.v))
                return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: node %d: %s = %g is not a finite number > 0", k, p.name, p.v);
        nodes[k] = {temp[k], press[k], q_t[k]};
    }
    h->n_nodes = h->rows_run = 0;        // until the new records are there
    int rc = exomol_settle(h);
    // hx_h2d waits for the stream: node runs still queued have read the records they were queued with
    if (!rc) rc = hx_h2d(ctx, h->nodes, nodes.data(), nodes.size() * sizeof(ExoNode));
    if (rc) return rc;
    const double common[6] = {molar_mass, cutoff, s_min, nu_first, dnu, cutoff * (1.0 + 1e-12) + 1e-9};
    memcpy(h->common, common, sizeof common);
    h->n_nodes = n_nodes;
    h->n_points = n_points;
    h->n_tiles = hx_cdiv(n_points, LINES_TILE);
    h->timing[0] = h->timing[1] = 0.0;
    return 0;
}

int hx_exomol_run_nodes(hx_exomol* h, int first_node, int n_nodes) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_nodes < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_run_nodes: no nodes (hx_exomol_set_nodes)");
    if (n_nodes < 1 || n_nodes > h->per_launch)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_run_nodes: %d nodes in one call, the handle holds 1 ... %d per launch", n_nodes,
                       h->per_launch);
    if (first_node < 0 || first_node > h->n_nodes - n_nodes)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_run_nodes: nodes %d ... %d, hx_exomol_set_nodes gave 0 ... %d", first_node,
                       first_node + n_nodes - 1, h->n_nodes - 1);
    int rc = exomol_settle(h);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_prepare);
    if (rc) return rc;
    const size_t stride = (size_t)h->trans_max;
    const double molar_mass = h->common[0], cutoff = h->common[1], s_min = h->common[2], nu_first = h->common[3], dnu = h->common[4];
    const ExoLists in = {h->e, h->g, h->jidx, h->up, h->low, h->a, h->nu0};
    const ExoBroad br = {h->n_broad, h->n_jidx, h->bx, h->btable};
    const ExoNode* nodes = h->nodes + first_node;
    const int nb = h->n_blocks, nt = h->n_tiles;
    k_exomol_count<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, in, nodes, s_min, nb, h->counts);
    HX_LAUNCH_CHECK(ctx);
    k_exomol_scan<<<n_nodes, EXO_B, 0, ctx->stream>>>(nb, h->counts, h->offsets, h->kept);
    HX_LAUNCH_CHECK(ctx);
    k_exomol_prepare<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, stride, in, br, nodes, s_min, molar_mass, nb, h->offsets,
                                                                  h->params);
    HX_LAUNCH_CHECK(ctx);
    k_exomol_ranges<<<dim3(hx_cdiv(nt, 256), n_nodes), 256, 0, ctx->stream>>>(nt, h->n_points, nu_first, dnu, h->common[5], stride,
                                                                             h->params, h->kept, h->ranges);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_sum);
    if (rc) return rc;
    if (h->want_fp64)
        k_exomol_sum_fp64<<<dim3(nt, n_nodes), LINES_THREADS, 0, ctx->stream>>>(h->ranges, nt, h->params, stride, h->n_points, nu_first,
                                                                               dnu, cutoff, molar_mass, h->kappa64, h->slabs32);
    else
        k_exomol_sum<<<dim3(nt, n_nodes), LINES_THREADS, 0, ctx->stream>>>(h->ranges, nt, h->params, stride, h->n_points, nu_first, dnu,
                                                                          cutoff, molar_mass, h->slabs32);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_sum);
    if (rc) return rc;
    h->rows_run = n_nodes;
    return 0;
}

int hx_exomol_device_ptr(hx_exomol* h, const char* name, void** out_dptr) {
    if (!h || !name || !out_dptr) return HX_E_ARG;
    if (strcmp(name, "slabs32") != 0) return hx_fail(h->ctx, HX_E_ARG, "hx_exomol_device_ptr: unknown name '%s'", name);
    *out_dptr = h->slabs32;
    return 0;
}

int hx_exomol_get(hx_exomol* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = exomol_settle(h);
    if (rc) return rc;
    const char* no_run = h->rows_run ? nullptr : "no nodes have been run (hx_exomol_run_nodes)";
    if (!strcmp(name, "line_params")) {                          // row after row, [4][kept[row]] out of [4][trans_max]
        if (no_run) return hx_fail(ctx, HX_E_STATE, "hx_exomol_get: %s", no_run);
        std::vector<int> kept((size_t)h->rows_run);
        rc = hx_d2h(ctx, kept.data(), h->kept, kept.size() * 4);
        if (rc) return rc;
        size_t total = 0;
        for (int k : kept) total += (size_t)k;
        if (out_bytes != 4 * total * 8)
            return hx_fail(ctx, HX_E_ARG, "hx_exomol_get(line_params): %zu bytes expected, got %zu", 4 * total * 8, out_bytes);
        char* dst = (char*)out;
        for (int r = 0; r < h->rows_run; r++)
            for (int k = 0; k < 4 && kept[r]; k++) {
                rc = hx_d2h(ctx, dst, h->params + ((size_t)r * 4 + k) * h->trans_max, (size_t)kept[r] * 8);
                if (rc) return rc;
                dst += (size_t)kept[r] * 8;
            }
        return 0;
    }
    const size_t rows = (size_t)h->rows_run;
    const hx_result results[] = {
        {"slabs32", h->slabs32, rows * h->n_points * 4, true, no_run},
        {"kappa64", h->kappa64, rows * h->n_points * 8, true,
         h->want_fp64 ? no_run : "the handle keeps no fp64 rows (want_fp64 of hx_exomol_create)"},
        {"kept", h->kept, rows * 4, true, no_run},
        {"tile_ranges", h->ranges, rows * h->n_tiles * sizeof(int2), true, no_run},
        {"timing_ms", h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, results, 5, name, out, out_bytes);
}

}  // extern "C"
