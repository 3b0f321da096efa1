// Line-by-line opacities: Voigt profiles of a resident line list summed onto a spectral grid, per (T, P) node
// (include/helios_hip.h section 11; the contract and the host side are helios_amd/lines.py, the statements one line and one
// point at a time tests/lines_reference.py).
//
//   k_lines_prepare_nodes
//                     one thread per line and node: nu_0', s = S(T) a / sqrt pi, a and y, kept [node][4][lines].  blockIdx.y is the
//                     node of the launch, which reads its own record (T, P, Q(T), the row of its pressure's tile ranges).
//   k_lines_sum_nodes a workgroup of LINES_THREADS owns LINES_TILE consecutive points of its node's row, LINES_PPT per thread; point j
//                     of thread t is tile + j * LINES_THREADS + t, so a wavefront's loads and stores are consecutive.  The host hands
//                     the tile the index range of the lines that can reach it.  The workgroup stages their four numbers through LDS,
//                     LINES_BLOCK lines at a time (every lane reads the same address: a broadcast), and every thread walks the
//                     block in line order, tests the cut-off on nu_0' and adds: a point's sum has the order of the contract, and
//                     there are no atomics.  A block whose every line is beyond |z| = LINES_FAR for the whole tile -- by its
//                     distance to the tile or by its y, a test on the region and the same for the whole workgroup -- takes a loop
//                     that knows the region: the same statements, so the same bits, without the branches.  It writes the row of
//                     fp32 slabs [node][n_points], the layout hx_kt_run_device sorts.
//   k_lines_sum_nodes_fp64
//                     the same sum for a handle made with want_fp64: the row kappa64 [node][n_points] before rounding as well.
//   k_lines_voigt     K(x, y) of the sum at given pairs, for the tests.
//
// All arithmetic is fp64 without contraction and complex division is written out.  K (lines_k*) and the sum of a tile
// (lines_sum_tile) stand in lines_device.h, which csrc/exomol.hip includes too.
#include "lines_device.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

__global__ __launch_bounds__(256) void k_lines_voigt(int n, const double* __restrict__ x, const double* __restrict__ y,
                                                     double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lines_k(x[i], y[i]);
}

// the seven numbers of the inputs' line j -> its four numbers for one node
__device__ __forceinline__ void lines_prepare_line(int j, size_t stride, const double* __restrict__ nu0,
                                                   const double* __restrict__ s_ref, const double* __restrict__ g_air,
                                                   const double* __restrict__ g_self, const double* __restrict__ e_low,
                                                   const double* __restrict__ n_air, const double* __restrict__ delta,
                                                   double temp, double press, double q_t, double q_ref, double molar_mass,
                                                   double x_self, double* __restrict__ params) {
    const double c2 = LC_H * LC_C / LC_KB;
    const double patm = press / LC_ATM;
    const double v = nu0[j];
    const double s = s_ref[j] * (q_ref / q_t) * exp(-c2 * e_low[j] * (1.0 / temp - 1.0 / LC_TREF)) *
                     (expm1(-c2 * v / temp) / expm1(-c2 * v / LC_TREF));
    const double vp = v + delta[j] * patm;
    const double gamma = pow(LC_TREF / temp, n_air[j]) * patm * (g_air[j] * (1.0 - x_self) + g_self[j] * x_self);
    const double alpha = (vp / LC_C) * sqrt(2.0 * LC_LN2 * LC_NA * LC_KB * temp / molar_mass);
    const double a = sqrt(LC_LN2) / alpha;
    params[j] = vp;
    params[stride + j] = s * a * LC_INV_SQRT_PI;
    params[2 * stride + j] = a;
    params[3 * stride + j] = fmax(a * gamma, LC_YMIN);
}

// what a node of a batch brings of its own; the rest of a node's arguments is the batch's
struct LinesNode {
    double temp, press, q_t;
    int tile_row, unused;              // the row of its pressure in the tile ranges [pressure][tile]
};

struct LinesInputs {
    const double *nu0, *s_ref, *g_air, *g_self, *e_low, *n_air, *delta;
};

__global__ __launch_bounds__(256) void k_lines_prepare_nodes(int n, size_t stride, LinesInputs in,
                                                             const LinesNode* __restrict__ nodes, double q_ref, double molar_mass,
                                                             double x_self, double* __restrict__ params) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const LinesNode node = nodes[blockIdx.y];
    lines_prepare_line(j, stride, in.nu0, in.s_ref, in.g_air, in.g_self, in.e_low, in.n_air, in.delta, node.temp, node.press, node.q_t,
                       q_ref, molar_mass, x_self, params + (size_t)blockIdx.y * 4 * stride);
}

// tile_lines [pressure][n_tiles], params [node][4][stride], slabs32 and kappa64 [node][n_points].  Without the bound of five waves per
// SIMD the compiler spends 101 VGPRs and keeps four
__global__ __launch_bounds__(LINES_THREADS, 5) void k_lines_sum_nodes(const int2* __restrict__ tile_lines, int n_tiles,
                                                                   const LinesNode* __restrict__ nodes,
                                                                   const double* __restrict__ params, size_t stride, int n_points,
                                                                   double nu_first, double dnu, double cutoff, double molar_mass,
                                                                   float* __restrict__ slabs32) {
    const int2* range = tile_lines + (size_t)nodes[blockIdx.y].tile_row * n_tiles + blockIdx.x;
    lines_sum_tile<false>(range, params + (size_t)blockIdx.y * 4 * stride, stride, n_points, nu_first, dnu, cutoff, molar_mass,
                          nullptr, slabs32 + (size_t)blockIdx.y * n_points);
}

// the same bound: with the node's indexing the compiler spends 101 VGPRs here too, where the single-node sum it replaces held 85
__global__ __launch_bounds__(LINES_THREADS, 5) void k_lines_sum_nodes_fp64(const int2* __restrict__ tile_lines, int n_tiles,
                                                                        const LinesNode* __restrict__ nodes,
                                                                     const double* __restrict__ params, size_t stride, int n_points,
                                                                     double nu_first, double dnu, double cutoff, double molar_mass,
                                                                     double* __restrict__ kappa64, float* __restrict__ slabs32) {
    const int2* range = tile_lines + (size_t)nodes[blockIdx.y].tile_row * n_tiles + blockIdx.x;
    lines_sum_tile<true>(range, params + (size_t)blockIdx.y * 4 * stride, stride, n_points, nu_first, dnu, cutoff, molar_mass,
                         kappa64 + (size_t)blockIdx.y * n_points, slabs32 + (size_t)blockIdx.y * n_points);
}

}  // namespace

struct hx_lines : hx_node_rows {
    hx_context* ctx;
    int lines_max, n_lines, n_tiles;   // n_tiles: of the last set_nodes
    double* in[7];                     // nu0, s_ref, gamma_air, gamma_self, e_low, n_air, delta_air: lines_max each
    double* params;                    // [per_launch][4][lines_max]
    LinesNode* nodes;                  // [nodes_max]
    int2* tile_lines;                  // [distinct pressures][n_tiles], grown by set_nodes
    size_t tile_lines_bytes;
    std::vector<double> nu0;           // host copy: the tiles' line ranges are searched in it
    double max_abs_delta;
    double common[6];                  // q_ref, molar_mass, x_self, cutoff, nu_first, dnu of set_nodes
    hx_owned owned;
    hx_stream_timer t_prepare, t_sum;
    double timing[2];                  // ms in k_lines_prepare_nodes and in the sum since set_nodes
};

static int lines_settle(hx_lines* h) {
    int rc = hx_stream_timer_settle(h->ctx, h->t_prepare, &h->timing[0]);
    if (!rc) rc = hx_stream_timer_settle(h->ctx, h->t_sum, &h->timing[1]);
    return rc;
}

// per tile the lines whose nu_0 lies within the cut-off, widened by the largest pressure shift, of the tile's points
static void lines_tile_ranges(const hx_lines* h, double press, double cutoff, double nu_first, double dnu, int n_points, int2* tiles) {
    const int n_tiles = hx_cdiv(n_points, LINES_TILE);
    const double reach = cutoff + h->max_abs_delta * (press / LC_ATM);
    const double widen = reach * (1.0 + 1e-12) + 1e-9;
    for (int t = 0; t < n_tiles; t++) {
        const int first = t * LINES_TILE, last = std::min(first + LINES_TILE, n_points) - 1;
        const double lo = nu_first + (double)first * dnu - widen, hi = nu_first + (double)last * dnu + widen;
        tiles[t].x = (int)(std::lower_bound(h->nu0.begin(), h->nu0.end(), lo) - h->nu0.begin());
        tiles[t].y = (int)(std::upper_bound(h->nu0.begin(), h->nu0.end(), hi) - h->nu0.begin());
    }
}

extern "C" {

int hx_lines_create(hx_context* ctx, int n_lines_max, int n_points_max, int nodes_per_launch, int n_nodes_max, int want_fp64,
                    hx_lines** out_lines) {
    if (!ctx || !out_lines) return HX_E_ARG;
    HX_REQUIRE(ctx, n_lines_max >= 1 && n_lines_max <= (1 << 27), HX_E_ARG, "1 ... 2^27 lines");
    hx_node_rows rows;
    int rc = hx_node_rows_init(ctx, __func__, rows, n_points_max, nodes_per_launch, n_nodes_max, want_fp64);
    if (rc) return rc;
    hx_lines* h = new (std::nothrow) hx_lines{rows};
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->lines_max = n_lines_max;
    const size_t nl = (size_t)n_lines_max;
    for (int k = 0; k < 7 && !rc; k++) rc = hx_owned_alloc(ctx, h->owned, nl * 8, &h->in[k]);
    const size_t bytes[2] = {(size_t)nodes_per_launch * 4 * nl * 8, (size_t)n_nodes_max * sizeof(LinesNode)};
    static const char* const what[2] = {"line parameters", "node records"};
    void** where[2] = {(void**)&h->params, (void**)&h->nodes};
    for (int k = 0; k < 2 && !rc; k++)
        if (hx_owned_alloc(ctx, h->owned, bytes[k], where[k]))
            rc = hx_fail(ctx, HX_E_ARG, "%s: the %s of %d nodes per launch need %zu bytes, which the device does not give", __func__,
                         what[k], nodes_per_launch, bytes[k]);
    if (!rc) rc = hx_node_rows_alloc(ctx, __func__, h->owned, *h);
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_sum);
    if (rc) {
        (void)hipGetLastError();         // a refused hipMalloc is not the next launch's error
        hx_lines_destroy(h);
        return rc;
    }
    *out_lines = h;
    return 0;
}

int hx_lines_destroy(hx_lines* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->t_prepare);
    hx_stream_timer_destroy(h->t_sum);
    delete h;
    return 0;
}

int hx_lines_set_lines(hx_lines* h, int n_lines, const double* nu0, const double* s_ref, const double* gamma_air,
                       const double* gamma_self, const double* e_low, const double* n_air, const double* delta_air) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, nu0 && s_ref && gamma_air && gamma_self && e_low && n_air && delta_air, HX_E_ARG, "null array");
    if (n_lines < 1 || n_lines > h->lines_max)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_set_lines: %d lines, the handle holds 1 ... %d", n_lines, h->lines_max);
    const double* src[7] = {nu0, s_ref, gamma_air, gamma_self, e_low, n_air, delta_air};
    static const char* const names[7] = {"nu0", "s_ref", "gamma_air", "gamma_self", "e_low", "n_air", "delta_air"};
    double max_delta = 0.0;
    for (int j = 0; j < n_lines; j++) {
        for (int k = 0; k < 7; k++)
            if (!std::isfinite(src[k][j]))
                return hx_fail(ctx, HX_E_ARG, "hx_lines_set_lines: line %d: %s = %g is not a finite number", j, names[k], src[k][j]);
        if (!(nu0[j] > 0.0)) return hx_fail(ctx, HX_E_ARG, "hx_lines_set_lines: line %d: nu0 = %g is not > 0", j, nu0[j]);
        if (s_ref[j] < 0.0) return hx_fail(ctx, HX_E_ARG, "hx_lines_set_lines: line %d: s_ref = %g is negative", j, s_ref[j]);
        if (j > 0 && nu0[j] < nu0[j - 1])
            return hx_fail(ctx, HX_E_ARG, "hx_lines_set_lines: line %d: nu0 = %.17g lies below line %d's %.17g: the list is sorted",
                           j, nu0[j], j - 1, nu0[j - 1]);
        max_delta = std::max(max_delta, fabs(delta_air[j]));
    }
    h->n_lines = 0;
    for (int k = 0; k < 7; k++) {
        int rc = hx_h2d(ctx, h->in[k], src[k], (size_t)n_lines * 8);
        if (rc) return rc;
    }
    h->nu0.assign(nu0, nu0 + n_lines);
    h->max_abs_delta = max_delta;
    h->n_lines = n_lines;
    h->n_nodes = h->rows_run = 0;        // the tile ranges of set_nodes were another list's
    return 0;
}

int hx_lines_set_nodes(hx_lines* h, int n_nodes, const double* temp, const double* press, const double* q_t, double q_ref,
                       double molar_mass, double x_self, double cutoff, double nu_first, double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_lines < 1) return hx_fail(ctx, HX_E_STATE, "hx_lines_set_nodes: no line list (hx_lines_set_lines)");
    HX_REQUIRE(ctx, temp && press && q_t, HX_E_ARG, "null array");
    int rc = hx_node_rows_counts(ctx, __func__, *h, n_nodes, n_points);
    if (!rc) rc = hx_require_positive(ctx, __func__, -1, {{"Q(296)", q_ref}, {"M", molar_mass}, {"cutoff", cutoff}, {"dnu", dnu}});
    if (rc) return rc;
    if (!(x_self >= 0.0 && x_self <= 1.0)) return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: x_self = %g lies outside [0, 1]", x_self);
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: nu of point 0 = %g is not finite", nu_first);
    for (int k = 0; k < n_nodes && !rc; k++)
        rc = hx_require_positive(ctx, __func__, k, {{"T", temp[k]}, {"P", press[k]}, {"Q(T)", q_t[k]}});
    if (rc) return rc;
    // the reach of a tile depends on P alone: one row of ranges per distinct pressure
    std::vector<double> distinct(press, press + n_nodes);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const int n_tiles = hx_cdiv(n_points, LINES_TILE);
    std::vector<int2> tiles(distinct.size() * (size_t)n_tiles);
    for (size_t r = 0; r < distinct.size(); r++)
        lines_tile_ranges(h, distinct[r], cutoff, nu_first, dnu, n_points, tiles.data() + r * (size_t)n_tiles);
    std::vector<LinesNode> nodes((size_t)n_nodes);
    for (int k = 0; k < n_nodes; k++) {
        const int row = (int)(std::lower_bound(distinct.begin(), distinct.end(), press[k]) - distinct.begin());
        nodes[k] = {temp[k], press[k], q_t[k], row, 0};
    }
    h->n_nodes = h->rows_run = 0;        // until the new tables are there
    rc = lines_settle(h);
    const size_t bytes = tiles.size() * sizeof(int2);
    if (!rc && bytes > h->tile_lines_bytes) {
        rc = hx_owned_free(ctx, h->owned, h->tile_lines);
        h->tile_lines = nullptr;
        h->tile_lines_bytes = 0;
        if (!rc && hx_owned_alloc(ctx, h->owned, bytes, &h->tile_lines)) {
            (void)hipGetLastError();
            return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: the tile ranges of %zu pressures need %zu bytes, which the device "
                           "does not give", distinct.size(), bytes);
        }
        if (!rc) h->tile_lines_bytes = bytes;
    }
    // hx_h2d waits for the stream: node runs still queued have read the tables they were queued with
    if (!rc) rc = hx_h2d(ctx, h->tile_lines, tiles.data(), bytes);
    if (!rc) rc = hx_h2d(ctx, h->nodes, nodes.data(), nodes.size() * sizeof(LinesNode));
    if (rc) return rc;
    const double common[6] = {q_ref, molar_mass, x_self, cutoff, nu_first, dnu};
    memcpy(h->common, common, sizeof common);
    h->n_nodes = n_nodes;
    h->n_points = n_points;
    h->n_tiles = n_tiles;
    h->timing[0] = h->timing[1] = 0.0;
    return 0;
}

int hx_lines_run_nodes(hx_lines* h, int first_node, int n_nodes) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = hx_node_rows_check_run(ctx, __func__, "hx_lines_set_nodes", *h, first_node, n_nodes);
    if (!rc) rc = lines_settle(h);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_prepare);
    if (rc) return rc;
    const size_t stride = (size_t)h->lines_max;
    const double* c = h->common;         // q_ref, molar_mass, x_self, cutoff, nu_first, dnu
    const LinesInputs in = {h->in[0], h->in[1], h->in[2], h->in[3], h->in[4], h->in[5], h->in[6]};
    const LinesNode* nodes = h->nodes + first_node;
    k_lines_prepare_nodes<<<dim3(hx_cdiv(h->n_lines, 256), n_nodes), 256, 0, ctx->stream>>>(h->n_lines, stride, in, nodes, c[0], c[1],
                                                                                           c[2], h->params);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_sum);
    if (rc) return rc;
    const dim3 grid(h->n_tiles, n_nodes);
    if (h->want_fp64)
        k_lines_sum_nodes_fp64<<<grid, LINES_THREADS, 0, ctx->stream>>>(h->tile_lines, h->n_tiles, nodes, h->params, stride, h->n_points,
                                                                       c[4], c[5], c[3], c[1], h->kappa64, h->slabs32);
    else
        k_lines_sum_nodes<<<grid, LINES_THREADS, 0, ctx->stream>>>(h->tile_lines, h->n_tiles, nodes, h->params, stride, h->n_points, c[4],
                                                                  c[5], c[3], c[1], h->slabs32);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_sum);
    if (rc) return rc;
    h->rows_run = n_nodes;
    return 0;
}

int hx_lines_device_ptr(hx_lines* h, const char* name, void** out_dptr) {
    if (!h || !name || !out_dptr) return HX_E_ARG;
    return hx_node_rows_device_ptr(h->ctx, __func__, *h, name, out_dptr);
}

int hx_lines_get(hx_lines* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = lines_settle(h);
    if (rc) return rc;
    const char* no_run = h->rows_run ? nullptr : "no nodes have been run (hx_lines_run_nodes)";
    if (!strcmp(name, "line_params")) {                          // [rows_run][4][n_lines] out of [per_launch][4][lines_max]
        const size_t row = (size_t)h->n_lines * 8, want = (size_t)h->rows_run * 4 * row;
        if (no_run) return hx_fail(ctx, HX_E_STATE, "hx_lines_get: %s", no_run);
        if (out_bytes != want) return hx_fail(ctx, HX_E_ARG, "hx_lines_get(line_params): %zu bytes expected, got %zu", want, out_bytes);
        for (int k = 0; k < 4 * h->rows_run && !rc; k++) rc = hx_d2h(ctx, (char*)out + k * row, h->params + (size_t)k * h->lines_max, row);
        return rc;
    }
    const hx_result rows[] = {hx_node_rows_slabs32(*h, no_run),
                              hx_node_rows_kappa64(*h, no_run, "the handle keeps no fp64 rows (want_fp64 of hx_lines_create)"),
                              {"timing_ms", h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, rows, 3, name, out, out_bytes);
}

int hx_lines_voigt(hx_context* ctx, int n, const double* x, const double* y, double* out) {
    if (!ctx) return HX_E_ARG;
    HX_REQUIRE(ctx, x && y && out, HX_E_ARG, "null array");
    HX_REQUIRE(ctx, n >= 1 && n <= (1 << 26), HX_E_ARG, "1 ... 2^26 pairs");
    hx_owned owned;
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * 8;
    int rc = hx_owned_alloc(ctx, owned, bytes, &dx);
    if (!rc) rc = hx_owned_alloc(ctx, owned, bytes, &dy);
    if (!rc) rc = hx_owned_alloc(ctx, owned, bytes, &dout);
    if (!rc) rc = hx_h2d(ctx, dx, x, bytes);
    if (!rc) rc = hx_h2d(ctx, dy, y, bytes);
    if (!rc) {
        k_lines_voigt<<<hx_cdiv(n, 256), 256, 0, ctx->stream>>>(n, dx, dy, dout);
        rc = hipGetLastError() == hipSuccess ? 0 : hx_fail(ctx, HX_E_ARG, "hx_lines_voigt: the launch failed");
    }
    if (!rc) rc = hx_d2h(ctx, out, dout, bytes);
    (void)hx_sync(ctx);
    hx_owned_free_all(ctx, owned);
    return rc;
}

}  // extern "C"
