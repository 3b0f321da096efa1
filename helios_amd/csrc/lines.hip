// Line-by-line opacities: Voigt profiles of a resident line list summed onto a spectral grid, per (T, P) node
// (include/helios_hip.h section 11; the contract and the host side are helios_amd/lines.py, the statements one line and one
// point at a time tests/lines_reference.py).
//
//   k_lines_prepare   one thread per line: nu_0', s = S(T) a / sqrt pi, a and y of the node, kept [4][lines].
//   k_lines_sum       a workgroup of LINES_THREADS owns LINES_TILE consecutive points, LINES_PPT per thread; point j of thread t is
//                     tile + j * LINES_THREADS + t, so a wavefront's loads and stores are consecutive.  The host hands the tile the
//                     index range of the lines that can reach it.  The workgroup stages their four numbers through LDS,
//                     LINES_BLOCK lines at a time (every lane reads the same address: a broadcast), and every thread walks the
//                     block in line order, tests the cut-off on nu_0' and adds: a point's sum has the order of the contract, and
//                     there are no atomics.  A block whose every line is beyond |z| = LINES_FAR for the whole tile -- by its
//                     distance to the tile or by its y, a test on the region and the same for the whole workgroup -- takes a loop
//                     that knows the region: the same statements, so the same bits, without the branches.
//   k_lines_voigt     K(x, y) of the sum at given pairs, for the tests.
//   k_lines_prepare_nodes, k_lines_sum_nodes
//                     the same two for several nodes per launch: blockIdx.y is the node, which reads its own record (T, P, Q(T), the
//                     row of its pressure's tile ranges), writes its own plane of params[node][4][lines] and row of fp32 slabs
//                     [node][n_points] -- the layout hx_kt_run_device sorts -- and no fp64.  The statements are the single-node
//                     kernels' own (lines_prepare_line, lines_sum_tile), so a row holds that node's kappa32 to the bit.
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

__global__ __launch_bounds__(256) void k_lines_prepare(int n, size_t stride, const double* __restrict__ nu0,
                                                       const double* __restrict__ s_ref, const double* __restrict__ g_air,
                                                       const double* __restrict__ g_self, const double* __restrict__ e_low,
                                                       const double* __restrict__ n_air, const double* __restrict__ delta,
                                                       double temp, double press, double q_t, double q_ref, double molar_mass,
                                                       double x_self, double* __restrict__ params) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    lines_prepare_line(j, stride, nu0, s_ref, g_air, g_self, e_low, n_air, delta, temp, press, q_t, q_ref, molar_mass, x_self, params);
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

__global__ __launch_bounds__(LINES_THREADS) void k_lines_sum(const int2* __restrict__ tile_lines, const double* __restrict__ params,
                                                             size_t stride, int n_points, double nu_first, double dnu, double cutoff,
                                                             double molar_mass, double* __restrict__ kappa64,
                                                             float* __restrict__ kappa32) {
    lines_sum_tile<true>(tile_lines + blockIdx.x, params, stride, n_points, nu_first, dnu, cutoff, molar_mass, kappa64, kappa32);
}

// tile_lines [pressure][n_tiles], params [node][4][stride], slabs32 [node][n_points].  Five waves per SIMD are k_lines_sum's own
// occupancy; without the bound the compiler spends 101 VGPRs and keeps four
__global__ __launch_bounds__(LINES_THREADS, 5) void k_lines_sum_nodes(const int2* __restrict__ tile_lines, int n_tiles,
                                                                   const LinesNode* __restrict__ nodes,
                                                                   const double* __restrict__ params, size_t stride, int n_points,
                                                                   double nu_first, double dnu, double cutoff, double molar_mass,
                                                                   float* __restrict__ slabs32) {
    const int2* range = tile_lines + (size_t)nodes[blockIdx.y].tile_row * n_tiles + blockIdx.x;
    lines_sum_tile<false>(range, params + (size_t)blockIdx.y * 4 * stride, stride, n_points, nu_first, dnu, cutoff, molar_mass,
                          nullptr, slabs32 + (size_t)blockIdx.y * n_points);
}

}  // namespace

struct hx_lines {
    hx_context* ctx;
    int lines_max, points_max, n_lines, n_points;
    double* in[7];                     // nu0, s_ref, gamma_air, gamma_self, e_low, n_air, delta_air: lines_max each
    double* params;                    // [4][lines_max] of the last node
    double* kappa64;                   // points_max
    float* kappa32;
    int2* tile_lines;                  // per tile of the largest grid
    std::vector<double> nu0;           // host copy: the tiles' line ranges are searched in it
    double max_abs_delta;
    hx_owned owned;
    hx_stream_timer t_prepare, t_sum;
    double timing[2];                  // ms in k_lines_prepare and k_lines_sum, of the last run
    // several nodes per launch (hx_lines_create_nodes); all null and zero in a handle of hx_lines_create
    int per_launch, nodes_max;         // rows of params_nodes and slabs32; records of `nodes`
    int n_nodes, nodes_points, nodes_tiles, rows_run;      // of the last set_nodes; slab rows the last run_nodes filled
    bool nodes_ran_last;               // "timing_ms" is the node runs' since set_nodes
    double* params_nodes;              // [per_launch][4][lines_max]
    float* slabs32;                    // [per_launch][points_max], rows run with the stride nodes_points
    LinesNode* nodes;                  // [nodes_max]
    int2* tile_lines_nodes;            // [distinct pressures][nodes_tiles], grown by set_nodes
    size_t tile_lines_nodes_bytes;
    double nodes_common[6];            // q_ref, molar_mass, x_self, cutoff, nu_first, dnu of set_nodes
    hx_stream_timer t_prepare_nodes, t_sum_nodes;
    double timing_nodes[2];
};

static int lines_settle_nodes(hx_lines* h) {
    int rc = hx_stream_timer_settle(h->ctx, h->t_prepare_nodes, &h->timing_nodes[0]);
    if (!rc) rc = hx_stream_timer_settle(h->ctx, h->t_sum_nodes, &h->timing_nodes[1]);
    return rc;
}

// the values every node shares: hx_lines_run's checks, under the caller's name
static int lines_check_common(hx_context* ctx, const char* fn, double q_ref, double molar_mass, double x_self, double cutoff,
                              double nu_first, double dnu) {
    const struct { const char* name; double v; } positive[] = {{"Q(296)", q_ref}, {"M", molar_mass}, {"cutoff", cutoff}, {"dnu", dnu}};
    for (const auto& p : positive)
        if (!(p.v > 0.0) || !std::isfinite(p.v)) return hx_fail(ctx, HX_E_ARG, "%s: %s = %g is not a finite number > 0", fn, p.name, p.v);
    if (!(x_self >= 0.0 && x_self <= 1.0)) return hx_fail(ctx, HX_E_ARG, "%s: x_self = %g lies outside [0, 1]", fn, x_self);
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "%s: nu of point 0 = %g is not finite", fn, nu_first);
    return 0;
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

// nodes_per_launch = 0: a handle of hx_lines_create
static int lines_create(hx_context* ctx, const char* fn, int n_lines_max, int n_points_max, int nodes_per_launch, int n_nodes_max,
                        hx_lines** out_lines) {
    hx_lines* h = new (std::nothrow) hx_lines();
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->lines_max = n_lines_max;
    h->points_max = n_points_max;
    h->per_launch = nodes_per_launch;
    h->nodes_max = n_nodes_max;
    const size_t nl = (size_t)n_lines_max, np = (size_t)n_points_max, npl = (size_t)nodes_per_launch;
    int rc = 0;
    for (int k = 0; k < 7 && !rc; k++) rc = hx_owned_alloc(ctx, h->owned, nl * 8, &h->in[k]);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, 4 * nl * 8, &h->params);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, np * 8, &h->kappa64);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, np * 4, &h->kappa32);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)hx_cdiv(n_points_max, LINES_TILE) * sizeof(int2), &h->tile_lines);
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_create(ctx, h->t_sum);
    if (!rc && npl) {
        const size_t bytes[3] = {npl * 4 * nl * 8, npl * np * 4, (size_t)n_nodes_max * sizeof(LinesNode)};
        static const char* const what[3] = {"line parameters", "fp32 slabs", "node records"};
        void** where[3] = {(void**)&h->params_nodes, (void**)&h->slabs32, (void**)&h->nodes};
        for (int k = 0; k < 3 && !rc; k++)
            if (hx_owned_alloc(ctx, h->owned, bytes[k], where[k]))
                rc = hx_fail(ctx, HX_E_ARG, "%s: the %s of %d nodes per launch need %zu bytes, which the device does not give", fn,
                             what[k], nodes_per_launch, bytes[k]);
        if (!rc) rc = hx_stream_timer_create(ctx, h->t_prepare_nodes);
        if (!rc) rc = hx_stream_timer_create(ctx, h->t_sum_nodes);
    }
    if (rc) {
        (void)hipGetLastError();         // a refused hipMalloc is not the next launch's error
        hx_lines_destroy(h);
        return rc;
    }
    *out_lines = h;
    return 0;
}

int hx_lines_create(hx_context* ctx, int n_lines_max, int n_points_max, hx_lines** out_lines) {
    if (!ctx || !out_lines) return HX_E_ARG;
    HX_REQUIRE(ctx, n_lines_max >= 1 && n_lines_max <= (1 << 27), HX_E_ARG, "1 ... 2^27 lines");
    HX_REQUIRE(ctx, n_points_max >= 1 && n_points_max <= (1 << 30), HX_E_ARG, "1 ... 2^30 spectral points");
    return lines_create(ctx, __func__, n_lines_max, n_points_max, 0, 0, out_lines);
}

int hx_lines_create_nodes(hx_context* ctx, int n_lines_max, int n_points_max, int nodes_per_launch, int n_nodes_max,
                          hx_lines** out_lines) {
    if (!ctx || !out_lines) return HX_E_ARG;
    HX_REQUIRE(ctx, n_lines_max >= 1 && n_lines_max <= (1 << 27), HX_E_ARG, "1 ... 2^27 lines");
    HX_REQUIRE(ctx, n_points_max >= 1 && n_points_max <= (1 << 30), HX_E_ARG, "1 ... 2^30 spectral points");
    HX_REQUIRE(ctx, nodes_per_launch >= 1 && nodes_per_launch <= 65535, HX_E_ARG, "1 ... 65535 nodes per launch");
    HX_REQUIRE(ctx, n_nodes_max >= 1 && n_nodes_max <= (1 << 24), HX_E_ARG, "1 ... 2^24 nodes");
    return lines_create(ctx, __func__, n_lines_max, n_points_max, nodes_per_launch, n_nodes_max, out_lines);
}

int hx_lines_destroy(hx_lines* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->t_prepare);
    hx_stream_timer_destroy(h->t_sum);
    hx_stream_timer_destroy(h->t_prepare_nodes);
    hx_stream_timer_destroy(h->t_sum_nodes);
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
    h->n_points = 0;
    h->n_nodes = h->rows_run = 0;        // the tile ranges of set_nodes were another list's
    return 0;
}

int hx_lines_run(hx_lines* h, double temp, double press, double q_t, double q_ref, double molar_mass, double x_self,
                 double cutoff, double nu_first, double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_lines < 1) return hx_fail(ctx, HX_E_STATE, "hx_lines_run: no line list (hx_lines_set_lines)");
    if (n_points < 1 || n_points > h->points_max)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_run: %d spectral points, the handle holds 1 ... %d", n_points, h->points_max);
    const struct { const char* name; double v; } positive[] = {{"T", temp}, {"P", press}, {"Q(T)", q_t}, {"Q(296)", q_ref},
                                                               {"M", molar_mass}, {"cutoff", cutoff}, {"dnu", dnu}};
    for (const auto& p : positive)
        if (!(p.v > 0.0) || !std::isfinite(p.v))
            return hx_fail(ctx, HX_E_ARG, "hx_lines_run: %s = %g is not a finite number > 0", p.name, p.v);
    if (!(x_self >= 0.0 && x_self <= 1.0)) return hx_fail(ctx, HX_E_ARG, "hx_lines_run: x_self = %g lies outside [0, 1]", x_self);
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "hx_lines_run: nu of point 0 = %g is not finite", nu_first);

    const int n_tiles = hx_cdiv(n_points, LINES_TILE);
    std::vector<int2> tiles((size_t)n_tiles);
    lines_tile_ranges(h, press, cutoff, nu_first, dnu, n_points, tiles.data());
    int rc = hx_h2d(ctx, h->tile_lines, tiles.data(), tiles.size() * sizeof(int2));
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_prepare);
    if (rc) return rc;
    const size_t stride = (size_t)h->lines_max;
    k_lines_prepare<<<hx_cdiv(h->n_lines, 256), 256, 0, ctx->stream>>>(h->n_lines, stride, h->in[0], h->in[1], h->in[2], h->in[3],
                                                                      h->in[4], h->in[5], h->in[6], temp, press, q_t, q_ref,
                                                                      molar_mass, x_self, h->params);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_prepare);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_sum);
    if (rc) return rc;
    k_lines_sum<<<n_tiles, LINES_THREADS, 0, ctx->stream>>>(h->tile_lines, h->params, stride, n_points, nu_first, dnu, cutoff,
                                                           molar_mass, h->kappa64, h->kappa32);
    HX_LAUNCH_CHECK(ctx);
    h->timing[0] = h->timing[1] = 0.0;  // of this run alone, and it has ended when the call returns
    h->nodes_ran_last = false;
    rc = hx_stream_timer_stop(ctx, h->t_sum);
    if (!rc) rc = hx_stream_timer_settle(ctx, h->t_prepare, &h->timing[0]);
    if (!rc) rc = hx_stream_timer_settle(ctx, h->t_sum, &h->timing[1]);
    if (!rc) h->n_points = n_points;
    return rc;
}

int hx_lines_set_nodes(hx_lines* h, int n_nodes, const double* temp, const double* press, const double* q_t, double q_ref,
                       double molar_mass, double x_self, double cutoff, double nu_first, double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (!h->per_launch) return hx_fail(ctx, HX_E_STATE, "hx_lines_set_nodes: the handle runs one node at a time (hx_lines_create_nodes)");
    if (h->n_lines < 1) return hx_fail(ctx, HX_E_STATE, "hx_lines_set_nodes: no line list (hx_lines_set_lines)");
    HX_REQUIRE(ctx, temp && press && q_t, HX_E_ARG, "null array");
    if (n_nodes < 1 || n_nodes > h->nodes_max)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: %d nodes, the handle holds 1 ... %d", n_nodes, h->nodes_max);
    if (n_points < 1 || n_points > h->points_max)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: %d spectral points, the handle holds 1 ... %d", n_points, h->points_max);
    int rc = lines_check_common(ctx, __func__, q_ref, molar_mass, x_self, cutoff, nu_first, dnu);
    if (rc) return rc;
    for (int k = 0; k < n_nodes; k++) {
        const struct { const char* name; double v; } positive[] = {{"T", temp[k]}, {"P", press[k]}, {"Q(T)", q_t[k]}};
        for (const auto& p : positive)
            if (!(p.v > 0.0) || !std::isfinite(p.v))
                return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: node %d: %s = %g is not a finite number > 0", k, p.name, p.v);
    }
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
    rc = lines_settle_nodes(h);
    const size_t bytes = tiles.size() * sizeof(int2);
    if (!rc && bytes > h->tile_lines_nodes_bytes) {
        rc = hx_owned_free(ctx, h->owned, h->tile_lines_nodes);
        h->tile_lines_nodes = nullptr;
        h->tile_lines_nodes_bytes = 0;
        if (!rc && hx_owned_alloc(ctx, h->owned, bytes, &h->tile_lines_nodes)) {
            (void)hipGetLastError();
            return hx_fail(ctx, HX_E_ARG, "hx_lines_set_nodes: the tile ranges of %zu pressures need %zu bytes, which the device "
                           "does not give", distinct.size(), bytes);
        }
        if (!rc) h->tile_lines_nodes_bytes = bytes;
    }
    // hx_h2d waits for the stream: node runs still queued have read the tables they were queued with
    if (!rc) rc = hx_h2d(ctx, h->tile_lines_nodes, tiles.data(), bytes);
    if (!rc) rc = hx_h2d(ctx, h->nodes, nodes.data(), nodes.size() * sizeof(LinesNode));
    if (rc) return rc;
    const double common[6] = {q_ref, molar_mass, x_self, cutoff, nu_first, dnu};
    memcpy(h->nodes_common, common, sizeof common);
    h->n_nodes = n_nodes;
    h->nodes_points = n_points;
    h->nodes_tiles = n_tiles;
    h->timing_nodes[0] = h->timing_nodes[1] = 0.0;
    return 0;
}

int hx_lines_run_nodes(hx_lines* h, int first_node, int n_nodes) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_nodes < 1) return hx_fail(ctx, HX_E_STATE, "hx_lines_run_nodes: no nodes (hx_lines_set_nodes)");
    if (n_nodes < 1 || n_nodes > h->per_launch)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_run_nodes: %d nodes in one call, the handle holds 1 ... %d per launch", n_nodes,
                       h->per_launch);
    if (first_node < 0 || first_node > h->n_nodes - n_nodes)
        return hx_fail(ctx, HX_E_ARG, "hx_lines_run_nodes: nodes %d ... %d, hx_lines_set_nodes gave 0 ... %d", first_node,
                       first_node + n_nodes - 1, h->n_nodes - 1);
    int rc = lines_settle_nodes(h);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_prepare_nodes);
    if (rc) return rc;
    const size_t stride = (size_t)h->lines_max;
    const double* c = h->nodes_common;   // q_ref, molar_mass, x_self, cutoff, nu_first, dnu
    const LinesInputs in = {h->in[0], h->in[1], h->in[2], h->in[3], h->in[4], h->in[5], h->in[6]};
    const LinesNode* nodes = h->nodes + first_node;
    k_lines_prepare_nodes<<<dim3(hx_cdiv(h->n_lines, 256), n_nodes), 256, 0, ctx->stream>>>(h->n_lines, stride, in, nodes, c[0], c[1],
                                                                                           c[2], h->params_nodes);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_prepare_nodes);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_sum_nodes);
    if (rc) return rc;
    k_lines_sum_nodes<<<dim3(h->nodes_tiles, n_nodes), LINES_THREADS, 0, ctx->stream>>>(h->tile_lines_nodes, h->nodes_tiles, nodes,
                                                                                       h->params_nodes, stride, h->nodes_points, c[4],
                                                                                       c[5], c[3], c[1], h->slabs32);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->t_sum_nodes);
    if (rc) return rc;
    h->rows_run = n_nodes;
    h->nodes_ran_last = true;
    return 0;
}

int hx_lines_device_ptr(hx_lines* h, const char* name, void** out_dptr) {
    if (!h || !name || !out_dptr) return HX_E_ARG;
    if (strcmp(name, "slabs32") != 0) return hx_fail(h->ctx, HX_E_ARG, "hx_lines_device_ptr: unknown name '%s'", name);
    if (!h->slabs32) return hx_fail(h->ctx, HX_E_STATE, "hx_lines_device_ptr: the handle holds no slabs (hx_lines_create_nodes)");
    *out_dptr = h->slabs32;
    return 0;
}

int hx_lines_get(hx_lines* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->per_launch) {
        int rc = lines_settle_nodes(h);
        if (rc) return rc;
    }
    const char* no_run = h->n_points ? nullptr : "no node has been run (hx_lines_run)";
    if (!strcmp(name, "line_params")) {                          // [4][n_lines] out of [4][lines_max]
        const size_t row = (size_t)h->n_lines * 8;
        if (no_run) return hx_fail(ctx, HX_E_STATE, "hx_lines_get: %s", no_run);
        if (out_bytes != 4 * row) return hx_fail(ctx, HX_E_ARG, "hx_lines_get(line_params): %zu bytes expected, got %zu", 4 * row, out_bytes);
        for (int k = 0; k < 4; k++) {
            int rc = hx_d2h(ctx, (char*)out + k * row, h->params + (size_t)k * h->lines_max, row);
            if (rc) return rc;
        }
        return 0;
    }
    const hx_result rows[] = {{"kappa64", h->kappa64, (size_t)h->n_points * 8, true, no_run},
                              {"kappa32", h->kappa32, (size_t)h->n_points * 4, true, no_run},
                              {"slabs32", h->slabs32, (size_t)h->rows_run * h->nodes_points * 4, true,
                               h->rows_run ? nullptr : "no nodes have been run (hx_lines_run_nodes)"},
                              {"timing_ms", h->nodes_ran_last ? h->timing_nodes : h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, rows, 4, name, out, out_bytes);
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
