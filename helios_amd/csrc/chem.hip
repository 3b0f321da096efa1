// Equilibrium chemistry of the C-H-O network of Heng & Lyons (2016) and Heng & Tsai (2016): the mixing ratios of H2, He, H2O, CO,
// CH4, CO2, C2H2 and the mean molecular mass per (chemistry, T, P) node (include/helios_hip.h section 14; the contract and the
// host side are helios_amd/chem.py, the statements one node at a time tests/chem_reference.py).
//
//   k_chem_nodes   one thread per node in workgroups of CHEM_THREADS, blockIdx.y is the chemistry (an abundance pair).  The
//                  workgroup stages the Gibbs rows through LDS once; a thread finds its temperature's interval there in a fixed
//                  number of steps, forms the three constants and the quintic's coefficients and bisects between x_min and 2 n_C
//                  on the BIT PATTERNS of the two ends: the doubles >= 0 are ordered like their patterns, so the interval
//                  collapses after at most 63 halvings wherever the root lies, forty orders of magnitude below the bracket
//                  included.  Every lane runs the same CHEM_STEPS steps -- a lane whose interval has collapsed keeps its ends --
//                  so the loop's exit is uniform.  The eight results go to eight planes [n_nodes], node after node.
//
// All arithmetic is fp64 without contraction; exp, sqrt and the divisions are the device library's.  Nothing is accumulated
// across threads, so there are no atomics; the kernel keeps its coefficients in registers and has no private segment.
#include "hx_tool.h"

#include <cmath>
#include <new>

namespace {

constexpr int CHEM_THREADS = 256;            // chem.py: THREADS, MAX_ROWS, PLANES
constexpr int CHEM_MAX_ROWS = 1024;          // Gibbs rows that LDS holds: 4 x 8 KB
constexpr int CHEM_PLANES = 8;               // H2, He, H2O, CO, CH4, CO2, C2H2, mu
constexpr int CHEM_STEPS = 64;               // halvings of a difference of two bit patterns below 2^63

struct ChemWeights {
    double h2, he, h2o, co, ch4, co2, c2h2;
};

// table [4][n_rows]: T, dG1, dG2, dG3; out [chemistry][CHEM_PLANES][n_nodes]
__global__ __launch_bounds__(CHEM_THREADS) void k_chem_nodes(const double* __restrict__ table, int n_rows,
                                                             const double* __restrict__ node_temp,
                                                             const double* __restrict__ node_press, int n_nodes,
                                                             const double* __restrict__ o_abund, const double* __restrict__ c_abund,
                                                             double n_he, double gas_constant, ChemWeights w,
                                                             double* __restrict__ out) {
    __shared__ double s_t[CHEM_MAX_ROWS], s_g1[CHEM_MAX_ROWS], s_g2[CHEM_MAX_ROWS], s_g3[CHEM_MAX_ROWS];
    const int tid = threadIdx.x;
    for (int e = tid; e < n_rows; e += CHEM_THREADS) {
        s_t[e] = table[e];
        s_g1[e] = table[n_rows + e];
        s_g2[e] = table[2 * n_rows + e];
        s_g3[e] = table[3 * n_rows + e];
    }
    __syncthreads();
    const int node = blockIdx.x * CHEM_THREADS + tid;
    if (node >= n_nodes) return;
    const double T = node_temp[node], P = node_press[node];
    const double n_o = o_abund[blockIdx.y], n_c = c_abund[blockIdx.y];

    // the last row at or below T, at most n_rows - 2 (the host refuses T outside the rows): the same steps in every lane
    int top = 1;
    while (2 * top < n_rows) top *= 2;
    int i = 0;
    for (int step = top; step > 0; step >>= 1) {
        const int j = min(i + step, n_rows - 1);
        if (s_t[j] <= T) i = j;
    }
    i = min(i, n_rows - 2);
    const double u = (T - s_t[i]) / (s_t[i + 1] - s_t[i]);
    const double g1 = s_g1[i] + u * (s_g1[i + 1] - s_g1[i]);
    const double g2 = s_g2[i] + u * (s_g2[i + 1] - s_g2[i]);
    const double g3 = s_g3[i] + u * (s_g3[i + 1] - s_g3[i]);
    const double rt = gas_constant * T;
    const double k1 = exp(-g1 / rt) / P / P;
    const double k2 = exp(-g2 / rt);
    const double k3 = exp(-g3 / rt) / P / P;
    const double d = n_o - n_c;

    const double a0 = -2.0 * n_c;
    const double a1 = 8.0 * k1 / k2 * d * d + 1.0 + 2.0 * k1 * d;
    const double a2 = 8.0 * k1 / k2 * d + 2.0 * k3 + k1;
    const double a3 = 2.0 * k1 / k2 * (1.0 + 8.0 * k3 * d) + 2.0 * k1 * k3;
    const double a4 = 8.0 * k1 * k3 / k2;
    const double a5 = 8.0 * k1 * k3 * k3 / k2;

    double x_min = 0.0;
    if (d < 0.0) {
        const double md = -d;
        x_min = 4.0 * md / (1.0 + sqrt(1.0 + 16.0 * k3 * md));
    }
    const double x_max = 2.0 * n_c;
    long long lo = __double_as_longlong(x_min), hi = __double_as_longlong(x_max);
    {
        const double f = ((((a5 * x_max + a4) * x_max + a3) * x_max + a2) * x_max + a1) * x_max + a0;
        if (!(f > 0.0)) lo = hi;             // all methane
    }
    for (int s = 0; s < CHEM_STEPS; s++) {
        const long long mid = lo + ((hi - lo) >> 1);
        const double x = __longlong_as_double(mid);
        const double f = ((((a5 * x + a4) * x + a3) * x + a2) * x + a1) * x + a0;
        if (f < 0.0) lo = mid;
        else hi = mid;
    }
    const double x = __longlong_as_double(hi);

    const double b = 1.0 + k1 * x;
    const double h = 4.0 * n_o / (b + sqrt(b * b + 16.0 * k1 * x * n_o / k2));
    const double co = k1 * x * h;
    const double co2 = co * h / k2;
    const double c2h2 = k3 * x * x;
    const double sum = 1.0 + n_he + h + co + x + co2 + c2h2;
    const double v_h2 = 1.0 / sum, v_he = n_he / sum, v_h2o = h / sum, v_co = co / sum, v_ch4 = x / sum, v_co2 = co2 / sum,
                 v_c2h2 = c2h2 / sum;
    const double mu = v_h2 * w.h2 + v_he * w.he + v_h2o * w.h2o + v_co * w.co + v_ch4 * w.ch4 + v_co2 * w.co2 + v_c2h2 * w.c2h2;

    double* o = out + (size_t)blockIdx.y * CHEM_PLANES * n_nodes + node;
    const size_t plane = (size_t)n_nodes;
    o[0] = v_h2;
    o[plane] = v_he;
    o[2 * plane] = v_h2o;
    o[3 * plane] = v_co;
    o[4 * plane] = v_ch4;
    o[5 * plane] = v_co2;
    o[6 * plane] = v_c2h2;
    o[7 * plane] = mu;
}

}  // namespace

struct hx_chem {
    hx_context* ctx;
    int rows_max, nodes_max, chem_max;
    int n_rows, n_nodes, n_chem;                     // of the last set_table, set_nodes, run
    double t_first, t_last, gas_constant;            // of the last set_table
    double* table;                                   // [4][rows_max], rows run with the stride n_rows
    double *node_temp, *node_press;                  // nodes_max
    double *o_abund, *c_abund;                       // chem_max
    double* vmr;                                     // [chem_max][8][nodes_max], run with the strides of n_nodes
    hx_owned owned;
    hx_stream_timer timer;
    double timing[2];                                // ms in k_chem_nodes and its launches since set_nodes
};

extern "C" {

int hx_chem_create(hx_context* ctx, int max_rows, int max_nodes, int max_chem, hx_chem** out_chem) {
    if (!ctx || !out_chem) return HX_E_ARG;
    if (max_rows < 2 || max_rows > CHEM_MAX_ROWS)
        return hx_fail(ctx, HX_E_ARG, "hx_chem_create: %d Gibbs rows, the kernel stages 2 ... %d", max_rows, CHEM_MAX_ROWS);
    HX_REQUIRE(ctx, max_nodes >= 1 && max_nodes <= (1 << 24), HX_E_ARG, "1 ... 2^24 nodes");
    HX_REQUIRE(ctx, max_chem >= 1 && max_chem <= 65535, HX_E_ARG, "1 ... 65535 chemistries per launch");
    hx_chem* h = new (std::nothrow) hx_chem();
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->rows_max = max_rows;
    h->nodes_max = max_nodes;
    h->chem_max = max_chem;
    const size_t out_bytes = (size_t)max_chem * CHEM_PLANES * (size_t)max_nodes * 8;
    int rc = hx_owned_alloc(ctx, h->owned, (size_t)4 * max_rows * 8, &h->table);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)max_nodes * 8, &h->node_temp);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)max_nodes * 8, &h->node_press);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)max_chem * 8, &h->o_abund);
    if (!rc) rc = hx_owned_alloc(ctx, h->owned, (size_t)max_chem * 8, &h->c_abund);
    if (!rc && hx_owned_alloc(ctx, h->owned, out_bytes, &h->vmr))
        rc = hx_fail(ctx, HX_E_ARG, "hx_chem_create: the results of %d chemistries x %d nodes need %zu bytes, which the device does "
                     "not give", max_chem, max_nodes, out_bytes);
    if (!rc) rc = hx_stream_timer_create(ctx, h->timer);
    if (rc) {
        (void)hipGetLastError();         // a refused hipMalloc is not the next launch's error
        hx_chem_destroy(h);
        return rc;
    }
    *out_chem = h;
    return 0;
}

int hx_chem_destroy(hx_chem* h) {
    if (!h) return HX_E_ARG;
    (void)hx_sync(h->ctx);
    hx_owned_free_all(h->ctx, h->owned);
    hx_stream_timer_destroy(h->timer);
    delete h;
    return 0;
}

int hx_chem_set_table(hx_chem* h, int n_rows, const double* temp, const double* dg1, const double* dg2, const double* dg3,
                      double gas_constant) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    HX_REQUIRE(ctx, temp && dg1 && dg2 && dg3, HX_E_ARG, "null array");
    if (n_rows < 2 || n_rows > h->rows_max)
        return hx_fail(ctx, HX_E_ARG, "hx_chem_set_table: %d Gibbs rows, the handle holds 2 ... %d", n_rows, h->rows_max);
    if (!(gas_constant > 0.0) || !std::isfinite(gas_constant))
        return hx_fail(ctx, HX_E_ARG, "hx_chem_set_table: the gas constant %g is not a finite number > 0", gas_constant);
    for (int r = 0; r < n_rows; r++) {
        if (!std::isfinite(temp[r]) || !std::isfinite(dg1[r]) || !std::isfinite(dg2[r]) || !std::isfinite(dg3[r]) || !(temp[r] > 0.0))
            return hx_fail(ctx, HX_E_ARG, "hx_chem_set_table: row %d: T = %g, dG = %g, %g, %g are not finite numbers, T > 0", r, temp[r],
                           dg1[r], dg2[r], dg3[r]);
        if (r > 0 && !(temp[r] > temp[r - 1]))
            return hx_fail(ctx, HX_E_ARG, "hx_chem_set_table: row %d: T = %.17g does not lie above %.17g", r, temp[r], temp[r - 1]);
    }
    h->n_rows = h->n_nodes = h->n_chem = 0;          // nodes were checked against the rows that go
    const size_t bytes = (size_t)n_rows * 8;
    int rc = hx_h2d(ctx, h->table, temp, bytes);
    if (!rc) rc = hx_h2d(ctx, h->table + n_rows, dg1, bytes);
    if (!rc) rc = hx_h2d(ctx, h->table + 2 * (size_t)n_rows, dg2, bytes);
    if (!rc) rc = hx_h2d(ctx, h->table + 3 * (size_t)n_rows, dg3, bytes);
    if (rc) return rc;
    h->n_rows = n_rows;
    h->t_first = temp[0];
    h->t_last = temp[n_rows - 1];
    h->gas_constant = gas_constant;
    return 0;
}

int hx_chem_set_nodes(hx_chem* h, int n_nodes, const double* temp, const double* press_bar) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_rows < 2) return hx_fail(ctx, HX_E_STATE, "hx_chem_set_nodes: no Gibbs rows (hx_chem_set_table)");
    HX_REQUIRE(ctx, temp && press_bar, HX_E_ARG, "null array");
    if (n_nodes < 1 || n_nodes > h->nodes_max)
        return hx_fail(ctx, HX_E_ARG, "hx_chem_set_nodes: %d nodes, the handle holds 1 ... %d", n_nodes, h->nodes_max);
    for (int n = 0; n < n_nodes; n++) {
        if (!(temp[n] >= h->t_first && temp[n] <= h->t_last))
            return hx_fail(ctx, HX_E_ARG, "hx_chem_set_nodes: node %d: T = %.17g lies outside the Gibbs rows %.17g ... %.17g", n, temp[n],
                           h->t_first, h->t_last);
        if (!(press_bar[n] > 0.0) || !std::isfinite(press_bar[n]))
            return hx_fail(ctx, HX_E_ARG, "hx_chem_set_nodes: node %d: P = %g is not a finite number > 0", n, press_bar[n]);
    }
    h->n_nodes = h->n_chem = 0;
    int rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    // hx_h2d waits for the stream: a run still queued has read the nodes it was queued with
    if (!rc) rc = hx_h2d(ctx, h->node_temp, temp, (size_t)n_nodes * 8);
    if (!rc) rc = hx_h2d(ctx, h->node_press, press_bar, (size_t)n_nodes * 8);
    if (rc) return rc;
    h->n_nodes = n_nodes;
    h->timing[0] = h->timing[1] = 0.0;
    return 0;
}

int hx_chem_run(hx_chem* h, int n_chem, const double* o_abund, const double* c_abund, double he_to_h, const double* weights) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_nodes < 1) return hx_fail(ctx, HX_E_STATE, "hx_chem_run: no nodes (hx_chem_set_nodes)");
    h->n_chem = 0;                       // a refused run leaves no result to take for its own
    HX_REQUIRE(ctx, o_abund && c_abund && weights, HX_E_ARG, "null array");
    if (n_chem < 1 || n_chem > h->chem_max)
        return hx_fail(ctx, HX_E_ARG, "hx_chem_run: %d chemistries, the handle holds 1 ... %d", n_chem, h->chem_max);
    for (int c = 0; c < n_chem; c++) {
        const struct { const char* name; double v; } ab[] = {{"n_O", o_abund[c]}, {"n_C", c_abund[c]}};
        for (const auto& a : ab)
            if (!(a.v > 0.0) || !std::isfinite(a.v))
                return hx_fail(ctx, HX_E_ARG, "hx_chem_run: chemistry %d: %s = %g is not a finite number > 0", c, a.name, a.v);
    }
    if (!(he_to_h >= 0.0) || !std::isfinite(he_to_h))
        return hx_fail(ctx, HX_E_ARG, "hx_chem_run: He/H = %g is not a finite number >= 0", he_to_h);
    for (int s = 0; s < 7; s++)
        if (!(weights[s] > 0.0) || !std::isfinite(weights[s]))
            return hx_fail(ctx, HX_E_ARG, "hx_chem_run: weight %d = %g is not a finite number > 0", s, weights[s]);
    int rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    if (!rc) rc = hx_h2d(ctx, h->o_abund, o_abund, (size_t)n_chem * 8);
    if (!rc) rc = hx_h2d(ctx, h->c_abund, c_abund, (size_t)n_chem * 8);
    if (!rc) rc = hx_stream_timer_start(ctx, h->timer);
    if (rc) return rc;
    const ChemWeights w = {weights[0], weights[1], weights[2], weights[3], weights[4], weights[5], weights[6]};
    const dim3 grid(hx_cdiv(h->n_nodes, CHEM_THREADS), n_chem);
    k_chem_nodes<<<grid, CHEM_THREADS, 0, ctx->stream>>>(h->table, h->n_rows, h->node_temp, h->node_press, h->n_nodes, h->o_abund,
                                                         h->c_abund, 2.0 * he_to_h, h->gas_constant, w, h->vmr);
    HX_LAUNCH_CHECK(ctx);
    rc = hx_stream_timer_stop(ctx, h->timer);
    if (rc) return rc;
    h->timing[1] += 1.0;
    h->n_chem = n_chem;
    return 0;
}

int hx_chem_get(hx_chem* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = hx_stream_timer_settle(ctx, h->timer, &h->timing[0]);
    if (rc) return rc;
    const hx_result rows[] = {{"vmr", h->vmr, (size_t)h->n_chem * CHEM_PLANES * (size_t)h->n_nodes * 8, true,
                               h->n_chem ? nullptr : "no chemistry has been run (hx_chem_run)"},
                              {"timing_ms", h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, rows, 2, name, out, out_bytes);
}

}  // extern "C"
