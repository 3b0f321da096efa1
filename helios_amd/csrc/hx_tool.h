// What the objects of the off-line tools (hx_ktable, hx_ktmix, hx_premix, hx_star, hx_mie, hx_lines, hx_cia, hx_exomol, hx_chem) share around their kernels: the list
// of an object's device allocations, an event pair that times a stretch of the stream and is read later, the tail of hx_*_get,
// the rows of a node object (hx_lines, hx_cia, hx_exomol) with the checks of its create, set_nodes, run_nodes, device_ptr and get,
// the rows of the batch object's (hx_rt) named arrays, and the re-gridding of a table onto another (T, P) grid.  The kernels and the
// state of the objects stay with the objects.
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

#include "hx_common.h"

// ---- the device allocations of one object: allocate through the list, and the object's destroy frees what it holds ----------
struct hx_owned {
    std::vector<void*> ptrs;
};

template <class T>
inline int hx_owned_alloc(hx_context* ctx, hx_owned& o, size_t bytes, T** out) {
    void* p = nullptr;
    int rc = hx_alloc(ctx, bytes, &p);
    if (rc) return rc;
    o.ptrs.push_back(p);
    *out = (T*)p;
    return 0;
}

// one allocation before the object goes; null is nothing to free
inline int hx_owned_free(hx_context* ctx, hx_owned& o, void* p) {
    if (!p) return 0;
    o.ptrs.erase(std::remove(o.ptrs.begin(), o.ptrs.end(), p), o.ptrs.end());
    return hx_free(ctx, p);
}

inline void hx_owned_free_all(hx_context* ctx, hx_owned& o) {
    for (void* p : o.ptrs) (void)hx_free(ctx, p);
    o.ptrs.clear();
}

// ---- an event pair around launches on the context's stream.  stop returns at once; settle waits for the second event and adds
// the milliseconds to *acc, so a run may return before its kernels end and the next call on the object settles -------------------
struct hx_stream_timer {
    hipEvent_t ev0, ev1;
    bool pending;
};

inline int hx_stream_timer_create(hx_context* ctx, hx_stream_timer& t) {
    if (hipEventCreate(&t.ev0) != hipSuccess || hipEventCreate(&t.ev1) != hipSuccess)
        return hx_fail(ctx, HX_E_ARG, "hipEventCreate failed");
    return 0;
}

inline void hx_stream_timer_destroy(hx_stream_timer& t) {
    if (t.ev0) (void)hipEventDestroy(t.ev0);
    if (t.ev1) (void)hipEventDestroy(t.ev1);
    t.ev0 = t.ev1 = nullptr;
}

inline int hx_stream_timer_start(hx_context* ctx, hx_stream_timer& t) {
    HX_HIP(ctx, hipEventRecord(t.ev0, ctx->stream));
    return 0;
}

inline int hx_stream_timer_stop(hx_context* ctx, hx_stream_timer& t) {
    HX_HIP(ctx, hipEventRecord(t.ev1, ctx->stream));
    t.pending = true;
    return 0;
}

inline int hx_stream_timer_settle(hx_context* ctx, hx_stream_timer& t, double* acc) {
    if (!t.pending) return 0;
    HX_HIP(ctx, hipEventSynchronize(t.ev1));
    float ms = 0;
    HX_HIP(ctx, hipEventElapsedTime(&ms, t.ev0, t.ev1));
    *acc += ms;
    t.pending = false;
    return 0;
}

// ---- the tail of hx_*_get: the caller fills a row per name it serves from one stretch of memory; names that are made up at the
// call (species_<n>) or gathered from several places stay with the caller ----------------------------------------------------------
struct hx_result {
    const char* name;
    const void* src;
    size_t bytes;
    bool on_device;
    const char* not_ready;      // null, or why the object's state does not hold the result yet (HX_E_STATE)
};

inline int hx_get_result(hx_context* ctx, const char* fn, const hx_result* rows, size_t n_rows, const char* name, void* out,
                         size_t out_bytes) {
    for (size_t k = 0; k < n_rows; k++) {
        const hx_result& r = rows[k];
        if (strcmp(r.name, name) != 0) continue;
        if (r.not_ready) return hx_fail(ctx, HX_E_STATE, "%s: %s", fn, r.not_ready);
        if (r.bytes != out_bytes)
            return hx_fail(ctx, HX_E_ARG, "%s(%s): %zu bytes expected, got %zu", fn, name, r.bytes, out_bytes);
        if (r.on_device) return hx_d2h(ctx, out, r.src, r.bytes);
        if (r.bytes) memcpy(out, r.src, r.bytes);
        return 0;
    }
    return hx_fail(ctx, HX_E_ARG, "%s: unknown name '%s'", fn, name);
}

// ---- the rows of a node object (hx_lines, hx_cia, hx_exomol are one): up to per_launch of the nodes_max nodes of set_nodes per
// run_nodes, into fp32 slabs that stay on the device and, where the handle was made for them, the fp64 rows before rounding.  `fn`
// is the caller's name in a message, `set_fn` that of its set_nodes ---------------------------------------------------------------
struct hx_node_rows {
    int points_max, per_launch, nodes_max;
    bool want_fp64;
    int n_nodes, n_points, rows_run;   // of the last set_nodes; rows the last run_nodes filled
    float* slabs32;                    // [per_launch][points_max], rows run with the stride n_points
    double* kappa64;                   // the same rows before rounding; null without want_fp64
};

struct hx_named_value { const char* name; double v; };

// create: the ranges of the three sizes, which the handle then holds
inline int hx_node_rows_init(hx_context* ctx, const char* fn, hx_node_rows& r, int n_points_max, int nodes_per_launch, int n_nodes_max,
                             int want_fp64) {
    if (n_points_max < 1 || n_points_max > (1 << 30)) return hx_fail(ctx, HX_E_ARG, "%s: 1 ... 2^30 spectral points", fn);
    if (nodes_per_launch < 1 || nodes_per_launch > 65535) return hx_fail(ctx, HX_E_ARG, "%s: 1 ... 65535 nodes per launch", fn);
    if (n_nodes_max < 1 || n_nodes_max > (1 << 24)) return hx_fail(ctx, HX_E_ARG, "%s: 1 ... 2^24 nodes", fn);
    r = {n_points_max, nodes_per_launch, n_nodes_max, want_fp64 != 0, 0, 0, 0, nullptr, nullptr};
    return 0;
}

// create: the slabs and the fp64 rows of a handle whose refusal names the nodes per launch alone
inline int hx_node_rows_alloc(hx_context* ctx, const char* fn, hx_owned& o, hx_node_rows& r) {
    const size_t n = (size_t)r.per_launch * (size_t)r.points_max;
    const char* const refusal = "%s: the %s of %d nodes per launch need %zu bytes, which the device does not give";
    if (hx_owned_alloc(ctx, o, n * 4, &r.slabs32)) return hx_fail(ctx, HX_E_ARG, refusal, fn, "fp32 slabs", r.per_launch, n * 4);
    if (r.want_fp64 && hx_owned_alloc(ctx, o, n * 8, &r.kappa64))
        return hx_fail(ctx, HX_E_ARG, refusal, fn, "fp64 rows", r.per_launch, n * 8);
    return 0;
}

// set_nodes: the two counts against what the handle holds
inline int hx_node_rows_counts(hx_context* ctx, const char* fn, const hx_node_rows& r, int n_nodes, int n_points) {
    if (n_nodes < 1 || n_nodes > r.nodes_max)
        return hx_fail(ctx, HX_E_ARG, "%s: %d nodes, the handle holds 1 ... %d", fn, n_nodes, r.nodes_max);
    if (n_points < 1 || n_points > r.points_max)
        return hx_fail(ctx, HX_E_ARG, "%s: %d spectral points, the handle holds 1 ... %d", fn, n_points, r.points_max);
    return 0;
}

// set_nodes: every value is a finite number > 0; node >= 0: the values are that node's, and the message says so
inline int hx_require_positive(hx_context* ctx, const char* fn, int node, std::initializer_list<hx_named_value> values) {
    for (const hx_named_value& p : values) {
        if (p.v > 0.0 && std::isfinite(p.v)) continue;
        if (node < 0) return hx_fail(ctx, HX_E_ARG, "%s: %s = %g is not a finite number > 0", fn, p.name, p.v);
        return hx_fail(ctx, HX_E_ARG, "%s: node %d: %s = %g is not a finite number > 0", fn, node, p.name, p.v);
    }
    return 0;
}

inline int hx_node_rows_check_run(hx_context* ctx, const char* fn, const char* set_fn, const hx_node_rows& r, int first_node,
                                  int n_nodes) {
    if (r.n_nodes < 1) return hx_fail(ctx, HX_E_STATE, "%s: no nodes (%s)", fn, set_fn);
    if (n_nodes < 1 || n_nodes > r.per_launch)
        return hx_fail(ctx, HX_E_ARG, "%s: %d nodes in one call, the handle holds 1 ... %d per launch", fn, n_nodes, r.per_launch);
    if (first_node < 0 || first_node > r.n_nodes - n_nodes)
        return hx_fail(ctx, HX_E_ARG, "%s: nodes %d ... %d, %s gave 0 ... %d", fn, first_node, first_node + n_nodes - 1, set_fn,
                       r.n_nodes - 1);
    return 0;
}

inline int hx_node_rows_device_ptr(hx_context* ctx, const char* fn, const hx_node_rows& r, const char* name, void** out_dptr) {
    if (strcmp(name, "slabs32") != 0) return hx_fail(ctx, HX_E_ARG, "%s: unknown name '%s'", fn, name);
    *out_dptr = r.slabs32;
    return 0;
}

// get: the rows "slabs32" and "kappa64"; `no_run`: null, or that no nodes have been run; `no_fp64`: what a handle without fp64 rows says
inline hx_result hx_node_rows_slabs32(const hx_node_rows& r, const char* no_run) {
    return {"slabs32", r.slabs32, (size_t)r.rows_run * r.n_points * 4, true, no_run};
}

inline hx_result hx_node_rows_kappa64(const hx_node_rows& r, const char* no_run, const char* no_fp64) {
    return {"kappa64", r.kappa64, (size_t)r.rows_run * r.n_points * 8, true, r.want_fp64 ? no_run : no_fp64};
}

// ---- the same for an object that holds a stretch of memory per column (hx_rt) and serves a name through up to three calls:
// a row per name; hx_find_array looks a name up among the rows that serve `call` ---------------------------------------------
enum : unsigned { HX_GET = 1, HX_SET = 2, HX_PTR = 4, HX_ANY_COL = 8 };   // (HX_ANY_COL: one value for the batch, no column is looked at)
struct hx_column_array {
    const char* name;
    const void* base;           // column 0's first element
    size_t stride, count;       // elements from one column to the next (0: one array for all columns), elements served
    size_t elem;                // bytes per element
    unsigned serves;
    bool on_device;
    const char* not_ready;      // null, or why the object's state does not hold the array yet (HX_E_STATE)

    size_t bytes() const { return count * elem; }
    void* at(int col) const { return (char*)base + (size_t)col * stride * elem; }
};

inline const hx_column_array* hx_find_array(const std::vector<hx_column_array>& rows, const char* name, unsigned call) {
    for (const hx_column_array& r : rows)
        if ((r.serves & call) && strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

// ---- re-gridding (k_ktable_regrid, ktable.hip): a table [nt_old][np_old][nc] onto nt_new x np_new nodes.  The plan names per
// target node the left source node and whether the axis is clamped there; the nodes are T and log10 P -----------------------------
struct hx_regrid_plan {
    int nt_old, np_old, nt_new, np_new;
    const int *t_left, *t_reduced, *p_left, *p_reduced;          // host
    const double *temp_old, *logp_old, *temp_new, *logp_new;     // host
};

// refuses null arrays and a plan that would read beyond the source's nodes; `fn` is the caller's name in the message
extern "C" int hx_internal_regrid_check(hx_context* ctx, const char* fn, const hx_regrid_plan* plan);
// checks the plan, stages it, runs the kernel from k_old into k_new (device, [nt_new][np_new][nc]) and adds its time to *ms
extern "C" int hx_internal_regrid(hx_context* ctx, const char* fn, const hx_regrid_plan* plan, const double* k_old, double* k_new,
                                  size_t nc, double* ms);
