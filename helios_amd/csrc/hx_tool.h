// What the objects of the off-line tools (hx_ktable, hx_ktmix, hx_premix, hx_star, hx_mie, hx_lines, hx_cia, hx_exomol, hx_chem) share around their kernels: the list
// of an object's device allocations, an event pair that times a stretch of the stream and is read later, the tail of hx_*_get,
// the rows of the batch object's (hx_rt) named arrays, and the re-gridding of a table onto another (T, P) grid.  The kernels and the
// state of the objects stay with the objects.
#pragma once
#include <algorithm>
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
