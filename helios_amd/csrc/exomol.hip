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
//   k_exomol_sum      lines_sum_tile (lines_device.h) over the node's own ranges: the bits of k_lines_sum_nodes for the same four numbers.
// With super-lines (hx_exomol_set_superlines) count, scan and prepare give way to:
//   k_exomol_classify S once per transition into the launch row's strengths; strong (S >= S_min and S >= S_sl) and weak (S_min <=
//                     S < S_sl) counted per workgroup.
//   k_exomol_cells    a wavefront per occupied cell of width d: S_c and G_c of the cell's weak transitions, which cells emit a
//                     super-line (a 64-bit mask per wavefront of cells) and how many per workgroup of EXO_B cells.
//   k_exomol_scan     as it is, over the strong and weak counts and over the cells' counts.
//   k_exomol_merge    strong transitions and super-lines to their positions by the key (cell, kind, position).
// k_exomol_ranges then searches with a reach wider by d -- inside a cell a super-line's nu_c may lie above a strong nu_0 -- and
// k_exomol_sum is unchanged.
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

// ---- super-lines: weak transitions (S_min <= S < S_sl) merged per cell of width d, cell = floor(nu_0 / d) ---------------------
// The occupied cells, each cell's first transition and every transition's occupied cell come from the host once per list.

struct ExoCells {
    int n_cells;
    const int* first;                  // [n_cells + 1]: the first transition of occupied cell k; first[n_cells] = n
    const int* id;                     // [n_cells]: floor(nu_0 / d) of the cell's transitions
    const int* of;                     // [n]: the occupied cell of a transition
};

__device__ __forceinline__ double exomol_gamma(const ExoLists& in, const ExoBroad& br, int j, const ExoNode& node) {
    const double pbar = node.press / EXO_BAR;
    const int jx = in.jidx[in.low[j]];
    double sum = 0.0;
    for (int b = 0; b < br.n_b; b++) {
        const double* row = br.table + ((size_t)b * br.n_j + jx) * 2;
        sum = sum + br.x[b] * row[0] * pow(LC_TREF / node.temp, row[1]);
    }
    return pbar * sum;
}

// S of every transition once, to strength [node][stride]; per workgroup the number of strong and of weak transitions, to
// counts [node][2][n_blocks]
__global__ __launch_bounds__(EXO_B) void k_exomol_classify(int n, size_t stride, ExoLists in, const ExoNode* __restrict__ nodes,
                                                           double s_min, double s_sl, int n_blocks, double* __restrict__ strength,
                                                           int* __restrict__ counts) {
    __shared__ int s_w[2][EXO_WAVES];
    const int j = blockIdx.x * EXO_B + threadIdx.x;
    const ExoNode node = nodes[blockIdx.y];
    int strong = 0, weak = 0;
    if (j < n) {
        const double s = exomol_strength(in, j, node.temp, node.q_t);
        strength[(size_t)blockIdx.y * stride + j] = s;
        const int keep = s >= s_min;
        strong = keep && s >= s_sl;
        weak = keep && !strong;
    }
    const unsigned long long ms = __ballot(strong), mw = __ballot(weak);
    if ((threadIdx.x & 63) == 0) {
        s_w[0][threadIdx.x >> 6] = __popcll(ms);
        s_w[1][threadIdx.x >> 6] = __popcll(mw);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < EXO_WAVES; w++) c += s_w[threadIdx.x][w];
        counts[((size_t)blockIdx.y * 2 + threadIdx.x) * n_blocks + blockIdx.x] = c;
    }
}

// A wavefront per occupied cell, 64 cells one after the other per wavefront, so a workgroup covers EXO_B cells: the lanes stride
// through the cell's run of the list, each adds its weak transitions' S and S gamma in list order, and a butterfly of shuffles
// adds the 64 partial sums -- a fixed order, whatever else the launch holds.  Lane i keeps cell i's sums; the wavefront's
// ballot of "holds a weak transition" is the emit mask, its population the workgroup's count.
// sums [node][2][n_cells]: S_c, G_c; masks [node][4 n_cblocks]; counts [node][n_cblocks]
__global__ __launch_bounds__(EXO_B) void k_exomol_cells(ExoCells cells, size_t stride, ExoLists in, ExoBroad br,
                                                        const ExoNode* __restrict__ nodes, double s_min, double s_sl,
                                                        const double* __restrict__ strength, int n_cblocks,
                                                        double* __restrict__ sums, unsigned long long* __restrict__ masks,
                                                        int* __restrict__ counts) {
    __shared__ int s_w[EXO_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ExoNode node = nodes[blockIdx.y];
    const double* s_of = strength + (size_t)blockIdx.y * stride;
    const int base = blockIdx.x * EXO_B + wave * 64;
    double my_s = 0.0, my_g = 0.0;
    int my_emit = 0;
    for (int i = 0; i < 64; i++) {
        const int k = base + i;
        if (k >= cells.n_cells) break;                           // the same for the whole wavefront
        const int first = cells.first[k], last = cells.first[k + 1];
        double ps = 0.0, pg = 0.0;
        int any = 0;
        for (int j = first + lane; j < last; j += 64) {
            const double s = s_of[j];
            if (s >= s_min && !(s >= s_sl)) {
                ps = ps + s;
                pg = pg + s * exomol_gamma(in, br, j, node);
                any = 1;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            ps = ps + __shfl_xor(ps, d);
            pg = pg + __shfl_xor(pg, d);
        }
        const int emit = __ballot(any) != 0ull;
        if (lane == i) {
            my_s = ps;
            my_g = pg;
            my_emit = emit;
        }
    }
    if (base + lane < cells.n_cells) {
        double* out = sums + (size_t)blockIdx.y * 2 * cells.n_cells;
        out[base + lane] = my_s;
        out[cells.n_cells + base + lane] = my_g;
    }
    const unsigned long long m = __ballot(my_emit);
    if (lane == 0) {
        masks[((size_t)blockIdx.y * n_cblocks + blockIdx.x) * EXO_WAVES + wave] = m;
        s_w[wave] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < EXO_WAVES; w++) c += s_w[w];
        counts[(size_t)blockIdx.y * n_cblocks + blockIdx.x] = c;
    }
}

// The node's list by the key (cell, kind, position): a strong transition goes to (strong transitions before it) + (super-lines
// of the cells up to its own); a cell's super-line goes to (strong transitions before the cell's first transition) +
// (super-lines of the cells before it), and the thread of that first transition writes it.  totals [node][2]: strong, weak, and
// n_super [node] are k_exomol_scan's; length [node] receives strong + super-lines, the list's length.
__global__ __launch_bounds__(EXO_B) void k_exomol_merge(int n, size_t stride, ExoLists in, ExoBroad br, ExoCells cells,
                                                        const ExoNode* __restrict__ nodes, double s_min, double s_sl, double step,
                                                        double molar_mass, const double* __restrict__ strength, int n_blocks,
                                                        const int* __restrict__ offsets, int n_cblocks,
                                                        const double* __restrict__ sums,
                                                        const unsigned long long* __restrict__ masks,
                                                        const int* __restrict__ cell_offsets, const int* __restrict__ totals,
                                                        const int* __restrict__ n_super, int* __restrict__ length,
                                                        double* __restrict__ params) {
    __shared__ int s_w[EXO_WAVES];
    const int j = blockIdx.x * EXO_B + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ExoNode node = nodes[blockIdx.y];
    if (j == 0) length[blockIdx.y] = totals[blockIdx.y * 2] + n_super[blockIdx.y];
    double s = 0.0;
    int strong = 0;
    if (j < n) {
        s = strength[(size_t)blockIdx.y * stride + j];
        strong = s >= s_min && s >= s_sl;
    }
    const unsigned long long m = __ballot(strong);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    if (j >= n) return;
    const int k = cells.of[j];
    const bool opens = cells.first[k] == j;
    if (!strong && !opens) return;
    int before = offsets[(size_t)blockIdx.y * 2 * n_blocks + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < EXO_WAVES; w++)
        if (w < wave) before += s_w[w];
    const unsigned long long* mk = masks + (size_t)blockIdx.y * n_cblocks * EXO_WAVES;
    const int kw = k / 64, kb = k / EXO_B;                       // k_exomol_cells: a mask word per 64 cells, a count per EXO_B
    int supers = cell_offsets[(size_t)blockIdx.y * n_cblocks + kb];
    for (int w = kb * EXO_WAVES; w < kw; w++) supers += __popcll(mk[w]);
    const unsigned long long mine = mk[kw];
    supers += __popcll(mine & ((1ull << (k & 63)) - 1ull));
    const int emits = (int)((mine >> (k & 63)) & 1ull);
    const double doppler = sqrt(2.0 * LC_LN2 * LC_NA * LC_KB * node.temp / molar_mass);
    double* p = params + (size_t)blockIdx.y * 4 * stride;
    if (opens && emits) {
        const double* sc = sums + (size_t)blockIdx.y * 2 * cells.n_cells;
        const double s_c = sc[k], g_c = sc[cells.n_cells + k];
        const double gamma = s_c > 0.0 ? g_c / s_c : 0.0;
        const double v = ((double)cells.id[k] + 0.5) * step;
        const double alpha = (v / LC_C) * doppler;
        const double a = sqrt(LC_LN2) / alpha;
        const int pos = before + supers;
        p[pos] = v;
        p[stride + pos] = s_c * a * LC_INV_SQRT_PI;
        p[2 * stride + pos] = a;
        p[3 * stride + pos] = fmax(a * gamma, LC_YMIN);
    }
    if (strong) {
        const double gamma = exomol_gamma(in, br, j, node);
        const double v = in.nu0[j];
        const double alpha = (v / LC_C) * doppler;
        const double a = sqrt(LC_LN2) / alpha;
        const int pos = before + supers + emits;
        p[pos] = v;
        p[stride + pos] = s * a * LC_INV_SQRT_PI;
        p[2 * stride + pos] = a;
        p[3 * stride + pos] = fmax(a * gamma, LC_YMIN);
    }
}

}  // namespace

struct hx_exomol : hx_node_rows {
    hx_context* ctx;
    int states_max, trans_max, broad_max, blocks_max, tiles_max;
    int n_states, max_jidx, n_trans, n_blocks, n_broad, n_jidx, n_tiles;
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
    std::vector<double> host_e;        // set_transitions takes nu_0 = E[up] - E[low] from it
    double common[6];                  // molar_mass, cutoff, s_min, nu_first, dnu, widen of set_nodes
    hx_owned owned;
    hx_stream_timer t_prepare, t_sum;
    double timing[2];                  // ms in count + scan + prepare + ranges and in the sum since set_nodes
    // super-lines (hx_exomol_set_superlines); nothing below is allocated while they are off
    double sl_threshold, sl_step;      // sl_step = 0: off
    int n_cells, n_cblocks;            // occupied cells, and workgroups of EXO_B of them
    int *cell_first, *cell_id;         // [n_cells + 1], [n_cells]
    int* cell_of;                      // trans_max
    double* strength;                  // [per_launch][trans_max]
    int *sl_counts, *sl_offsets;       // [per_launch][2][blocks_max]: strong, weak
    int* sl_totals;                    // [per_launch][2]
    double* cell_sums;                 // [per_launch][2][n_cells]: S_c, G_c
    unsigned long long* cell_masks;    // [per_launch][4 n_cblocks]
    int *cell_counts, *cell_offsets;   // [per_launch][n_cblocks]
    int* n_super;                      // per_launch
    int* list_len;                     // per_launch: strong + super-lines
    int cells_held;                    // the cells the per-cell arrays were allocated for
};

// (strong, weak, super-lines) of the rows of the last launch
static int exomol_superline_counts(hx_exomol* h, std::vector<int>& out) {
    const size_t rows = (size_t)h->rows_run;
    std::vector<int> sw(2 * rows), ns(rows);
    int rc = hx_d2h(h->ctx, sw.data(), h->sl_totals, sw.size() * 4);
    if (!rc) rc = hx_d2h(h->ctx, ns.data(), h->n_super, ns.size() * 4);
    if (rc) return rc;
    out.resize(3 * rows);
    for (size_t r = 0; r < rows; r++) {
        out[3 * r] = sw[2 * r];
        out[3 * r + 1] = sw[2 * r + 1];
        out[3 * r + 2] = ns[r];
    }
    return 0;
}

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
    hx_node_rows rows;
    int rc = hx_node_rows_init(ctx, __func__, rows, n_points_max, nodes_per_launch, n_nodes_max, want_fp64);
    if (rc) return rc;
    hx_exomol* h = new (std::nothrow) hx_exomol{rows};
    if (!h) return hx_fail(ctx, HX_E_ARG, "no host memory");
    h->ctx = ctx;
    h->states_max = n_states_max;
    h->trans_max = n_trans_max;
    h->broad_max = n_broadeners_max;
    h->blocks_max = hx_cdiv(n_trans_max, EXO_B);
    h->tiles_max = hx_cdiv(n_points_max, LINES_TILE);
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
    h->sl_step = h->sl_threshold = 0.0;
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
    h->sl_step = h->sl_threshold = 0.0;                          // the cells were the other list's
    int rc = hx_h2d(ctx, h->up, up, (size_t)n_trans * 4);
    if (!rc) rc = hx_h2d(ctx, h->low, low, (size_t)n_trans * 4);
    if (!rc) rc = hx_h2d(ctx, h->a, a, (size_t)n_trans * 8);
    if (!rc) rc = hx_h2d(ctx, h->nu0, nu0.data(), (size_t)n_trans * 8);
    if (rc) return rc;
    h->n_trans = n_trans;
    h->n_blocks = hx_cdiv(n_trans, EXO_B);
    return 0;
}

int hx_exomol_set_superlines(hx_exomol* h, double s_sl, double step) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_trans < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_superlines: no transitions (hx_exomol_set_transitions)");
    // from here on every return, a refusal included, leaves super-lines off until the call has succeeded, and the nodes dropped:
    // their tile reach was the other step's
    h->n_nodes = h->rows_run = 0;
    h->sl_step = h->sl_threshold = 0.0;
    if (!(s_sl >= 0.0)) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_superlines: S_sl = %g is not a number >= 0", s_sl);
    if (!(step >= 0.0) || !std::isfinite(step))
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_superlines: the step %g is not a finite number > 0, or 0 for none", step);
    if (step == 0.0) return 0;
    const int n = h->n_trans;
    std::vector<double> nu0((size_t)n);
    int rc = hx_d2h(ctx, nu0.data(), h->nu0, nu0.size() * 8);    // waits for the stream: queued launches have read their cells
    if (rc) return rc;
    if (!(nu0[n - 1] / step < 2147483648.0))
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_superlines: the step %.17g puts the largest nu_0 = %.17g into cell %.17g, cells "
                       "are numbered below 2^31", step, nu0[n - 1], std::floor(nu0[n - 1] / step));
    std::vector<int> first, id, of((size_t)n);
    for (int j = 0; j < n; j++) {
        const int c = (int)std::floor(nu0[j] / step);
        if (id.empty() || c != id.back()) {
            id.push_back(c);
            first.push_back(j);
        }
        of[j] = (int)id.size() - 1;
    }
    first.push_back(n);
    const int n_cells = (int)id.size(), ncb = hx_cdiv(n_cells, EXO_B);
    const size_t nt = (size_t)h->trans_max, npl = (size_t)h->per_launch, nb = (size_t)h->blocks_max;
    if (!h->cell_of) {                                           // what does not depend on the number of cells: once per handle
        const struct { const char* what; size_t bytes; void** where; } want[] = {
            {"cell of every transition", nt * 4, (void**)&h->cell_of}, {"strengths", npl * nt * 8, (void**)&h->strength},
            {"class counts", npl * 2 * nb * 4, (void**)&h->sl_counts}, {"class offsets", npl * 2 * nb * 4, (void**)&h->sl_offsets},
            {"class totals", npl * 2 * 4, (void**)&h->sl_totals}, {"super-line counts", npl * 4, (void**)&h->n_super},
            {"list lengths", npl * 4, (void**)&h->list_len}};
        for (const auto& w : want)
            if (!rc && hx_owned_alloc(ctx, h->owned, w.bytes, w.where)) {
                (void)hipGetLastError();
                rc = hx_fail(ctx, HX_E_ARG, "hx_exomol_set_superlines: the %s of %d transitions and %d nodes per launch need %zu bytes, "
                             "which the device does not give", w.what, h->trans_max, h->per_launch, w.bytes);
            }
        if (rc) {                                                // all or nothing
            void* got[] = {h->cell_of, h->strength, h->sl_counts, h->sl_offsets, h->sl_totals, h->n_super, h->list_len};
            for (void* p : got) (void)hx_owned_free(ctx, h->owned, p);
            h->cell_of = nullptr; h->strength = nullptr; h->sl_counts = h->sl_offsets = h->sl_totals = h->n_super = h->list_len = nullptr;
            return rc;
        }
    }
    if (n_cells > h->cells_held) {
        void* old[] = {h->cell_first, h->cell_id, h->cell_sums, h->cell_masks, h->cell_counts, h->cell_offsets};
        for (void* p : old) (void)hx_owned_free(ctx, h->owned, p);
        h->cell_first = h->cell_id = h->cell_counts = h->cell_offsets = nullptr;
        h->cell_sums = nullptr; h->cell_masks = nullptr;
        h->cells_held = 0;
        const size_t nc = (size_t)n_cells, nbc = (size_t)ncb;
        const struct { size_t bytes; void** where; } want[] = {
            {(nc + 1) * 4, (void**)&h->cell_first}, {nc * 4, (void**)&h->cell_id}, {npl * 2 * nc * 8, (void**)&h->cell_sums},
            {npl * nbc * EXO_WAVES * 8, (void**)&h->cell_masks}, {npl * nbc * 4, (void**)&h->cell_counts},
            {npl * nbc * 4, (void**)&h->cell_offsets}};
        for (const auto& w : want)
            if (!rc && hx_owned_alloc(ctx, h->owned, w.bytes, w.where)) {
                (void)hipGetLastError();
                rc = hx_fail(ctx, HX_E_ARG, "hx_exomol_set_superlines: the arrays of %d occupied cells and %d nodes per launch need "
                             "%zu bytes more, which the device does not give", n_cells, h->per_launch, w.bytes);
            }
        if (rc) {
            void* got[] = {h->cell_first, h->cell_id, h->cell_sums, h->cell_masks, h->cell_counts, h->cell_offsets};
            for (void* p : got) (void)hx_owned_free(ctx, h->owned, p);
            h->cell_first = h->cell_id = h->cell_counts = h->cell_offsets = nullptr;
            h->cell_sums = nullptr; h->cell_masks = nullptr;
            return rc;
        }
        h->cells_held = n_cells;
    }
    rc = hx_h2d(ctx, h->cell_first, first.data(), first.size() * 4);
    if (!rc) rc = hx_h2d(ctx, h->cell_id, id.data(), id.size() * 4);
    if (!rc) rc = hx_h2d(ctx, h->cell_of, of.data(), of.size() * 4);
    if (rc) return rc;
    h->n_cells = n_cells;
    h->n_cblocks = ncb;
    h->sl_threshold = s_sl;
    h->sl_step = step;
    return 0;
}

int hx_exomol_set_nodes(hx_exomol* h, int n_nodes, const double* temp, const double* press, const double* q_t, double molar_mass,
                        double cutoff, double s_min, double nu_first, double dnu, int n_points) {
    if (!h) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    if (h->n_trans < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_nodes: no transitions (hx_exomol_set_transitions)");
    if (h->n_broad < 1) return hx_fail(ctx, HX_E_STATE, "hx_exomol_set_nodes: no broadening table (hx_exomol_set_broadening)");
    HX_REQUIRE(ctx, temp && press && q_t, HX_E_ARG, "null array");
    int rc = hx_node_rows_counts(ctx, __func__, *h, n_nodes, n_points);
    if (!rc) rc = hx_require_positive(ctx, __func__, -1, {{"M", molar_mass}, {"cutoff", cutoff}, {"dnu", dnu}});
    if (rc) return rc;
    if (!(s_min >= 0.0) || !std::isfinite(s_min))
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: S_min = %g is not a finite number >= 0", s_min);
    if (!std::isfinite(nu_first)) return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: nu of point 0 = %g is not finite", nu_first);
    if (h->sl_step > cutoff)
        return hx_fail(ctx, HX_E_ARG, "hx_exomol_set_nodes: the super-line step %.17g is greater than the cut-off %.17g", h->sl_step,
                       cutoff);
    std::vector<ExoNode> nodes((size_t)n_nodes);
    for (int k = 0; k < n_nodes && !rc; k++) {
        rc = hx_require_positive(ctx, __func__, k, {{"T", temp[k]}, {"P", press[k]}, {"Q(T)", q_t[k]}});
        nodes[k] = {temp[k], press[k], q_t[k]};
    }
    if (rc) return rc;
    h->n_nodes = h->rows_run = 0;        // until the new records are there
    rc = exomol_settle(h);
    // hx_h2d waits for the stream: node runs still queued have read the records they were queued with
    if (!rc) rc = hx_h2d(ctx, h->nodes, nodes.data(), nodes.size() * sizeof(ExoNode));
    if (rc) return rc;
    // in super-line mode nu ascends only from cell to cell: a tile's reach is wider by the step
    const double common[6] = {molar_mass, cutoff, s_min, nu_first, dnu, cutoff * (1.0 + 1e-12) + 1e-9 + h->sl_step};
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
    int rc = hx_node_rows_check_run(ctx, __func__, "hx_exomol_set_nodes", *h, first_node, n_nodes);
    if (!rc) rc = exomol_settle(h);
    if (!rc) rc = hx_stream_timer_start(ctx, h->t_prepare);
    if (rc) return rc;
    const size_t stride = (size_t)h->trans_max;
    const double molar_mass = h->common[0], cutoff = h->common[1], s_min = h->common[2], nu_first = h->common[3], dnu = h->common[4];
    const ExoLists in = {h->e, h->g, h->jidx, h->up, h->low, h->a, h->nu0};
    const ExoBroad br = {h->n_broad, h->n_jidx, h->bx, h->btable};
    const ExoNode* nodes = h->nodes + first_node;
    const int nb = h->n_blocks, nt = h->n_tiles;
    if (h->sl_step > 0.0) {
        const ExoCells cells = {h->n_cells, h->cell_first, h->cell_id, h->cell_of};
        const int ncb = h->n_cblocks;
        k_exomol_classify<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, stride, in, nodes, s_min, h->sl_threshold, nb,
                                                                       h->strength, h->sl_counts);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_cells<<<dim3(ncb, n_nodes), EXO_B, 0, ctx->stream>>>(cells, stride, in, br, nodes, s_min, h->sl_threshold, h->strength,
                                                                     ncb, h->cell_sums, h->cell_masks, h->cell_counts);
        HX_LAUNCH_CHECK(ctx);
        // rows (node, strong) and (node, weak): of the weak rows only the total is read, for "kept" and "superline_counts"; their
        // offsets come with it from the one launch and nothing reads them
        k_exomol_scan<<<2 * n_nodes, EXO_B, 0, ctx->stream>>>(nb, h->sl_counts, h->sl_offsets, h->sl_totals);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_scan<<<n_nodes, EXO_B, 0, ctx->stream>>>(ncb, h->cell_counts, h->cell_offsets, h->n_super);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_merge<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, stride, in, br, cells, nodes, s_min, h->sl_threshold,
                                                                     h->sl_step, molar_mass, h->strength, nb, h->sl_offsets, ncb,
                                                                     h->cell_sums, h->cell_masks, h->cell_offsets, h->sl_totals,
                                                                     h->n_super, h->list_len, h->params);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_ranges<<<dim3(hx_cdiv(nt, 256), n_nodes), 256, 0, ctx->stream>>>(nt, h->n_points, nu_first, dnu, h->common[5], stride,
                                                                                 h->params, h->list_len, h->ranges);
        HX_LAUNCH_CHECK(ctx);
    } else {
        k_exomol_count<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, in, nodes, s_min, nb, h->counts);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_scan<<<n_nodes, EXO_B, 0, ctx->stream>>>(nb, h->counts, h->offsets, h->kept);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_prepare<<<dim3(nb, n_nodes), EXO_B, 0, ctx->stream>>>(h->n_trans, stride, in, br, nodes, s_min, molar_mass, nb,
                                                                      h->offsets, h->params);
        HX_LAUNCH_CHECK(ctx);
        k_exomol_ranges<<<dim3(hx_cdiv(nt, 256), n_nodes), 256, 0, ctx->stream>>>(nt, h->n_points, nu_first, dnu, h->common[5], stride,
                                                                                 h->params, h->kept, h->ranges);
        HX_LAUNCH_CHECK(ctx);
    }
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
    return hx_node_rows_device_ptr(h->ctx, __func__, *h, name, out_dptr);
}

int hx_exomol_get(hx_exomol* h, const char* name, void* out, size_t out_bytes) {
    if (!h || !name || !out) return HX_E_ARG;
    hx_context* ctx = h->ctx;
    int rc = exomol_settle(h);
    if (rc) return rc;
    const char* no_run = h->rows_run ? nullptr : "no nodes have been run (hx_exomol_run_nodes)";
    const bool superlines = h->sl_step > 0.0;
    if (superlines && (!strcmp(name, "kept") || !strcmp(name, "superline_counts"))) {
        if (no_run) return hx_fail(ctx, HX_E_STATE, "hx_exomol_get: %s", no_run);
        const bool three = name[0] == 's';
        const size_t want = (size_t)h->rows_run * (three ? 3 : 1) * 4;
        if (out_bytes != want) return hx_fail(ctx, HX_E_ARG, "hx_exomol_get(%s): %zu bytes expected, got %zu", name, want, out_bytes);
        std::vector<int> counts;
        rc = exomol_superline_counts(h, counts);
        if (rc) return rc;
        int* dst = (int*)out;
        for (int r = 0; r < h->rows_run; r++) {
            if (three) memcpy(dst + 3 * r, &counts[3 * r], 12);
            else dst[r] = counts[3 * r] + counts[3 * r + 1];     // kept: strong + weak
        }
        return 0;
    }
    if (!strcmp(name, "superline_counts"))
        return hx_fail(ctx, HX_E_STATE, "hx_exomol_get: no super-lines are set (hx_exomol_set_superlines)");
    if (!strcmp(name, "line_params")) {                          // row after row, [4][kept[row]] out of [4][trans_max]
        if (no_run) return hx_fail(ctx, HX_E_STATE, "hx_exomol_get: %s", no_run);
        std::vector<int> kept((size_t)h->rows_run);
        rc = hx_d2h(ctx, kept.data(), superlines ? h->list_len : h->kept, kept.size() * 4);    // the list's length per row
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
        hx_node_rows_slabs32(*h, no_run),
        hx_node_rows_kappa64(*h, no_run, "the handle keeps no fp64 rows (want_fp64 of hx_exomol_create)"),
        {"kept", h->kept, rows * 4, true, no_run},
        {"tile_ranges", h->ranges, rows * h->n_tiles * sizeof(int2), true, no_run},
        {"timing_ms", h->timing, sizeof h->timing, false, nullptr}};
    return hx_get_result(ctx, __func__, results, 5, name, out, out_bytes);
}

}  // extern "C"
