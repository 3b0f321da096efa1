// Random-overlap mixing for ANY number of Gauss points 2 <= ny <= 20: add_to_mixed_opac (kernels.cu:3283-3397) with
// 20 -> ny, 400 -> ny^2, 399 -> ny^2 - 1 and 19 -> ny - 1, for ONE wavefront per problem -- the general companion of ro::mix
// (random_overlap.h), which stays the mixer of ny == 20.
//
// Shared with ro::mix: the 512-position network, the 32-bit keys q(K) << TB | cell code (i << 5 | j, crossing bit 10: they
// ascend with the reference's fill order for any ny <= 32) and their decoding, the wave scan; the same exact fp64 finish --
// so the permutation is exactly the reference's stable one here too.  ro::mix's own functions are not parametrised for
// this: its kernels are held to a register budget (tests/test_abi.py) that any change to them moves.  Different:
//
//  * Position p = 8 lane + slot holds cell (p / ny, p % ny) of the tableau; HIGH padding (inf + inf, weight 0 x 0) follows
//    behind ny^2, and there is no low padding: rank w sits at position w.
//  * None of the shortcuts of the 16 + 4 run layout.  What the layout gives for nothing is kept: the network is entered
//    behind the phases that sort inside a row where a row is a block of it (two ascending curves, ny = 2, 4, 8, 16: a row
//    ascends in its keys for either fill order), it ends with the phase whose blocks hold all ny^2 sums (256 positions for
//    ny <= 16, 128 for ny <= 11, 64 for ny <= 8: every later block is padding), and it is skipped where the rows of the
//    tableau do not overlap (the sums ascend in fill order).
//  * The Gauss points find their interval by a plain binary search over the ranks 1 ... ny^2 - 1.
#pragma once
#include "random_overlap.h"

namespace ro {

// returns ny: what a caller hands to mix_ny
__device__ __forceinline__ int init_ny(Shared& sh, int lane, int ny, const double* gauss_weight, const double* gauss_y) {
    if (lane < NTAB) {
        const bool real = lane < ny;
        const double hw = real ? 0.5 * gauss_weight[lane] : 0.0;
        sh.tab[lane].ohw = sh.tab[lane].ihw = hw;
        if (!real) sh.tab[lane].ov = sh.tab[lane].iv = __builtin_inf();
        if (real) sh.gy[lane] = gauss_y[lane];
    }
    return ny;
}

// keys of the cells (p / ny, p % ny), p = 8 lane + slot: q clamped into the key's field, as in fill_any
template <bool CROSSING>
__device__ __forceinline__ void fill_cells(const Shared& sh, int lane, Keys& v, int ny, int n, int yx, int hmin, int sh_bits) {
    constexpr int TB = CROSSING ? 11 : 10;
    const unsigned qmax = (1u << (32 - TB)) - 1u;
    const unsigned inv_ny = (1048576u + ny - 1) / ny;   // e / ny = e * inv_ny >> 20, exact below 512 for ny <= 20
#pragma unroll
    for (int r = 0; r < SLOTS; r++) {
        const int e = SLOTS * lane + r;
        unsigned key = HIGHKEY;
        if (e < n) {
            const int i = (int)(__umul24(e, inv_ny) >> 20), j = e - ny * i;
            const double K = sh.tab[i].ov + sh.tab[j].iv;
            const int dh = max(__double2hiint(K) - hmin, 0);
            unsigned q = sh_bits >= 32 ? (unsigned)dh >> (sh_bits - 32)
                                       : __builtin_amdgcn_alignbit((unsigned)dh, (unsigned)__double2loint(K), sh_bits);
            q = min(max(q, 1u), qmax);
            // the reference's fill order: cell (i, j) at j + yx i where j < yx, at i + ny j behind all of those otherwise
            const bool second = CROSSING && j >= yx;
            key = q << TB | (second ? (1u << 10 | (unsigned)j << 5 | (unsigned)i) : ((unsigned)i << 5 | (unsigned)j));
        }
        v.k[r] = key;
    }
}

// The phases `sorted_log2` + 1 ... `total_log2` of sort512's nine (phase k merges ascending blocks of 2^(k-1) positions into
// ascending blocks of 2^k): blocks of 2^sorted_log2 positions ascend already, everything behind the first 2^total_log2
// positions is high padding.  Both wave-uniform.
__device__ __forceinline__ void sort_phases(Keys& v, int lane, const LaneMasks& lm, int sorted_log2, int total_log2) {
#define RO_LANE_TAIL lane_step<4>(v); lane_step<2>(v); lane_step<1>(v);
    if (sorted_log2 < 1) lane_step<1>(v);
    if (sorted_log2 < 2) { lane_mirror<4>(v); lane_step<1>(v); }
    if (sorted_log2 < 3) { lane_mirror<8>(v); lane_step<2>(v); lane_step<1>(v); }
    if (sorted_log2 < 4 && total_log2 >= 4) { cross_step<1, true>(v, lane, lm); RO_LANE_TAIL }
    if (total_log2 >= 5) { cross_step<3, true>(v, lane, lm); cross_step<1, false>(v, lane, lm); RO_LANE_TAIL }
    if (total_log2 >= 6) {
        cross_step<7, true>(v, lane, lm); cross_step<2, false>(v, lane, lm); cross_step<1, false>(v, lane, lm);
        RO_LANE_TAIL
    }
    if (total_log2 >= 7) {
        cross_step<15, true>(v, lane, lm); cross_step<4, false>(v, lane, lm); cross_step<2, false>(v, lane, lm);
        cross_step<1, false>(v, lane, lm); RO_LANE_TAIL
    }
    if (total_log2 >= 8) {
        cross_step<31, true>(v, lane, lm); cross_step<8, false>(v, lane, lm); cross_step<4, false>(v, lane, lm);
        cross_step<2, false>(v, lane, lm); cross_step<1, false>(v, lane, lm); RO_LANE_TAIL
    }
    if (total_log2 >= 9) {
        cross_step<63, true>(v, lane, lm); cross_step<16, false>(v, lane, lm); cross_step<8, false>(v, lane, lm);
        cross_step<4, false>(v, lane, lm); cross_step<2, false>(v, lane, lm); cross_step<1, false>(v, lane, lm);
        RO_LANE_TAIL
    }
#undef RO_LANE_TAIL
}

// The key scale of one problem (wave-uniform), as ro::mix sets it: q = (bits(K) - (hmin << 32)) >> sh with 1 <= q < 2^QB for
// Kmin <= K <= Kmax, QB = 22 bits without a crossing, 21 with one; beyond sh = 32 the base is a multiple of 2^(sh - 32).
__device__ __forceinline__ void key_scale(double kmin, double kmax, bool no_crossing, int& hmin, int& sh_bits) {
    const int QB = 32 - (no_crossing ? 10 : 11);
    const int hk = __builtin_amdgcn_readfirstlane(__double2hiint(kmin));
    const unsigned long long span =
        ((unsigned long long)(unsigned)(__builtin_amdgcn_readfirstlane(__double2hiint(kmax)) - hk) << 32) |
        (unsigned)__builtin_amdgcn_readfirstlane(__double2loint(kmax));
    const int bl0 = span ? 64 - __clzll((long long)span) : 0;
    const int bias = 1 << max(0, bl0 - QB - 30);
    hmin = hk - bias;
    const unsigned long long dmax = span + ((unsigned long long)(unsigned)bias << 32);
    const int bl = 64 - __clzll((long long)dmax);
    sh_bits = bl > QB ? bl - QB : 0;
    if (sh_bits > 32) {
        const unsigned long long slack = ((1ull << (sh_bits - 32)) - 1ull) << 32;
        if (64 - __clzll((long long)(dmax + slack)) > bl) sh_bits++;
        hmin &= ~((1 << (sh_bits - 32)) - 1);
    }
}

// re-binning (:3379-3396 with 400 -> n): the rank w in [1, n) whose abscissa is the first above Gauss point `lane`'s (returned
// in yq), n where there is none; at most one Gauss point per rank.  All 64 lanes call; lanes >= ny return a rank beyond the sums.
__device__ __forceinline__ int locate_ny(const Shared& sh, int lane, int ny, int n, double& yq, unsigned& skipped) {
    int w = n + lane;  // beyond the Gauss points: ascending, so that no skip is seen there
    yq = 0.0;
    if (lane < ny) {
        yq = sh.gy[lane];
        int lo = 1, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sh.Y[padded(mid)] > yq) hi = mid; else lo = mid + 1;
        }
        w = lo;
    }
    // a Gauss point that falls into the interval of its predecessor takes the next one (the reference's walk advances w
    // before it looks at the next point, and reports a malfunction, :3383-3387): w'_q = max over j <= q of (w_j + q - j)
    int wq = w;
    const int wprev = __builtin_amdgcn_update_dpp(0, w, 0x138, 0xF, 0xF, false);   // wave_shr:1: the lane below's rank
    if (__ballot(lane >= 1 && lane < ny && w <= wprev) != 0) {
        int t = lane < ny ? w - lane : -(1 << 20);
#pragma unroll 1
        for (int d = 1; d < 32; d <<= 1) {
            const int up = __builtin_amdgcn_ds_bpermute(max(lane - d, 0) << 2, t);
            if (lane >= d) t = max(t, up);
        }
        wq = t + lane;
        skipped += __popcll(__ballot(lane < ny && wq != w));
    }
    return wq;
}

// Behind the network (rank w at position w): the exact order, the keys by rank to LDS, the abscissae (pitch 9 per lane, as
// ro::mix lays them out); returns this lane's Gauss point re-binned.  The exact finish is ro::finish_and_rebin's, copied (see
// the head of this file): a fix to one of the two belongs in the other.
template <bool CROSSING>
__device__ __forceinline__ double finish_and_rebin_ny(Shared& sh, int lane, int ny, int n, Keys& v, double my_mix, Counters& cnt) {
    const bool mine = lane < NLANES;   // ranks 0 ... 399: all sums, and padding behind them
    const char* ob = (const char*)sh.tab;
    const char* ib = (const char*)sh.tab + IP_OFF;
    unsigned ao[SLOTS], ai[SLOTS];
#pragma unroll
    for (int r = 0; r < SLOTS; r++) decode<CROSSING>(v.k[r], ao[r], ai[r]);
    {
        double K[SLOTS];
#pragma unroll
        for (int r = 0; r < SLOTS; r++) K[r] = *(const double*)(ob + ao[r]) + *(const double*)(ib + ai[r]);   // padding: inf
        // exact finish: any inversion left by the quantisation?  (odd-even transposition on the exact sums, strict '>': stable;
        // the keys go along, sums and weights follow from them)
        auto inverted = [&]() {
            bool inv = false;
#pragma unroll
            for (int r = 0; r + 1 < SLOTS; r++) inv = inv || K[r] > K[r + 1];
            const double kn = from_next_lane(K[0]);
            inv = inv || (lane < 63 && K[SLOTS - 1] > kn);
            return __ballot(inv) != 0;
        };
        if (inverted()) {   // wave-uniform
            int passes = 0;
            do {
                passes++;
                auto ce = [&](int a, int b) {
                    const bool sw = K[a] > K[b];
                    const double ka = K[a], kb = K[b];
                    const unsigned ea = v.k[a], eb = v.k[b];
                    K[a] = sw ? kb : ka; K[b] = sw ? ka : kb;
                    v.k[a] = sw ? eb : ea; v.k[b] = sw ? ea : eb;
                };
                ce(0, 1); ce(2, 3); ce(4, 5); ce(6, 7);
                ce(1, 2); ce(3, 4); ce(5, 6);
                // across the lanes: every lane looks at its neighbours' values of BEFORE the exchange
                const double kn0 = from_next_lane(K[0]), kp7 = from_prev_lane(K[SLOTS - 1]);
                const bool sw_hi = lane < 63 && K[SLOTS - 1] > kn0, sw_lo = lane > 0 && kp7 > K[0];
                const unsigned en0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.k[0], 0x130, 0xF, 0xF, false);
                const unsigned ep7 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.k[SLOTS - 1], 0x138, 0xF, 0xF, false);
                if (sw_hi) { K[SLOTS - 1] = kn0; v.k[SLOTS - 1] = en0; }
                if (sw_lo) { K[0] = kp7; v.k[0] = ep7; }
            } while (passes < 2 * POSITIONS && inverted());
            cnt.passes += passes;
#pragma unroll
            for (int r = 0; r < SLOTS; r++) decode<CROSSING>(v.k[r], ao[r], ai[r]);
        }
    }
    if (mine) {   // the keys by rank: what the interpolation below reads its two sums from
        uint4* e = (uint4*)(sh.E + SLOTS * lane);
        e[0] = make_uint4(v.k[0], v.k[1], v.k[2], v.k[3]);
        e[1] = make_uint4(v.k[4], v.k[5], v.k[6], v.k[7]);
    }
    // the weights in rank order, from the cells; cumulative mid-point abscissae Y_w = sum_{v<w} g_v + g_w/2 (:3371-3376)
    double g[SLOTS], csum = 0.0;
#pragma unroll
    for (int r = 0; r < SLOTS; r++) {
        g[r] = *(const double*)(ob + ao[r] + 8) * *(const double*)(ib + ai[r] + 8);   // padding: 0
        csum += g[r];
    }
    double run = wave_inclusive_sum(csum) - csum;
#pragma unroll
    for (int r = 0; r < SLOTS; r++) {
        if (mine) sh.Y[(SLOTS + 1) * lane + r] = fma(0.5, g[r], run);  // = run + 0.5 g bit for bit (0.5 g is exact)
        run += g[r];
    }
    sync();
    double yq;
    const int wq = locate_ny(sh, lane, ny, n, yq, cnt.skipped);
    double out = my_mix;  // the walk ran out of sums: the reference leaves the entry as it was
    if (lane < ny && wq < n) {
        const double K0 = cell_sum<CROSSING>(sh, sh.E[wq - 1]), K1 = cell_sum<CROSSING>(sh, sh.E[wq]);
        const double y0 = sh.Y[padded(wq - 1)], y1 = sh.Y[padded(wq)];
        out = (K0 * (y1 - yq) + K1 * (yq - y0)) / (y1 - y0);
    }
    return out;
}

// One problem.  Lanes 0 ... ny - 1 pass the running mix and the new absorber's (already scaled) k-coefficients at their Gauss
// point and receive the mixed value; what the other lanes pass is not read (the species loop hands over its loader groups'
// coefficients there) and what they receive means nothing.  2 <= ny <= NY, wave-uniform.  All 64 lanes must call.
__device__ __forceinline__ double mix_ny(Shared& sh, int ny, int lane, double my_mix, double my_add, Counters& cnt) {
    ny = __builtin_amdgcn_readfirstlane(ny);
    const int last = ny - 1, n = ny * ny;
    const double m0 = lane_value<0>(my_mix), a0 = lane_value<0>(my_add);
    const double ml = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_mix), last), __builtin_amdgcn_readlane(__double2loint(my_mix), last));
    const double al = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_add), last), __builtin_amdgcn_readlane(__double2loint(my_add), last));
    // less than 1 % of the other everywhere: correlated-k (:3297-3310)
    if ((0.01 * m0 > al) || (0.01 * a0 > ml)) return my_mix + my_add;
    const bool mix_first = m0 > a0;
    sync();  // the previous problem's readers are done with sh
    if (lane < ny) {
        sh.tab[lane].ov = mix_first ? my_mix : my_add;
        sh.tab[lane].iv = mix_first ? my_add : my_mix;
    }
    sync();
    // last crossing of the two curves (:3321-3329); are both ascending?  Do the rows of the tableau overlap?
    bool cross = false, down = false, over = false;
    if (lane >= 1 && lane < ny) {
        const double po = sh.tab[lane - 1].ov, pi = sh.tab[lane - 1].iv;
        const double pm = mix_first ? po : pi, pa = mix_first ? pi : po;
        cross = (my_mix > my_add) != (pm > pa);
        down = my_mix < pm || my_add < pa;
        const double mo = mix_first ? my_mix : my_add;  // outer[lane]
        over = po + (mix_first ? al : ml) > mo + (mix_first ? a0 : m0);
    }
    const unsigned long long cmask = __ballot(cross);
    const int yx = cmask ? 63 - __clzll((long long)cmask) : ny;
    const bool monotone = __ballot(down) == 0;
    const bool rows_apart = __ballot(over) == 0;
    double kmin = m0 + a0, kmax = ml + al;
    if (!monotone) {  // the extreme sums are not at the corners of the tableau
        double mn1 = sh.tab[0].ov, mx1 = mn1, mn2 = sh.tab[0].iv, mx2 = mn2;
#pragma unroll 1
        for (int j = 1; j < ny; j++) {
            mn1 = fmin(mn1, sh.tab[j].ov); mx1 = fmax(mx1, sh.tab[j].ov);
            mn2 = fmin(mn2, sh.tab[j].iv); mx2 = fmax(mx2, sh.tab[j].iv);
        }
        kmin = mn1 + mn2;
        kmax = mx1 + mx2;
    }
    int hmin, sh_bits;
    key_scale(kmin, kmax, yx == ny, hmin, sh_bits);
    Keys v;
    if (yx == ny) fill_cells<false>(sh, lane, v, ny, n, yx, hmin, sh_bits);
    else fill_cells<true>(sh, lane, v, ny, n, yx, hmin, sh_bits);
    if (!(monotone && yx == ny && rows_apart)) {   // else: the sums ascend in fill order, which is the cells' order
        LaneMasks lm;
#pragma unroll
        for (int t = 0; t < 3; t++) lm.c[t] = (unsigned)__builtin_amdgcn_sbfe(lane, t, 1);
        const int total_log2 = 32 - __clz(n - 1);                                 // 2^total_log2 >= n
        const int sorted_log2 = (monotone && (ny & last) == 0) ? 31 - __clz(ny) : 0;   // a row is a block of the network
        sort_phases(v, lane, lm, sorted_log2, total_log2);
    }
    if (yx == ny) return finish_and_rebin_ny<false>(sh, lane, ny, n, v, my_mix, cnt);
    return finish_and_rebin_ny<true>(sh, lane, ny, n, v, my_mix, cnt);
}

}  // namespace ro
