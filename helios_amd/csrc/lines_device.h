// The device functions that the line-by-line sums share (csrc/lines.hip, csrc/exomol.hip): the constants of the contract, K(x, y)
// in its four regions and the sum of a tile of points over a range of prepared lines.  The contract is helios_amd/lines.py's; a
// file that includes this header applies its statements, so its rows have the bits of every other file's.
//
// All arithmetic is fp64 without contraction and complex division is written out.
#pragma once
#include "hx_tool.h"
#include "lines_weideman.h"

#include <cmath>

namespace {

constexpr int LINES_THREADS = 256;           // lines.py: THREADS, POINTS_PER_THREAD, LDS_BLOCK, FAR_Z
constexpr int LINES_PPT = 4;
constexpr int LINES_TILE = LINES_THREADS * LINES_PPT;
constexpr int LINES_BLOCK = 256;
constexpr int LINES_WAVES = LINES_THREADS / 64;
constexpr double LINES_FAR = 101.0;
static_assert(LINES_BLOCK <= LINES_THREADS, "a thread stages at most one line of a block");

// phys_const.py
constexpr double LC_C = 2.99792458e10, LC_KB = 1.380649e-16, LC_H = 6.62607015e-27, LC_NA = 6.02214076e23;
constexpr double LC_TREF = 296.0, LC_ATM = 1013250.0, LC_YMIN = 1e-8;
constexpr double LC_LN2 = 0.6931471805599453, LC_INV_SQRT_PI = 0.5641895835477563;
constexpr double LC_R2_WEIDEMAN = 42.25, LC_R2_EIGHT = 225.0, LC_R2_FOUR = 1.0e4;

__device__ __forceinline__ double lines_k_weideman(double x, double y) {
    constexpr double A[LINES_WEIDEMAN_N] = {LINES_WEIDEMAN_A};
    const double lr = LINES_WEIDEMAN_L + y, li = -x;             // l = L - i z
    const double nr = LINES_WEIDEMAN_L - y, ni = x;              // L + i z
    const double d = lr * lr + li * li;
    const double zr = (nr * lr + ni * li) / d, zi = (ni * lr - nr * li) / d;
    double pr = A[0], pi = 0.0;
#pragma unroll
    for (int n = 1; n < LINES_WEIDEMAN_N; n++) {
        const double tr = pr * zr - pi * zi + A[n];
        pi = pr * zi + pi * zr;
        pr = tr;
    }
    const double l2r = lr * lr - li * li, l2i = 2.0 * lr * li;
    const double d2 = l2r * l2r + l2i * l2i;
    return (2.0 * pr * l2r + 2.0 * pi * l2i) / d2 + LC_INV_SQRT_PI * lr / d;
}

// Re of (i / sqrt pi) / t with t = z, then t = z - (k/2) / t for k = LEVELS ... 1
template <int LEVELS>
__device__ __forceinline__ double lines_k_fraction(double x, double y) {
    double tr = x, ti = y;
#pragma unroll
    for (int k = LEVELS; k >= 1; k--) {
        const double c = 0.5 * (double)k;
        const double d = tr * tr + ti * ti;
        const double nr = x - c * tr / d;
        ti = y + c * ti / d;
        tr = nr;
    }
    return LC_INV_SQRT_PI * ti / (tr * tr + ti * ti);
}

__device__ __forceinline__ double lines_k(double x, double y) {
    const double r2 = x * x + y * y;
    if (r2 > LC_R2_FOUR) return lines_k_fraction<2>(x, y);
    if (r2 > LC_R2_EIGHT) return lines_k_fraction<4>(x, y);
    if (r2 > LC_R2_WEIDEMAN) return lines_k_fraction<8>(x, y);
    return lines_k_weideman(x, y);
}

// the tile blockIdx.x of one node: the lines tile_range->x ... tile_range->y - 1 of `params` onto the tile's points
template <bool WITH_FP64>
__device__ __forceinline__ void lines_sum_tile(const int2* __restrict__ tile_range, const double* __restrict__ params,
                                               size_t stride, int n_points, double nu_first, double dnu, double cutoff, double molar_mass,
                                               double* __restrict__ kappa64, float* __restrict__ kappa32) {
    __shared__ double s_nu[LINES_BLOCK], s_s[LINES_BLOCK], s_a[LINES_BLOCK], s_y[LINES_BLOCK];
    __shared__ int s_far[LINES_WAVES];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x * LINES_TILE;
    const int2 range = *tile_range;
    double nu[LINES_PPT], acc[LINES_PPT];
#pragma unroll
    for (int j = 0; j < LINES_PPT; j++) {
        nu[j] = nu_first + (double)(tile + j * LINES_THREADS + tid) * dnu;
        acc[j] = 0.0;
    }
    const double tile_lo = nu_first + (double)tile * dnu;
    const double tile_hi = nu_first + (double)(min(tile + LINES_TILE, n_points) - 1) * dnu;

    for (int b = range.x; b < range.y; b += LINES_BLOCK) {
        const int n = min(LINES_BLOCK, range.y - b);
        __syncthreads();                                         // the block before has been walked by every thread
        int far = 1;
        if (tid < n) {
            const double v = params[b + tid], a = params[2 * stride + b + tid], y = params[3 * stride + b + tid];
            s_nu[tid] = v;
            s_s[tid] = params[stride + b + tid];
            s_a[tid] = a;
            s_y[tid] = y;
            const double dist = fmax(fmax(v - tile_hi, tile_lo - v), 0.0);
            far = (a * dist > LINES_FAR) || (y > LINES_FAR);
        }
        const int wave_far = __all(far);
        if ((tid & 63) == 0) s_far[tid >> 6] = wave_far;
        __syncthreads();
        int all_far = 1;
#pragma unroll
        for (int w = 0; w < LINES_WAVES; w++) all_far &= s_far[w];
        if (__builtin_amdgcn_readfirstlane(all_far)) {
            for (int l = 0; l < n; l++) {
                const double v = s_nu[l], s = s_s[l], a = s_a[l], y = s_y[l];
#pragma unroll
                for (int j = 0; j < LINES_PPT; j++) {
                    const double d = nu[j] - v;
                    const double term = s * lines_k_fraction<2>(a * d, y);
                    acc[j] = acc[j] + (fabs(d) <= cutoff ? term : 0.0);
                }
            }
        } else {
            for (int l = 0; l < n; l++) {
                const double v = s_nu[l], s = s_s[l], a = s_a[l], y = s_y[l];
#pragma unroll
                for (int j = 0; j < LINES_PPT; j++) {
                    const double d = nu[j] - v;
                    if (fabs(d) <= cutoff) acc[j] = acc[j] + s * lines_k(a * d, y);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LINES_PPT; j++) {
        const int p = tile + j * LINES_THREADS + tid;
        if (p < n_points) {
            const double k = acc[j] * LC_NA / molar_mass;
            if (WITH_FP64) kappa64[p] = k;
            kappa32[p] = (float)k;
        }
    }
}

}  // namespace
