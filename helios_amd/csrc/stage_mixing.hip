// Per-stage entry points, part 4: on-the-fly opacity mixing (correlated-k and random overlap),
// H2O Rayleigh scattering, scattering-cross-section accumulation, total asymmetry parameter.
#include "two_stream.h"
#include "random_overlap_ny.h"
#include <cstdlib>
#include <string>

using namespace hx;

namespace {

constexpr int RO_NY = 20;
constexpr int RO_N = RO_NY * RO_NY;  // 400 pair sums
constexpr int RO_PER_LANE = 7;       // 64 * 7 = 448 >= 400

// add_to_mixed_opac (kernels.cu:3263-3399) by all-pairs ranking: the simple, independent cross-check of
// the product kernel below (HELIOS_RO_SORT=rank).  ONE wavefront (= one 64-thread workgroup) per (bin x, level i): the
// 20+20 k-coefficients, the 400 pair sums and their sorted copies live in LDS.
//
// The reference repeats adjacent-swap passes with a strict '<' (a stable sort of the fill-ordered array), i.e.
// position(e) = #{f : K_f < K_e} + #{f < e : K_f == K_e} with e, f the positions in the reference's fill order (the order
// inside a group of equal sums matters: it decides which weight sits at the group's edge).  Here every pair sum is ranked
// against all 400 (LDS broadcasts, one fp64 compare + add per pair): 5.6 k VALU instructions per problem, 160 000 compares.
// (Measured alternatives, both slower on gfx950: 64-bit integer keys -- v_cmp_lt_u64 issues at a fraction of the fp64
// compare rate; a first pass on the upper 32 key bits -- pair sums of a dominant and a minor absorber agree to < 1e-6 far
// too often.)
__global__ void __launch_bounds__(64)
k_add_to_mixed_opac_rank(const double* __restrict__ vmr, const double* __restrict__ opac_spec,
                         double* __restrict__ opac_wg, const double* __restrict__ meanmolmass,
                         const double* __restrict__ gauss_weight, const double* __restrict__ gauss_y,
                         double mass_spec, int s, int ro_method, int ny, int nbin, int nlev,
                         unsigned long long* __restrict__ rebin_skipped) {
    __shared__ double s_mix[RO_NY], s_add[RO_NY], s_hw[RO_NY], s_gy[RO_NY];
    __shared__ double s_G[RO_N], s_Ks[RO_N], s_Y[RO_N];
    __shared__ __align__(16) double s_K[RO_N];
    __shared__ int s_w[RO_NY];
    int* s_slot = (int*)s_Ks;  // rank slots alias the sorted-sum buffer (used before it is filled)
    const int lane = threadIdx.x;
    const long long npair = (long long)nbin * nlev;
    if (lane < ny && lane < RO_NY) {
        s_hw[lane] = 0.5 * gauss_weight[lane];
        s_gy[lane] = gauss_y[lane];
    }
    for (long long pair = blockIdx.x; pair < npair; pair += gridDim.x) {
        const int i = (int)(pair / nbin);
        const size_t base = (size_t)ny * pair;  // = ny*x + ny*nbin*i
        __syncthreads();
        const double scale_num = vmr[i] * mass_spec;
        const double mmm = meanmolmass[i];
        if (ny > RO_NY || ny == 1 || ro_method == 0 || s == 0) {
            // correlated-k for any ny (kernels.cu:3302-3310)
            for (int y = lane; y < ny; y += 64) opac_wg[base + y] += scale_num / mmm * opac_spec[base + y];
            continue;
        }
        if (lane < ny) {
            s_mix[lane] = opac_wg[base + lane];
            s_add[lane] = scale_num / mmm * opac_spec[base + lane];
        }
        __syncthreads();
        // negligibility test (:3297): wave-uniform
        const bool negligible = (0.01 * s_mix[0] > s_add[ny - 1]) || (0.01 * s_add[0] > s_mix[ny - 1]);
        if (negligible) {
            if (lane < ny) opac_wg[base + lane] = s_mix[lane] + s_add[lane];
            continue;
        }
        // last crossing of the two curves (:3321-3329)
        bool cross = false;
        if (lane >= 1 && lane < ny)
            cross = (s_mix[lane] > s_add[lane]) != (s_mix[lane - 1] > s_add[lane - 1]);
        const unsigned long long cmask = __ballot(cross);
        const int yx = cmask ? 63 - __clzll((long long)cmask) : ny;
        const bool mix_first = s_mix[0] > s_add[0];
        // fill in the reference's order (:3332-3365)
        // e / yx and e / 20 for e < 512 as multiply-shift (exact: e * d < 2^20 / d for d <= 20), full-rate 24-bit
        // multiplies instead of the generic 32-bit division sequence
        const int nfirst = RO_NY * yx;
        const int inv_yx = (1048576 + yx - 1) / yx;  // yx is wave-uniform: once per problem
        auto pair_of = [&](int e, int& y1, int& y2) {  // y1 indexes the running mix, y2 the new species
            const bool first = e < nfirst;
            const int q = (int)(__umul24(e, first ? inv_yx : 52429) >> 20);  // e / yx  or  e / 20
            const int rem = e - __umul24(q, first ? yx : RO_NY);
            const bool q_is_mix = mix_first == first;
            y1 = q_is_mix ? q : rem;
            y2 = q_is_mix ? rem : q;
        };
        double ke[RO_PER_LANE];
        for (int r = 0; r < RO_PER_LANE; r++) {
            const int e = lane + 64 * r;
            ke[r] = 0.0;
            if (e < RO_N) {
                int y1, y2;
                pair_of(e, y1, y2);
                ke[r] = s_mix[y1] + s_add[y2];
                s_G[e] = s_hw[y1] * s_hw[y2];
                s_K[e] = ke[r];
            }
        }
        __syncthreads();
        // ranks
        int rank[RO_PER_LANE];
#pragma unroll
        for (int r = 0; r < RO_PER_LANE; r++) rank[r] = 0;
        {
            const double2* keys2 = reinterpret_cast<const double2*>(s_K);
#pragma unroll 8
            for (int f2 = 0; f2 < RO_N / 2; f2++) {
                const double2 kf = keys2[f2];
#pragma unroll
                for (int r = 0; r < RO_PER_LANE; r++) rank[r] += (kf.x < ke[r] ? 1 : 0) + (kf.y < ke[r] ? 1 : 0);
            }
        }
        // equal sums collide on a rank slot (detected by writing the positions into the rank slots and reading
        // them back, a wave-uniform decision); only then a second pass adds the tie-break
        for (int r = 0; r < RO_PER_LANE; r++) {
            const int e = lane + 64 * r;
            if (e < RO_N) s_slot[rank[r]] = e;
        }
        __syncthreads();
        bool clash = false;
        for (int r = 0; r < RO_PER_LANE; r++) {
            const int e = lane + 64 * r;
            if (e < RO_N && s_slot[rank[r]] != e) clash = true;
        }
        const bool any_clash = __ballot(clash) != 0;
        __syncthreads();
        if (any_clash) {  // rare: exact ties -> stable order by fill position
            for (int f = 0; f < RO_N; f++) {
                const double kf = s_K[f];
#pragma unroll
                for (int r = 0; r < RO_PER_LANE; r++) rank[r] += (kf == ke[r] && f < lane + 64 * r) ? 1 : 0;
            }
        }
        // scatter into sorted order; s_Y temporarily holds the sorted weights
        for (int r = 0; r < RO_PER_LANE; r++) {
            const int e = lane + 64 * r;
            if (e < RO_N) {
                s_Ks[rank[r]] = ke[r];
                s_Y[rank[r]] = s_G[e];
            }
        }
        __syncthreads();
        // cumulative mid-point abscissae Y_w = sum_{v<w} g_v + g_w/2 (:3371-3376): lane-contiguous chunks of 8 + wave
        // exclusive scan, rank w at position ro::RANK0 + w -- the slots of a lane in the product kernel's network, so that
        // both kernels add in the same order and agree bit for bit
        double g[ro::SLOTS], csum = 0.0;
        for (int r = 0; r < ro::SLOTS; r++) {
            const int w = lane * ro::SLOTS + r - ro::RANK0;
            g[r] = (w >= 0 && w < RO_N) ? s_Y[w] : 0.0;
            csum += g[r];
        }
        double run = ro::wave_inclusive_sum(csum) - csum;
        __syncthreads();
        for (int r = 0; r < ro::SLOTS; r++) {
            const int w = lane * ro::SLOTS + r - ro::RANK0;
            if (w >= 0 && w < RO_N) s_Y[w] = run + 0.5 * g[r];
            run += g[r];
        }
        __syncthreads();
        // re-binning (:3379-3396): first w >= 1 with Y_w > y_q, at most one Gauss point per w
        if (lane < ny) {
            const double yq = s_gy[lane];
            int lo = 1, hi = RO_N;  // first index in [1, 400) with Y > yq, else 400
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_Y[mid] > yq) hi = mid; else lo = mid + 1;
            }
            s_w[lane] = lo;
        }
        __syncthreads();
        if (lane == 0) {
            // a Gauss point that falls into the interval of its predecessor takes the next one; the reference reports
            // this as a malfunction of the re-binning (:3383-3387), here it is counted (hx_diag_read)
            int skipped = 0;
            for (int q = 1; q < ny; q++)
                if (s_w[q] <= s_w[q - 1]) {
                    s_w[q] = s_w[q - 1] + 1;
                    skipped++;
                }
            if (skipped) atomicAdd(rebin_skipped, (unsigned long long)skipped);
        }
        __syncthreads();
        if (lane < ny) {
            const int w = s_w[lane];
            if (w < RO_N) {
                const double yq = s_gy[lane];
                opac_wg[base + lane] =
                    (s_Ks[w - 1] * (s_Y[w] - yq) + s_Ks[w] * (yq - s_Y[w - 1])) / (s_Y[w] - s_Y[w - 1]);
            }
        }
    }
}

// ---- random overlap, the product kernel: 32-bit keys that carry their cell, bitonic network, exact finish (random_overlap.h)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5)))
k_add_to_mixed_opac_lean(const double* __restrict__ vmr, const double* __restrict__ opac_spec,
                         double* __restrict__ opac_wg, const double* __restrict__ meanmolmass,
                         const double* __restrict__ gauss_weight, const double* __restrict__ gauss_y,
                         double mass_spec, int nbin, int nlev, unsigned long long* __restrict__ diag) {
    __shared__ ro::Shared sh;
    const int lane = threadIdx.x;
    const ro::LaneConst lc = ro::init(sh, lane, gauss_weight, gauss_y);
    const long long npair = (long long)nbin * nlev;
    const long long chunk = (npair + gridDim.x - 1) / gridDim.x;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = min(npair, p0 + chunk);
    int i_cur = -1;
    double fac = 0.0;
    ro::Counters cnt;
    for (long long pair = p0; pair < p1; pair++) {
        const int i = (int)(pair / nbin);
        if (i != i_cur) {
            i_cur = i;
            fac = vmr[i] * mass_spec / meanmolmass[i];  // (vmr * mass) / mu, then times kappa (:3293)
        }
        const size_t base = (size_t)RO_NY * pair;  // = ny*x + ny*nbin*i
        double my_mix = 0.0, my_add = 0.0;
        if (lane < RO_NY) {
            my_mix = opac_wg[base + lane];
            my_add = fac * opac_spec[base + lane];
        }
        const double out = ro::mix(sh, lc, lane, my_mix, my_add, cnt);
        if (lane < RO_NY) opac_wg[base + lane] = out;
    }
    ro::flush(cnt, lane, diag);
}

// ---- random overlap for 2 <= ny <= 19 Gauss points: the same loop around the general mixer (random_overlap_ny.h)
__global__ void __launch_bounds__(64) k_add_to_mixed_opac_ny(const double* __restrict__ vmr, const double* __restrict__ opac_spec,
                       double* __restrict__ opac_wg, const double* __restrict__ meanmolmass,
                       const double* __restrict__ gauss_weight, const double* __restrict__ gauss_y,
                       double mass_spec, int ny, int nbin, int nlev, unsigned long long* __restrict__ diag) {
    __shared__ ro::Shared sh;
    const int lane = threadIdx.x;
    ro::init_ny(sh, lane, ny, gauss_weight, gauss_y);
    const long long npair = (long long)nbin * nlev;
    const long long chunk = (npair + gridDim.x - 1) / gridDim.x;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = min(npair, p0 + chunk);
    int i_cur = -1;
    double fac = 0.0;
    ro::Counters cnt;
    for (long long pair = p0; pair < p1; pair++) {
        const int i = (int)(pair / nbin);
        if (i != i_cur) {
            i_cur = i;
            fac = vmr[i] * mass_spec / meanmolmass[i];  // (vmr * mass) / mu, then times kappa (:3293)
        }
        const size_t base = (size_t)ny * pair;  // = ny*x + ny*nbin*i
        double my_mix = 0.0, my_add = 0.0;
        if (lane < ny) {
            my_mix = opac_wg[base + lane];
            my_add = fac * opac_spec[base + lane];
        }
        const double out = ro::mix_ny(sh, ny, lane, my_mix, my_add, cnt);
        if (lane < ny) opac_wg[base + lane] = out;
    }
    ro::flush(cnt, lane, diag);
}

__global__ void __launch_bounds__(256)
k_add_correlated_k(const double* __restrict__ vmr, const double* __restrict__ opac_spec, double* __restrict__ opac_wg,
                   const double* __restrict__ meanmolmass, double mass_spec, int ny, int nbin, int nlev) {
    // kernels.cu:3302-3310 for any ny: opac += (vmr * mass / mu) * kappa
    const size_t per_level = (size_t)ny * nbin;
    const int i = blockIdx.y;
    const double fac = vmr[i] * mass_spec / meanmolmass[i];
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < per_level; k += (size_t)gridDim.x * blockDim.x)
        opac_wg[per_level * i + k] += fac * opac_spec[per_level * i + k];
}

// calc_index_h2o / calc_h2o_scat (kernels.cu:3174-3205, :3404-3440)
__global__ void __launch_bounds__(256)
k_calc_h2o_scat(const double* __restrict__ temp, const double* __restrict__ press,
                const double* __restrict__ wave, double* __restrict__ scat_cross,
                const double* __restrict__ vmr, double mass_h2o, int nbin, int nlev) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (x >= nbin) return;
    const double sc = h2o_rayleigh_cross(temp[i], press[i], vmr[i], wave[x], mass_h2o);
    scat_cross[x + (size_t)nbin * i] = sc;
}

__global__ void __launch_bounds__(256)
k_add_to_mixed_scat(const double* __restrict__ vmr, const double* __restrict__ spec,
                    double* __restrict__ total, int nbin, int nlev) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (x >= nbin) return;
    const size_t b = x + (size_t)nbin * i;
    total[b] += vmr[i] * spec[b];
}

__global__ void __launch_bounds__(256)
k_calc_total_g0(const double* __restrict__ scat_cross, const double* __restrict__ g_cl,
                const double* __restrict__ scat_cl, double* __restrict__ g_tot, double g_0, size_t n) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double num = g_0 * scat_cross[k] + g_cl[k] * scat_cl[k];
    const double den = scat_cross[k] + scat_cl[k];
    g_tot[k] = num / den;
}

}  // namespace

extern "C" {

int hx_add_to_mixed_opac(hx_context* ctx, const double* vmr, const double* opac_spec,
                         double* opac_wg, const double* meanmolmass, const double* gauss_weight,
                         const double* gauss_y, double mass_spec, int s, int ro_method, int ny,
                         int nbin, int nlay_or_nint) {
    // HELIOS_RO_SORT, read once: unset or lean (the product kernel), rank (the all-pairs cross-check).  Anything else is
    // refused, so that a recipe written for the older sort kernels does not silently time the product kernel.
    static const std::string sort = [] {
        const char* e = getenv("HELIOS_RO_SORT");
        return std::string(e ? e : "");
    }();
    const bool rank = sort == "rank";
    if (!rank && !sort.empty() && sort != "lean")
        return hx_fail(ctx, HX_E_ARG, "HELIOS_RO_SORT=%s is not a random-overlap kernel of this library (lean or rank)",
                       sort.c_str());
    const bool ro_possible = ro_method != 0 && s != 0 && ny != 1;
    if (ro_possible && ny != RO_NY)
        return hx_fail(ctx, HX_E_RO_NY, "random-overlap mixing needs ny == 20 (got %d)", ny);
    const long long npair = (long long)nbin * nlay_or_nint;
    const int grid = (int)min(npair, (long long)256 * 12 * 16);
    if (rank)
        k_add_to_mixed_opac_rank<<<grid, 64, 0, ctx->stream>>>(vmr, opac_spec, opac_wg, meanmolmass, gauss_weight,
                                                              gauss_y, mass_spec, s, ro_method, ny, nbin, nlay_or_nint,
                                                              ctx->diag + HX_DIAG_RO_REBIN);
    else if (!ro_possible)
        k_add_correlated_k<<<dim3(hx_cdiv((long long)ny * nbin, 1024), nlay_or_nint), 256, 0, ctx->stream>>>(
            vmr, opac_spec, opac_wg, meanmolmass, mass_spec, ny, nbin, nlay_or_nint);
    else
        k_add_to_mixed_opac_lean<<<grid, 64, 0, ctx->stream>>>(vmr, opac_spec, opac_wg, meanmolmass, gauss_weight,
                                                              gauss_y, mass_spec, nbin, nlay_or_nint, ctx->diag);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

int hx_add_to_mixed_opac_ny(hx_context* ctx, const double* vmr, const double* opac_spec, double* opac_wg,
                            const double* meanmolmass, const double* gauss_weight, const double* gauss_y, double mass_spec,
                            int s, int ro_method, int ny, int nbin, int nlay_or_nint) {
    const bool ro_possible = ro_method != 0 && s != 0 && ny != 1;
    if (!ro_possible || ny >= RO_NY)   // the kernel of 20 points, correlated-k for any ny, the refusal beyond 20
        return hx_add_to_mixed_opac(ctx, vmr, opac_spec, opac_wg, meanmolmass, gauss_weight, gauss_y, mass_spec, s, ro_method,
                                    ny, nbin, nlay_or_nint);
    // HELIOS_RO_SORT chooses between the two kernels of 20 points; below 20 there is one kernel, and a value that asks for
    // another one (the all-pairs ranking included) is refused instead of being ignored
    const char* sort = getenv("HELIOS_RO_SORT");
    if (sort && *sort && std::string(sort) != "lean")
        return hx_fail(ctx, HX_E_ARG, "HELIOS_RO_SORT=%s: random overlap at %d Gauss points has the one kernel (lean)", sort, ny);
    const long long npair = (long long)nbin * nlay_or_nint;
    const int grid = (int)min(npair, (long long)256 * 12 * 16);
    if (grid > 0)
        k_add_to_mixed_opac_ny<<<grid, 64, 0, ctx->stream>>>(vmr, opac_spec, opac_wg, meanmolmass, gauss_weight, gauss_y,
                                                            mass_spec, ny, nbin, nlay_or_nint, ctx->diag);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

int hx_calc_h2o_scat(hx_context* ctx, const double* temp, const double* press, const double* wave,
                     double* scat_cross, const double* vmr, double mass_h2o, int nbin,
                     int nlay_or_nint) {
    k_calc_h2o_scat<<<dim3(hx_cdiv(nbin, 256), nlay_or_nint), 256, 0, ctx->stream>>>(
        temp, press, wave, scat_cross, vmr, mass_h2o, nbin, nlay_or_nint);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

int hx_add_to_mixed_scat(hx_context* ctx, const double* vmr, const double* scat_cross_spec,
                         double* scat_cross, int nbin, int nlay_or_nint) {
    k_add_to_mixed_scat<<<dim3(hx_cdiv(nbin, 256), nlay_or_nint), 256, 0, ctx->stream>>>(
        vmr, scat_cross_spec, scat_cross, nbin, nlay_or_nint);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

int hx_calc_total_g_0_of_gas_and_clouds(hx_context* ctx, const double* scat_cross,
                                        const double* g_0_all_clouds,
                                        const double* scat_cross_all_clouds, double* g_0_tot,
                                        double g_0, int nbin, int nlay_or_nint) {
    const size_t n = (size_t)nbin * nlay_or_nint;
    k_calc_total_g0<<<hx_cdiv((long long)n, 256), 256, 0, ctx->stream>>>(
        scat_cross, g_0_all_clouds, scat_cross_all_clouds, g_0_tot, g_0, n);
    HX_LAUNCH_CHECK(ctx);
    return 0;
}

}  // extern "C"
