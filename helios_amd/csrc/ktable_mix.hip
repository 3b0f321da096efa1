// The mixing stage of the k-table tool (include/helios_hip.h section 9; the contract and the host side are
// helios_amd/ktable_mix.py): the species' tables on the final (T, P) grid stay on the device, and every chemistry is one pass
//
//   kpoints[node][e] = sum over the absorbers s, in file order, of m_s[node] * k_s[node][e]      (e = y + ny * x)
//   scat[node][x]    = sum over the scattering species s, in file order, of x_s[node] * sigma_s(node, x)
//
// with one rounded product and one rounded add per term (the library is built with -ffp-contract=off).
//
//   k_ktmix_sum     grid (spans of 512 entries, nodes); a thread owns two neighbouring entries of one node's row, paired so that
//                   its 16-byte loads and stores are aligned whatever the parity of the row's start (rows are nc doubles apart,
//                   so with odd nc every other row starts 8 bytes off); the entry in front of or behind the pairs goes as 8 bytes.
//                   The node is uniform per workgroup: the species' mass mixing ratios arrive by scalar loads.  Up to KM_G
//                   species per launch, their tables as pointers in the argument struct; more are further launches that start
//                   from the accumulator.  Traffic: (absorbers + 1) tables per chemistry, no atomics.
//   k_ktable_regrid a native table onto the final grid into its slot: the k-table stage's own kernel (hx_internal_regrid, ktable.hip)
//   k_ktmix_scat    a thread owns one bin of one node; the water vapour's cross-section is stage 2's own formula (not the run-time
//                   h2o_rayleigh_cross of two_stream.h): no min(1, density), lambda <= 2.5 micron, the Lorentz-Lorenz factor is A
#include <algorithm>
#include <new>
#include <vector>

#include "hx_tool.h"

namespace {

constexpr int KM_G = 16;            // species per launch of k_ktmix_sum
constexpr int KM_THREADS = 256;
constexpr double KM_H2O_WEIGHT = 18.0153;      // g / mol, helios_amd/species_data.py
constexpr double KM_KB = 1.380649e-16;         // erg / K: helios_amd/phys_const.py, the k-table tool's (HX_KBOLTZMANN is the run-time kernels')
constexpr int KM_SPAN = 2 * KM_THREADS;
constexpr size_t KM_STAGE = (size_t)64 << 20;      // bytes per host-to-device copy of a table
constexpr unsigned long long KM_GUARD = 0x7ff8dead0badbeefULL;      // a NaN with a payload: the rows behind the tables

struct KmSum {
    const double* k[KM_G];
    const double* m[KM_G];          // m[g][node]
    double* acc;
    int n, nc, first_node, from_acc;
};

__global__ void __launch_bounds__(KM_THREADS) k_ktmix_sum(KmSum A) {
    const size_t node = (size_t)A.first_node + blockIdx.y;
    const size_t row = node * (size_t)A.nc;
    const int par = (int)(row & 1);                    // the tables' bases are 16-byte aligned (checked on the host)
    const int e0 = 2 * (int)(blockIdx.x * KM_THREADS + threadIdx.x) - par;
    if (e0 >= A.nc) return;
    const bool v0 = e0 >= 0, v1 = e0 + 1 < A.nc;
    double* __restrict__ out = A.acc + row;
    if (v0 && v1) {
        double2 a = A.from_acc ? *reinterpret_cast<const double2*>(out + e0) : make_double2(0.0, 0.0);
        int g = 0;
        for (; g + 4 <= A.n; g += 4) {                  // four species' loads in flight; the adds stay in species order
            double m[4];
            double2 k[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                m[u] = A.m[g + u][node];
                k[u] = *reinterpret_cast<const double2*>(A.k[g + u] + row + e0);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                a.x = a.x + m[u] * k[u].x;
                a.y = a.y + m[u] * k[u].y;
            }
        }
        for (; g < A.n; g++) {
            const double m = A.m[g][node];
            const double2 k = *reinterpret_cast<const double2*>(A.k[g] + row + e0);
            a.x = a.x + m * k.x;
            a.y = a.y + m * k.y;
        }
        *reinterpret_cast<double2*>(out + e0) = a;
    } else {
        const int e = v0 ? e0 : e0 + 1;
        double a = A.from_acc ? out[e] : 0.0;
        for (int g = 0; g < A.n; g++) a = a + A.m[g][node] * A.k[g][row + e];
        out[e] = a;
    }
}

struct KmScat {
    const double *sigma;            // [ns][nbin]
    const int* kind;                // 0: does not scatter or has no cross-section, 1: sigma[s], 2: water vapour
    const double *vmr;              // [ns][nodes]
    const double *wave, *temp, *press;
    double* out;
    int ns, nbin, np, first_node;
    size_t nodes;
    double m_h2o;                   // g
};

__global__ void __launch_bounds__(KM_THREADS) k_ktmix_scat(KmScat A) {
    const size_t node = (size_t)A.first_node + blockIdx.y;
    const int x = (int)(blockIdx.x * KM_THREADS + threadIdx.x);
    if (x >= A.nbin) return;
    const double T = A.temp[node / A.np], P = A.press[node % A.np];
    const double lam = A.wave[x];
    double acc = 0.0;
    for (int s = 0; s < A.ns; s++) {
        const int kind = A.kind[s];
        if (kind == 0) continue;
        const double f = A.vmr[(size_t)s * A.nodes + node];
        double sig;
        if (kind == 1) {
            sig = A.sigma[(size_t)s * A.nbin + x];
        } else {
            sig = 0.0;
            if (lam <= 2.5e-4 && f != 0.0) {
                // per node: the vapour's density, its number density and theta; they do not depend on the bin
                const double kt = KM_KB * T;
                const double delta = f * P * A.m_h2o / kt;
                const double n_ref = f * P / kt;
                const double theta = T / 273.15;
                const double a0 = 0.244257733, a1 = 0.974634476e-2, a2 = -0.373234996e-2, a3 = 0.268678472e-3,
                             a4 = 0.158920570e-2, a5 = 0.245934259e-2, a6 = 0.900704920, a7 = -0.166626219e-1;
                const double uv = 0.229202, ir = 5.432937;
                const double L = lam / 0.589e-4;
                const double l2 = L * L;
                const double Aq = delta * (a0 + a1 * delta + a2 * theta + a3 * l2 * theta + a4 / l2 + a5 / (l2 - uv * uv) +
                                           a6 / (l2 - ir * ir) + a7 * (delta * delta));
                const double lam2 = lam * lam;
                const double king = (6.0 + 3.0 * 3e-4) / (6.0 - 7.0 * 3e-4);
                sig = 24.0 * (HX_PI * HX_PI * HX_PI) / ((n_ref * n_ref) * (lam2 * lam2)) * (Aq * Aq) * king;
            }
        }
        acc = acc + f * sig;
    }
    A.out[node * (size_t)A.nbin + x] = acc;
}

}  // namespace

struct hx_ktmix {
    hx_context* ctx;
    int nbin, ny, nt, np, ns;
    size_t nc, nodes;
    double *wave, *temp, *press, *kpoints, *scat, *sigma, *mmr, *vmr;
    int* kind;
    std::vector<double*> slot;
    std::vector<int> hkind;
    hx_owned owned;
    bool have_grid, ran;
    double timing[4];               // ms in k_ktmix_sum and in k_ktmix_scat of the last run, ms in k_ktable_regrid so far, runs
};

// refuses what the device's free memory cannot hold, before asking for it
template <class T>
static int km_alloc(hx_ktmix* km, size_t bytes, T** p, const char* what) {
    size_t free_b = 0, total_b = 0;
    int rc = hx_mem_info(km->ctx, &free_b, &total_b);
    if (rc) return rc;
    if (bytes > free_b)
        return hx_fail(km->ctx, HX_E_ARG, "hx_ktmix: %s needs %zu bytes, the device has %zu free", what, bytes, free_b);
    rc = hx_owned_alloc(km->ctx, km->owned, bytes, p);
    if (rc) return hx_fail(km->ctx, rc, "hx_ktmix: the allocation of %zu bytes for %s failed", bytes, what);
    if (((uintptr_t)*p & 15) != 0) return hx_fail(km->ctx, HX_E_STATE, "hx_ktmix: %s is not 16-byte aligned", what);
    return 0;
}

static int km_upload(hx_ktmix* km, double* dst, const double* src, size_t n) {
    for (size_t done = 0; done < n;) {
        const size_t part = std::min(n - done, KM_STAGE / 8);
        int rc = hx_h2d(km->ctx, dst + done, src + done, part * 8);
        if (rc) return rc;
        done += part;
    }
    return 0;
}

static int km_slot_index(hx_ktmix* km, int s, const char* fn) {
    if (s < 0 || s >= km->ns)
        return hx_fail(km->ctx, HX_E_ARG, "%s: species slot %d out of range, the object has %d", fn, s, km->ns);
    return 0;
}

extern "C" {

int hx_ktmix_destroy(hx_ktmix* km) {
    if (!km) return HX_E_ARG;
    (void)hx_sync(km->ctx);
    hx_owned_free_all(km->ctx, km->owned);
    delete km;
    return 0;
}

int hx_ktmix_create(hx_context* ctx, int nbin, int ny, int nt, int np, int nspecies, hx_ktmix** out_km) {
    if (!ctx || !out_km) return HX_E_ARG;
    HX_REQUIRE(ctx, nbin >= 1 && ny >= 1 && nt >= 1 && np >= 1 && nspecies >= 1, HX_E_ARG,
               "bins, Gauss points, temperatures, pressures and species are >= 1");
    HX_REQUIRE(ctx, (long long)nbin * ny <= (1LL << 30), HX_E_ARG, "at most 2^30 entries per (T, P) node");
    HX_REQUIRE(ctx, (long long)nt * np <= (1LL << 30), HX_E_ARG, "at most 2^30 (T, P) nodes");
    hx_ktmix* km = new (std::nothrow) hx_ktmix();
    if (!km) return hx_fail(ctx, HX_E_ARG, "no host memory");
    km->ctx = ctx;
    km->nbin = nbin; km->ny = ny; km->nt = nt; km->np = np; km->ns = nspecies;
    km->nc = (size_t)nbin * ny; km->nodes = (size_t)nt * np;
    km->slot.assign(nspecies, nullptr);
    km->hkind.assign(nspecies, 0);
    // one row more than the tables hold: the guard rows behind them, which no kernel may touch
    int rc = km_alloc(km, (km->nodes + 1) * km->nc * 8, &km->kpoints, "kpoints");
    if (!rc) rc = km_alloc(km, (km->nodes + 1) * nbin * 8, &km->scat, "the Rayleigh table");
    if (!rc) rc = km_alloc(km, (size_t)nspecies * km->nodes * 8, &km->mmr, "the mass mixing ratios");
    if (!rc) rc = km_alloc(km, (size_t)nspecies * km->nodes * 8, &km->vmr, "the mixing ratios");
    if (!rc) rc = km_alloc(km, (size_t)nspecies * nbin * 8, &km->sigma, "the cross-sections");
    if (!rc) rc = km_alloc(km, (size_t)nspecies * 4, &km->kind, "the species' kinds");
    if (!rc) rc = km_alloc(km, (size_t)nbin * 8, &km->wave, "the wavelengths");
    if (!rc) rc = km_alloc(km, (size_t)nt * 8, &km->temp, "the temperatures");
    if (!rc) rc = km_alloc(km, (size_t)np * 8, &km->press, "the pressures");
    if (!rc) rc = hx_memset0(ctx, km->sigma, (size_t)nspecies * nbin * 8);
    if (!rc) rc = hx_memset0(ctx, km->kind, (size_t)nspecies * 4);
    if (!rc) {
        std::vector<unsigned long long> g(std::max(km->nc, (size_t)nbin), KM_GUARD);
        rc = hx_h2d(ctx, km->kpoints + km->nodes * km->nc, g.data(), km->nc * 8);
        if (!rc) rc = hx_h2d(ctx, km->scat + km->nodes * nbin, g.data(), (size_t)nbin * 8);
    }
    if (rc) {
        hx_ktmix_destroy(km);
        return rc;
    }
    *out_km = km;
    return 0;
}

int hx_ktmix_set_grid(hx_ktmix* km, const double* wave, const double* temp, const double* press) {
    if (!km) return HX_E_ARG;
    hx_context* ctx = km->ctx;
    HX_REQUIRE(ctx, wave && temp && press, HX_E_ARG, "null array");
    for (int i = 0; i < km->nt; i++) HX_REQUIRE(ctx, temp[i] > 0.0, HX_E_ARG, "temperatures are > 0");
    for (int j = 0; j < km->np; j++) HX_REQUIRE(ctx, press[j] > 0.0, HX_E_ARG, "pressures are > 0");
    for (int x = 0; x < km->nbin; x++) HX_REQUIRE(ctx, wave[x] > 0.0, HX_E_ARG, "wavelengths are > 0");
    int rc = hx_h2d(ctx, km->wave, wave, (size_t)km->nbin * 8);
    if (!rc) rc = hx_h2d(ctx, km->temp, temp, (size_t)km->nt * 8);
    if (!rc) rc = hx_h2d(ctx, km->press, press, (size_t)km->np * 8);
    if (rc) return rc;
    km->have_grid = true;
    return 0;
}

int hx_ktmix_set_species(hx_ktmix* km, int s, const double* k_on_final_grid) {
    if (!km) return HX_E_ARG;
    int rc = km_slot_index(km, s, "hx_ktmix_set_species");
    if (rc) return rc;
    if (!k_on_final_grid) {                 // not absorbing
        rc = hx_owned_free(km->ctx, km->owned, km->slot[s]);
        km->slot[s] = nullptr;
        return rc;
    }
    if (!km->slot[s]) {
        rc = km_alloc(km, km->nodes * km->nc * 8, &km->slot[s], "a species table");
        if (rc) { km->slot[s] = nullptr; return rc; }
    }
    return km_upload(km, km->slot[s], k_on_final_grid, km->nodes * km->nc);
}

int hx_ktmix_set_species_native(hx_ktmix* km, int s, const double* k_native, int nt_old, int np_old, const int* t_left,
                                const int* t_reduced, const int* p_left, const int* p_reduced, const double* temp_old,
                                const double* logp_old, const double* temp_new, const double* logp_new) {
    if (!km) return HX_E_ARG;
    hx_context* ctx = km->ctx;
    int rc = km_slot_index(km, s, "hx_ktmix_set_species_native");
    if (rc) return rc;
    HX_REQUIRE(ctx, nt_old >= 1 && np_old >= 1 && (long long)nt_old * np_old <= (1LL << 30), HX_E_ARG, "an empty native grid");
    HX_REQUIRE(ctx, k_native, HX_E_ARG, "null array");
    const hx_regrid_plan plan = {nt_old, np_old, km->nt, km->np, t_left, t_reduced, p_left, p_reduced,
                                 temp_old, logp_old, temp_new, logp_new};
    rc = hx_internal_regrid_check(ctx, __func__, &plan);
    if (rc) return rc;
    if (!km->slot[s]) {
        rc = km_alloc(km, km->nodes * km->nc * 8, &km->slot[s], "a species table");
        if (rc) { km->slot[s] = nullptr; return rc; }
    }
    const size_t n_old = (size_t)nt_old * np_old * km->nc;
    double* d_old = nullptr;
    rc = km_alloc(km, n_old * 8, &d_old, "a native species table");
    if (!rc) rc = km_upload(km, d_old, k_native, n_old);
    if (!rc) rc = hx_internal_regrid(ctx, __func__, &plan, d_old, km->slot[s], km->nc, &km->timing[2]);
    (void)hx_owned_free(ctx, km->owned, d_old);
    return rc;
}

int hx_ktmix_set_rayleigh(hx_ktmix* km, int s, const double* sigma, int is_h2o) {
    if (!km) return HX_E_ARG;
    int rc = km_slot_index(km, s, "hx_ktmix_set_rayleigh");
    if (rc) return rc;
    HX_REQUIRE(km->ctx, !(sigma && is_h2o), HX_E_ARG, "water vapour's cross-section is computed per node; it takes no sigma");
    const int kind = is_h2o ? 2 : (sigma ? 1 : 0);
    if (sigma) {
        rc = hx_h2d(km->ctx, km->sigma + (size_t)s * km->nbin, sigma, (size_t)km->nbin * 8);
        if (rc) return rc;
    }
    km->hkind[s] = kind;
    return hx_h2d(km->ctx, km->kind, km->hkind.data(), (size_t)km->ns * 4);
}

int hx_ktmix_run(hx_ktmix* km, const double* mmr, const double* vmr_scat) {
    if (!km) return HX_E_ARG;
    hx_context* ctx = km->ctx;
    HX_REQUIRE(ctx, km->have_grid, HX_E_STATE, "set the grid first");
    HX_REQUIRE(ctx, mmr && vmr_scat, HX_E_ARG, "null array");
    const size_t per = (size_t)km->ns * km->nodes;
    int rc = km_upload(km, km->mmr, mmr, per);
    if (!rc) rc = km_upload(km, km->vmr, vmr_scat, per);
    if (rc) return rc;
    std::vector<int> absorbers;
    for (int s = 0; s < km->ns; s++)
        if (km->slot[s]) absorbers.push_back(s);
    double ms_sum = 0.0, ms_scat = 0.0;
    rc = hx_timer_start(ctx);
    if (rc) return rc;
    if (absorbers.empty()) {
        rc = hx_memset0(ctx, km->kpoints, km->nodes * km->nc * 8);
        if (rc) return rc;
    }
    const int spans = hx_cdiv((long long)km->nc + 1, KM_SPAN);      // + 1: a row that starts 8 bytes off is shifted by one entry
    for (size_t a = 0; a < absorbers.size(); a += KM_G) {
        KmSum A;
        A.n = (int)std::min<size_t>(KM_G, absorbers.size() - a);
        for (int g = 0; g < KM_G; g++) {
            const int s = absorbers[std::min(a + g, absorbers.size() - 1)];
            A.k[g] = km->slot[s];
            A.m[g] = km->mmr + (size_t)s * km->nodes;
        }
        A.acc = km->kpoints; A.nc = (int)km->nc; A.from_acc = a > 0;
        for (size_t first = 0; first < km->nodes; first += 65535) {
            A.first_node = (int)first;
            const unsigned rows = (unsigned)std::min<size_t>(65535, km->nodes - first);
            k_ktmix_sum<<<dim3(spans, rows), KM_THREADS, 0, ctx->stream>>>(A);
            HX_LAUNCH_CHECK(ctx);
        }
    }
    rc = hx_timer_stop_ms(ctx, &ms_sum);
    if (rc) return rc;
    KmScat S;
    S.sigma = km->sigma; S.kind = km->kind; S.vmr = km->vmr; S.wave = km->wave; S.temp = km->temp; S.press = km->press;
    S.out = km->scat; S.ns = km->ns; S.nbin = km->nbin; S.np = km->np; S.nodes = km->nodes; S.m_h2o = KM_H2O_WEIGHT * HX_AMU;
    rc = hx_timer_start(ctx);
    if (rc) return rc;
    for (size_t first = 0; first < km->nodes; first += 65535) {
        S.first_node = (int)first;
        const unsigned rows = (unsigned)std::min<size_t>(65535, km->nodes - first);
        k_ktmix_scat<<<dim3(hx_cdiv(km->nbin, KM_THREADS), rows), KM_THREADS, 0, ctx->stream>>>(S);
        HX_LAUNCH_CHECK(ctx);
    }
    rc = hx_timer_stop_ms(ctx, &ms_scat);
    if (rc) return rc;
    km->timing[0] = ms_sum; km->timing[1] = ms_scat; km->timing[3] += 1.0;
    km->ran = true;
    return 0;
}

int hx_ktmix_get(hx_ktmix* km, const char* name, void* out, size_t out_bytes) {
    if (!km || !name || !out) return HX_E_ARG;
    hx_context* ctx = km->ctx;
    char* end = nullptr;
    const long s = strncmp(name, "species_", 8) == 0 ? strtol(name + 8, &end, 10) : 0;
    if (end && end != name + 8 && !*end) {
        if (s < 0 || s >= km->ns)
            return hx_fail(ctx, HX_E_ARG, "hx_ktmix_get: species slot %ld out of range, the object has %d", s, km->ns);
        if (!km->slot[s]) return hx_fail(ctx, HX_E_STATE, "hx_ktmix_get: species slot %ld holds no table", s);
        const hx_result row = {name, km->slot[s], km->nodes * km->nc * 8, true, nullptr};
        return hx_get_result(ctx, __func__, &row, 1, name, out, out_bytes);
    }
    const char* run_first = km->ran ? nullptr : "run first";
    const hx_result rows[] = {
        {"timing_ms", km->timing, sizeof km->timing, false, nullptr},
        {"kpoints", km->kpoints, km->nodes * km->nc * 8, true, run_first},
        {"scat_cross", km->scat, km->nodes * km->nbin * 8, true, run_first},
        {"kpoints_guard", km->kpoints + km->nodes * km->nc, km->nc * 8, true, nullptr},
        {"scat_cross_guard", km->scat + km->nodes * km->nbin, (size_t)km->nbin * 8, true, nullptr},
    };
    return hx_get_result(ctx, __func__, rows, 5, name, out, out_bytes);
}

}  // extern "C"
