/* helios_hip.h -- C-ABI of libhelios_hip.so, the MI355X (gfx950) implementation of the HELIOS
 * wavelength x layer radiative-transfer hot path.
 *
 * What this boundary replaces.  The reference has no FFI: its `Compute` class JIT-compiles
 * source/kernels.cu with PyCUDA (source/computation.py:34-37) and launches kernels by name with
 * `f(args..., block=..., grid=...)` + `cuda.Context.synchronize()`; device arrays are PyCUDA
 * `gpuarray.to_gpu(np_array)` / `cuda.mem_alloc(nbytes)` objects kept on `Store`
 * (source/quantities.py:463-665).  A maintainer of the reference binds THIS library with ctypes
 * instead (INTEGRATION.md shows the stub):
 *
 *   (1) hx_create/hx_destroy/hx_sync/hx_last_error        <- pycuda.autoinit, Context.synchronize
 *   (2) hx_alloc/hx_free/hx_h2d/hx_d2h/hx_d2d/hx_memset0  <- gpuarray.to_gpu, .get(), mem_alloc and the
 *                                                           "upload zeros" idiom (host_functions.py:1050)
 *   (3) one `hx_<kernel>` per reference kernel: SAME argument order as the `__global__` function,
 *       device pointers + scalars, no block/grid (launch geometry is the library's business)
 *   (4) hx_rt_*: the fused fast path (one call per refresh, one per iteration) that the shipped
 *       `helios_amd.computation.Compute.radiation_loop` uses by default
 *
 * Conventions: every function returns 0 on success, <0 for a HIP runtime error (-hipError_t),
 * >0 for a domain error (HX_E_*); hx_last_error() gives the text.  All arrays are fp64 unless
 * declared `int*`.  Pointers named *_dev / passed to hx_<kernel> are DEVICE pointers obtained from
 * hx_alloc.  Calls are asynchronous on the context's stream and ordered; hx_d2h and hx_sync block.
 * One host thread per context.  Array layouts are the reference's.
 */
#ifndef HELIOS_HIP_H
#define HELIOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hx_context hx_context;
typedef struct hx_rt hx_rt;

#define HX_E_ARG 1         /* invalid argument / unsupported dimension */
#define HX_E_RO_NY 2       /* random-overlap mixing holds 2 ... 20 Gauss points (hx_add_to_mixed_opac, the reference's kernel: 20 only) */
#define HX_E_UNSUPPORTED 3 /* configuration outside the fused path; use the per-stage entry points */
#define HX_E_STATE 4       /* call order violated (e.g. hx_rt_step before hx_rt_refresh) */

/* ---- (1) lifecycle ------------------------------------------------------------------------- */
int hx_create(int device_id, hx_context** out_ctx);
int hx_destroy(hx_context* ctx);
int hx_sync(hx_context* ctx);
const char* hx_last_error(hx_context* ctx);
int hx_device_name(hx_context* ctx, char* buf, int buflen);
/* Conditions the reference reports through device-side printf (kernels.cu:227 G_limiter, :1458 ff. negative fluxes,
 * :3385 random-overlap re-binning, :455 energy-budget correction) are counted in a per-context device record
 * instead.  The flux and G counters only run in calls that are given debug = 1 (the reference prints under the same
 * flag); the re-binning counter and the correction factor are always kept.  hx_diag_read blocks. */
typedef struct hx_diag {
    uint64_t negative_down_flux; /* entries < 0 in F_down_wg / Fc_down_wg after a flux solve */
    uint64_t negative_up_flux;   /* entries < 0 in F_up_wg / Fc_up_wg */
    uint64_t g_limited;          /* G+ / G- values clipped to +-1e8 */
    uint64_t ro_rebin_skipped;   /* Gauss points that met an already used interval in add_to_mixed_opac */
    double energy_correction;    /* factor applied by the last hx_corr_inc_energy (0 = none yet) */
    uint64_t ro_fixup_passes;    /* exact odd-even passes add_to_mixed_opac ran after its quantised-key sort (a cost
                                    figure: how often two pair sums of different rows agree to 2^-18) */
    uint64_t reserved[2];
} hx_diag;
int hx_diag_read(hx_context* ctx, hx_diag* out);
int hx_diag_reset(hx_context* ctx);
int hx_abi_version(void);
/* raw hipStream_t of the context (for interop with another runtime's stream guards) */
void* hx_stream(hx_context* ctx);
/* HIP-event timing on the context's stream (bench.py / profiling): record two marks, read ms */
int hx_timer_start(hx_context* ctx);
int hx_timer_stop_ms(hx_context* ctx, double* out_ms);

/* ---- (2) memory ---------------------------------------------------------------------------- */
int hx_alloc(hx_context* ctx, size_t nbytes, void** out_dptr);
int hx_free(hx_context* ctx, void* dptr);
int hx_h2d(hx_context* ctx, void* dptr, const void* hptr, size_t nbytes);
int hx_d2h(hx_context* ctx, void* hptr, const void* dptr, size_t nbytes);
int hx_d2d(hx_context* ctx, void* dst, const void* src, size_t nbytes);
int hx_memset0(hx_context* ctx, void* dptr, size_t nbytes);
int hx_mem_info(hx_context* ctx, size_t* out_free, size_t* out_total);
/* Host utility (no context, no device call): nrows rows "\n%-8g%-18.9g%-21.9g%-19.9g" of prefix[4 * r ...] followed by
 * ncols cells `cell_format` ("%-<width>[.<precision>]e" or "...g") of values[ncols * r ...] -- the rows of the reference's
 * per-bin output tables (source/write.py:576-714), formatted by `nthreads` threads.  *out_text is released with
 * hx_host_free. */
int hx_host_format_rows(const double* prefix, const double* values, int nrows, int ncols, const char* cell_format,
                        int nthreads, char** out_text, size_t* out_len);
void hx_host_free(void* p);

/* ---- (3) per-stage entry points: one per reference kernel ------------------------------------
 * Each comment gives the kernel it replaces (source/kernels.cu) and its launcher
 * (source/computation.py).                                                                      */

/* plancktable, kernels.cu:362 / computation.py:39 -- all ten p_iter launches in one call */
int hx_plancktable(hx_context* ctx, double* planck_grid, const double* lambda_edge,
                   const double* deltalambda, int nwave, double Tstar, int dim, int step);
/* corr_inc_energy, kernels.cu:420 / computation.py:62 */
int hx_corr_inc_energy(hx_context* ctx, double* planck_grid, double* starflux,
                       const double* deltalambda, int realstar, int nwave, double Tstar, int dim);
/* calc_total_g_0_of_gas_and_clouds, kernels.cu:472 / computation.py:331 */
int hx_calc_total_g_0_of_gas_and_clouds(hx_context* ctx, const double* scat_cross,
                                        const double* g_0_all_clouds,
                                        const double* scat_cross_all_clouds, double* g_0_tot,
                                        double g_0, int nbin, int nlay_or_nint);
/* temp_inter, kernels.cu:496 / computation.py:104 */
int hx_temp_inter(hx_context* ctx, const double* tlay, double* tint, int numinterfaces,
                  int itervalue);
/* opac_interpol, kernels.cu:524 / computation.py:119 */
int hx_opac_interpol(hx_context* ctx, const double* temp, const double* opactemp,
                     const double* press, const double* opacpress, const double* ktable,
                     double* opac, const double* crosstable, double* scat_cross, int npress,
                     int ntemp, int ny, int nbin, int nlay_or_nint);
/* meanmolmass_interpol, kernels.cu:649 / computation.py:163 */
int hx_meanmolmass_interpol(hx_context* ctx, const double* temp, const double* opactemp,
                            double* meanmolmass, const double* opac_meanmass, const double* press,
                            const double* opacpress, int npress, int ntemp, int ninterface);
/* kappa_interpol, kernels.cu:703 and cp_interpol, kernels.cu:761 / computation.py:199 */
int hx_kappa_interpol(hx_context* ctx, const double* temp, const double* entr_temp,
                      const double* press, const double* entr_press, double* kappa,
                      const double* entr_kappa, int entr_npress, int entr_ntemp, int nlay_or_nint);
int hx_cp_interpol(hx_context* ctx, const double* temp, const double* entr_temp,
                   const double* press, const double* entr_press, double* cp_lay,
                   const double* entr_cp, int entr_npress, int entr_ntemp, int nlayer);
/* entropy_interpol, kernels.cu:815 (log10 T grid) and phase_number_interpol, kernels.cu:869 /
 * computation.py:252, :273 -- diagnostics of the kappa-file modes */
int hx_entropy_interpol(hx_context* ctx, const double* temp, const double* entr_temp,
                        const double* press, const double* entr_press, double* entropy,
                        const double* entr_entropy, int entr_npress, int entr_ntemp, int nlayer);
int hx_phase_number_interpol(hx_context* ctx, const double* temp, const double* entr_temp,
                             const double* press, const double* entr_press, double* state,
                             const double* entr_state, int entr_npress, int entr_ntemp, int nlayer);
/* planck_interpol_layer, kernels.cu:923 / computation.py:294 */
int hx_planck_interpol_layer(hx_context* ctx, const double* temp, double* planckband_lay,
                             const double* planck_grid, const double* starflux, int realstar,
                             int numlayers, int nwave, int dim, int step);
/* planck_interpol_interface, kernels.cu:981 / computation.py:315 */
int hx_planck_interpol_interface(hx_context* ctx, const double* temp, double* planckband_int,
                                 const double* planck_grid, int numinterfaces, int nwave, int dim,
                                 int step);
/* calc_trans_iso, kernels.cu:1015 / computation.py:370 */
int hx_calc_trans_iso(hx_context* ctx, double* trans_wg, double* delta_tau_wg, double* M_term,
                      double* N_term, double* P_term, double* G_plus, double* G_minus,
                      const double* delta_colmass, const double* opac_wg_lay,
                      const double* meanmolmass_lay, const double* scat_cross_lay,
                      const double* abs_cross_all_clouds_lay,
                      const double* scat_cross_all_clouds_lay, double* delta_tau_all_clouds,
                      double* w_0, const double* g_0_tot_lay, int* scat_trigger, double g_0,
                      double epsi, double epsi2, double mu_star, double w_0_limit,
                      double w_0_scat_limit, int scat, int nbin, int ny, int nlayer, int clouds,
                      int scat_corr, int debug, double i2s_transition);
/* calc_trans_noniso, kernels.cu:1107 / computation.py:408 */
int hx_calc_trans_noniso(
    hx_context* ctx, double* trans_wg_upper, double* trans_wg_lower, double* delta_tau_wg_upper,
    double* delta_tau_wg_lower, double* M_upper, double* M_lower, double* N_upper, double* N_lower,
    double* P_upper, double* P_lower, double* G_plus_upper, double* G_plus_lower,
    double* G_minus_upper, double* G_minus_lower, const double* delta_col_upper,
    const double* delta_col_lower, const double* opac_wg_lay, const double* opac_wg_int,
    const double* meanmolmass_lay, const double* meanmolmass_int, const double* scat_cross_lay,
    const double* scat_cross_int, const double* abs_cross_all_clouds_lay,
    const double* abs_cross_all_clouds_int, const double* scat_cross_all_clouds_lay,
    const double* scat_cross_all_clouds_int, double* delta_tau_all_clouds_upper,
    double* delta_tau_all_clouds_lower, double* w_0_upper, double* w_0_lower,
    const double* g_0_tot_lay, const double* g_0_tot_int, int* scat_trigger, double g_0, double epsi,
    double epsi2, double mu_star, double w_0_limit, double w_0_scat_limit, int scat, int nbin, int ny,
    int nlayer, int clouds, int scat_corr, int debug, double i2s_transition);
/* calc_delta_z, kernels.cu:1247 / computation.py:464 */
int hx_calc_delta_z(hx_context* ctx, const double* tlay, const double* pint, const double* play,
                    const double* meanmolmass_lay, double* delta_z_lay, double g, int nlayer);
/* fdir_iso, kernels.cu:1265 / computation.py:484 */
int hx_fdir_iso(hx_context* ctx, double* F_dir_wg, const double* planckband_lay,
                const double* delta_tau_wg, const double* z_lay, double mu_star, double R_planet,
                double R_star, double a, int dir_beam, int geom_zenith_corr, int ninterface,
                int nbin, int ny);
/* fdir_noniso, kernels.cu:1313 / computation.py:504 */
int hx_fdir_noniso(hx_context* ctx, double* F_dir_wg, double* Fc_dir_wg,
                   const double* planckband_lay, const double* delta_tau_wg_upper,
                   const double* delta_tau_wg_lower, const double* z_lay, double mu_star,
                   double R_planet, double R_star, double a, int dir_beam, int geom_zenith_corr,
                   int ninterface, int nbin, int ny);
/* fband_iso, kernels.cu:1366 / computation.py:539 (one sweep) */
int hx_fband_iso(hx_context* ctx, double* F_down_wg, double* F_up_wg, const double* F_dir_wg,
                 const double* planckband_lay, const double* w_0, const double* M_term,
                 const double* N_term, const double* P_term, const double* G_plus,
                 const double* G_minus, const double* surf_albedo, const double* g_0_tot_lay,
                 double g_0, int singlewalk, double Rstar, double a, int numinterfaces, int nbin,
                 double f_factor, double mu_star, int ny, double epsi, int dir_beam, int clouds,
                 int scat_corr, int debug, double i2s_transition);
/* fband_noniso, kernels.cu:1521 / computation.py:573 (one sweep) */
int hx_fband_noniso(hx_context* ctx, double* F_down_wg, double* F_up_wg, double* Fc_down_wg,
                    double* Fc_up_wg, const double* F_dir_wg, const double* Fc_dir_wg,
                    const double* planckband_lay, const double* planckband_int,
                    const double* w_0_upper, const double* w_0_lower,
                    const double* delta_tau_wg_upper, const double* delta_tau_wg_lower,
                    const double* delta_tau_all_clouds_upper,
                    const double* delta_tau_all_clouds_lower, const double* M_upper,
                    const double* M_lower, const double* N_upper, const double* N_lower,
                    const double* P_upper, const double* P_lower, const double* G_plus_upper,
                    const double* G_plus_lower, const double* G_minus_upper,
                    const double* G_minus_lower, const double* surf_albedo,
                    const double* g_0_tot_lay, const double* g_0_tot_int, double g_0,
                    int singlewalk, double Rstar, double a, int numinterfaces, int nbin,
                    double f_factor, double mu_star, int ny, double epsi, double delta_tau_limit,
                    int dir_beam, int clouds, int scat_corr, int debug, double i2s_transition);
/* fband_matrix_iso, kernels.cu:1803 / computation.py:625 -- the flux solve as one tridiagonal system
 * (Thomas algorithm) per spectral point; alpha .. d_prime are caller-provided work arrays
 * (ny*nbin*nlayer each for alpha, beta and the two sources; ny*nbin*2*ninterface for c_prime, d_prime).
 * The surface albedo must be > 0 (the reference's reader enforces >= 1e-8, read.py:1261). */
int hx_fband_matrix_iso(hx_context* ctx, double* F_down_wg, double* F_up_wg, const double* F_dir_wg,
                        const double* planckband_lay, const double* w_0, const double* M_term,
                        const double* N_term, const double* P_term, const double* G_plus,
                        const double* G_minus, const double* g_0_tot_lay, double* alpha, double* beta,
                        double* source_term_down, double* source_term_up, double* c_prime,
                        double* d_prime, const int* scat_trigger, const double* trans_wg,
                        const double* surf_albedo, double g_0, int singlewalk, double Rstar, double a,
                        int numinterfaces, int nbin, double f_factor, double mu_star, int ny,
                        double epsi, int dir_beam, int clouds, int scat_corr, int debug,
                        double i2s_transition);
/* fband_matrix_noniso, kernels.cu:2028 / computation.py:667 (work arrays: 2*nlayer planes for alpha,
 * beta, sources; 4*ninterface-2 planes for c_prime, d_prime) */
int hx_fband_matrix_noniso(
    hx_context* ctx, double* F_down_wg, double* F_up_wg, double* Fc_down_wg, double* Fc_up_wg,
    const double* F_dir_wg, const double* Fc_dir_wg, const double* planckband_lay,
    const double* planckband_int, const double* w_0_upper, const double* w_0_lower,
    const double* delta_tau_wg_upper, const double* delta_tau_wg_lower,
    const double* delta_tau_all_clouds_upper, const double* delta_tau_all_clouds_lower,
    const double* M_upper, const double* M_lower, const double* N_upper, const double* N_lower,
    const double* P_upper, const double* P_lower, const double* G_plus_upper,
    const double* G_plus_lower, const double* G_minus_upper, const double* G_minus_lower,
    const double* g_0_tot_lay, const double* g_0_tot_int, double* alpha, double* beta,
    double* source_term_down, double* source_term_up, double* c_prime, double* d_prime,
    const int* scat_trigger, const double* trans_wg_upper, const double* trans_wg_lower,
    const double* surf_albedo, double g_0, int singlewalk, double Rstar, double a, int numinterfaces,
    int nbin, double f_factor, double mu_star, int ny, double epsi, double delta_tau_limit,
    int dir_beam, int clouds, int scat_corr, int debug, double i2s_transition);
/* integrate_flux_double, kernels.cu:2428 / computation.py:731 (deterministic summation order) */
int hx_integrate_flux(hx_context* ctx, const double* deltalambda, double* F_down_tot,
                      double* F_up_tot, double* F_net, const double* F_down_wg,
                      const double* F_up_wg, const double* F_dir_wg, double* F_down_band,
                      double* F_up_band, double* F_dir_band, const double* gauss_weight, int nbin,
                      int numinterfaces, int ny);
/* rad_temp_iter, kernels.cu:2606 / computation.py:759 */
int hx_rad_temp_iter(hx_context* ctx, const double* F_down_tot, const double* F_up_tot,
                     const double* F_net, double* F_net_diff, double* tlay, const double* play,
                     const double* tint, const double* pint, int* abrt, double* T_store,
                     double* deltat_prefactor, const double* F_add_heat_lay,
                     const double* F_add_heat_sum, double* F_smooth, double* F_smooth_sum,
                     const double* c_p_lay, const double* meanmolmass_lay, int itervalue,
                     double f_factor, int foreplay, double g, int numlayers, double physical_tstep,
                     double local_limit, int adapt_interval, int smooth, int dim, int step,
                     double F_intern, int no_atmo);
/* conv_temp_iter, kernels.cu:2768 / computation.py:799 */
int hx_conv_temp_iter(hx_context* ctx, const double* F_down_tot, const double* F_up_tot,
                      const double* F_net, double* F_net_diff, double* tlay, const double* play,
                      const double* pint, double* T_store, double* deltat_prefactor,
                      const int* marked_red, const double* F_add_heat_lay, double* F_smooth,
                      double* F_smooth_sum, int numlayers, int itervalue, int adapt_interval,
                      int smooth, double F_intern);
/* integrate_optdepth_transmission_{iso,noniso}, kernels.cu:2888/:2916 / computation.py:1176 */
int hx_integrate_optdepth_transmission_iso(hx_context* ctx, const double* trans_wg,
                                           double* trans_band, const double* delta_tau_wg,
                                           double* delta_tau_band, const double* gauss_weight,
                                           int nbin, int nlayer, int ny);
int hx_integrate_optdepth_transmission_noniso(
    hx_context* ctx, const double* trans_wg_upper, const double* trans_wg_lower, double* trans_band,
    const double* delta_tau_wg_upper, const double* delta_tau_wg_lower, double* delta_tau_band,
    const double* gauss_weight, double* delta_tau_all_clouds,
    const double* delta_tau_all_clouds_upper, const double* delta_tau_all_clouds_lower, int nbin,
    int nlayer, int ny);
/* calc_contr_func_{iso,noniso}, kernels.cu:2951/:2987 / computation.py:1216 */
int hx_calc_contr_func_iso(hx_context* ctx, const double* trans_wg, double* trans_weight_band,
                           double* contr_func_band, const double* gauss_weight,
                           const double* planckband_lay, double epsi, int nbin, int nlayer, int ny);
int hx_calc_contr_func_noniso(hx_context* ctx, const double* trans_wg_upper,
                              const double* trans_wg_lower, double* trans_weight_band,
                              double* contr_func_band, const double* gauss_weight,
                              const double* planckband_lay, double epsi, int nbin, int nlayer,
                              int ny);
/* calc_mean_opacities, kernels.cu:3024 / computation.py:1254 */
int hx_calc_mean_opacities(hx_context* ctx, double* planck_opac_T_pl, double* ross_opac_T_pl,
                           double* planck_opac_T_star, double* ross_opac_T_star,
                           const double* opac_wg_lay, const double* abs_cross_all_clouds_lay,
                           const double* meanmolmass_lay, const double* planckband_lay,
                           const double* opac_interwave, const double* opac_deltawave,
                           const double* T_lay, const double* gauss_weight, const double* gauss_y,
                           double* opac_band_lay, int nlayer, int nbin, int ny, double T_star);
/* integrate_beamflux, kernels.cu:3119 / computation.py:1283 */
int hx_integrate_beamflux(hx_context* ctx, double* F_dir_tot, const double* F_dir_band,
                          const double* deltalambda, const double* gauss_weight, int nbin,
                          int numinterfaces);
/* opac_species_interpol, kernels.cu:3209 / computation.py:1298 */
int hx_opac_species_interpol(hx_context* ctx, const double* temp, const double* opactemp,
                             const double* press, const double* opacpress,
                             const double* opac_opacity_pretab, double* opac_spec_wg, int npress,
                             int ntemp, int ny, int nbin, int nlay_or_nint);
/* add_to_mixed_opac, kernels.cu:3263 / computation.py:1338 */
int hx_add_to_mixed_opac(hx_context* ctx, const double* vmr, const double* opac_spec,
                         double* opac_wg, const double* meanmolmass, const double* gauss_weight,
                         const double* gauss_y, double mass_spec, int s, int ro_method, int ny,
                         int nbin, int nlay_or_nint);
/* the same with random overlap for any 2 <= ny <= 20 (the reference's rule with 20 -> ny, 400 -> ny * ny): ny == 20, ny == 1,
 * correlated-k and ny > 20 are hx_add_to_mixed_opac's */
int hx_add_to_mixed_opac_ny(hx_context* ctx, const double* vmr, const double* opac_spec,
                            double* opac_wg, const double* meanmolmass, const double* gauss_weight,
                            const double* gauss_y, double mass_spec, int s, int ro_method, int ny,
                            int nbin, int nlay_or_nint);
/* calc_h2o_scat, kernels.cu:3404 / computation.py:1390 */
int hx_calc_h2o_scat(hx_context* ctx, const double* temp, const double* press, const double* wave,
                     double* scat_cross, const double* vmr, double mass_h2o, int nbin,
                     int nlay_or_nint);
/* add_to_mixed_scat, kernels.cu:3444 / computation.py:1425 */
int hx_add_to_mixed_scat(hx_context* ctx, const double* vmr, const double* scat_cross_spec,
                         double* scat_cross, int nbin, int nlay_or_nint);
/* Transit depth spectrum of a column (csrc/stage_transit.hip; not in the reference -- the contract is README, "Transit depth
 * spectrum").  nshell homogeneous spherical shells with the ascending boundaries zb[0 .. nshell] (altitudes, z = 0 at radius R0);
 * one chord per shell, through its centre.
 *   isothermal layers:  nshell = nlayer, shell i = layer i; delta_tau_wg[c + ny*nbin*i] (c = y + ny*x), delta_tau_clouds[x + nbin*i],
 *                       the two `_upper` pointers null
 *   otherwise:          nshell = 2 nlayer, shell 2i = the lower half of layer i (delta_tau_wg, delta_tau_clouds: the `_lower`
 *                       arrays of the run), shell 2i + 1 = its upper half (the `_upper` arrays); same layouts
 * Out: A[nbin] the occulting area above zb[0] divided by pi, T_floor[nbin] the band transmission of the deepest chord and,
 * unless null, T_band[x + nbin*j] that of every chord j.  `work` holds hx_transit_work_doubles(nshell, nbin) doubles (path
 * lengths, thicknesses, T_band when it is not asked for).  A thread carries hx_transit_chord_block() chords in registers.
 * Any number of shells (up to 2^31 - 1 workgroups); 1 <= ny <= 256.  All pointers are device pointers. */
int hx_transit_chord_block(void);
int64_t hx_transit_work_doubles(int nshell, int nbin);
int hx_transit_depth(hx_context* ctx, const double* delta_tau_wg, const double* delta_tau_wg_upper,
                     const double* delta_tau_clouds, const double* delta_tau_clouds_upper, const double* zb,
                     const double* gauss_weight, double R0, int nbin, int ny, int nshell, double* work, double* A,
                     double* T_floor, double* T_band);
/* Angular emission spectrum of a column (csrc/stage_emission.hip; not in the reference -- the contract is README, "Angular
 * emission spectrum"): the intensity leaving the top of the atmosphere along `nangle` emission angles, by the formal solution
 * with a source linear in tau per shell, built from the Planck values and the run's own spectral fluxes.
 *   isothermal layers:  one shell per layer; delta_tau_wg[c + ny*nbin*i] (c = y + ny*x), delta_tau_clouds[x + nbin*i],
 *                       w_0[c + ny*nbin*i]; the three `_upper` pointers, planckband_int and the Fc_* pointers null
 *   otherwise:          two shells per layer: delta_tau_wg, delta_tau_clouds, w_0 are the `_lower` arrays of the run, the
 *                       `_upper` pointers its `_upper` arrays; Fc_*[c + ny*nbin*i] the fluxes at the layer centres
 * planckband_lay[i + x*(nlayer+2)], planckband_int[i + x*(nlayer+1)]; F_*_wg[c + ny*nbin*i] at the nlayer + 1 interfaces.
 * F_dir_wg (and Fc_dir_wg) null: no beam, `beta` is ignored.  mu_inv[m] = 1 / mu_m, m < nangle <= 16.
 * Out: I_band[x + nbin*m] and, unless null, I_wg[c + ny*nbin*m] before the Gauss sum.  1 <= ny <= 256.  All pointers are
 * device pointers. */
int hx_emission_angles(hx_context* ctx, const double* delta_tau_wg, const double* delta_tau_wg_upper,
                       const double* delta_tau_clouds, const double* delta_tau_clouds_upper, const double* w_0,
                       const double* w_0_upper, const double* planckband_lay, const double* planckband_int,
                       const double* F_up_wg, const double* F_down_wg, const double* F_dir_wg, const double* Fc_up_wg,
                       const double* Fc_down_wg, const double* Fc_dir_wg, const double* gauss_weight,
                       const double* mu_inv, double beta, int nbin, int ny, int nlayer, int nangle, double* I_band,
                       double* I_wg);

/* ---- (4) fused fast path --------------------------------------------------------------------
 * One hx_rt object = one batch of `ncol` independent atmosphere columns (planets / T-P profiles of
 * a parameter sweep) that share wavelength grid, Gauss points and opacity tables.  Non-isothermal
 * layers, iterative flux solver (the reference's defaults for an iterative run, param.dat:28,:109).
 *
 *   hx_rt_create            allocate the device-resident state (tiles, node arrays, per-column vectors)
 *   hx_rt_set_*             hand over shared tables / per-column inputs (copied to the device once)
 *   hx_rt_refresh           the every-10th-iteration block of radiation_loop (computation.py:860-879):
 *                           opacity interpolation or on-the-fly mixing, transmission coefficients,
 *                           delta z / altitude, direct beam  ->  compact coefficient tiles
 *   hx_rt_step              one iteration (computation.py:856-857, :880-888, :926-932): T_int, Planck
 *                           interpolation, (3*scat+1) two-stream sweeps, quadrature, totals, temperature
 *                           step, per-column convergence count -- no host round trip
 *   hx_rt_get / hx_rt_export_* read results back in the REFERENCE's layouts (hx_rt_get also: "flux_launch_policy",
 *                           two doubles -- whether the flux kernel's launches walk the grid back and forth and how
 *                           many MiB of up-flux state a launch leaves in the Infinity Cache; a choice of the batch,
 *                           HELIOS_RT_SERPENTINE / HELIOS_RT_STATE_CACHE_MB override it, results do not depend on it)
 */
typedef struct hx_rt_dims {
    int32_t nbin, ny, nlayer, ncol;
    int32_t ntemp, npress;        /* opacity-table grid */
    int32_t plancktable_dim, plancktable_step;
    int32_t nspecies;             /* 0 = premixed table; >0 = on-the-fly mixing of that many species */
    int32_t reserved[7];
} hx_rt_dims;

typedef struct hx_rt_flags {
    int32_t scat, dir_beam, clouds, scat_corr, geom_zenith_corr, smooth, real_star, planet_type_gas;
    int32_t kcoeff_mixing_ro;     /* 1 = random overlap, 0 = correlated-k (param.dat:110) */
    int32_t debug;
    int32_t iso;                  /* 1 = isothermal layers (fband_iso / calc_trans_iso / fdir_iso), read.py:888-935 */
    int32_t singlewalk;           /* 1 = post-processing run type: 1000*scat+1 sweeps, no temperature iteration
                                     (computation.py:531-537) */
    int32_t matrix;               /* 1 = `flux calculation method = matrix`: one tridiagonal solve per spectral point and
                                     iteration (fband_matrix_*, computation.py:625-710) instead of the sweeps.  The batch
                                     then holds the reference's per-half-layer arrays (calc_trans_*' outputs, ~20 arrays of
                                     ny*nbin*nlayer doubles per column) in place of the compact coefficient tiles */
    int32_t coef_fp32;            /* 1 = `precision = single`: the coefficient planes (alpha, beta, u', v', dd, du) are stored
                                     in fp32 -- rounded once when written, widened to fp64 when read; all arithmetic and every
                                     other array stay fp64.  The matrix method and tilings without an fp32 variant (columns of
                                     more than 416 layers, 832 isothermal) keep fp64 planes; hx_rt_get(rt, -1,
                                     "coef_plane_bytes", &int32, 4) says which width is in use (4 or 8).
                                     hx_rt_get(rt, -1, "flux_tiling", int32[14], 56) reads the batch's tiling: {k, ROWS,
                                     threads, nparts, nxb, ypb, NW, nplane, has_vp, pl_vp, pl_dd, coef_tpb, coef_bytes,
                                     generic_scans} -- coef_tpb the tiles per workgroup of the coefficient kernel that runs
                                     (after HELIOS_RT_COEF_TPB and the LDS limits), coef_bytes 4 or 8 as above.
                                     hx_rt_get(rt, col, "coef_planes", buf, nbytes) copies column col's coefficient planes
                                     as the coefficient kernel wrote them at the last refresh: coef_bytes-wide elements
                                     laid out [tile][plane][row][lane] (64 lanes, ROWS rows, nplane planes); fp32 planes
                                     in their stored coding (csrc/plane_code.h) */
    int32_t reserved[2];
    double epsi, epsi2, g_0, i2s_transition, w_0_limit, w_0_scat_limit, delta_tau_limit;
    double reserved_d[9];
} hx_rt_flags;

/* per-column scalars, host array of ncol structs */
typedef struct hx_rt_column {
    double g, a, R_planet, R_star, T_star, f_factor, mu_star, F_intern;
    double rad_convergence_limit, physical_tstep;
    int32_t adapt_interval, foreplay, no_atmo, reserved_i;
    double reserved_d[4];
} hx_rt_column;

int hx_rt_struct_sizes(int* dims_size, int* flags_size, int* column_size);
/* nlayer >= 1.  A one-layer batch takes every input and builds and returns cloud planes; hx_rt_refresh, hx_rt_step, hx_rt_run,
 * hx_rt_kappa_cp_refresh and the hx_rt_conv_* calls need two layers and return HX_E_UNSUPPORTED for it, before any launch. */
int hx_rt_create(hx_context* ctx, const hx_rt_dims* dims, const hx_rt_flags* flags,
                 const hx_rt_column* columns, hx_rt** out_rt);
int hx_rt_destroy(hx_rt* rt);
/* shared (per batch) host inputs */
int hx_rt_set_grid(hx_rt* rt, const double* opac_interwave, const double* opac_deltawave,
                   const double* opac_wave, const double* gauss_y, const double* gauss_weight,
                   const double* ktemp, const double* kpress);
int hx_rt_set_premixed_tables(hx_rt* rt, const double* opac_k, const double* opac_scat_cross,
                              const double* opac_meanmass);
/* one absorbing/scattering species of the on-the-fly mix (index s in species-file order, the first
 * absorber at s = 0, read.py:1373).  opacity_pretab may be NULL for a pure scatterer; scat_cross[nbin]
 * may be NULL for a non-scatterer; is_h2o selects calc_h2o_scat; is_cia forces correlated-k
 * (computation.py:1343); in_mu = contributes to the mean molecular mass (host_functions.py:940) */
int hx_rt_set_species(hx_rt* rt, int s, const double* opacity_pretab, const double* scat_cross,
                      double weight, int is_h2o, int is_cia, int in_mu);
/* Synthetic tables (bench.py, tests; helios_amd/synthetic.py:ktable): kappa[t][p][x][y] = kxy[y + ny*x] * ftp[p + npress*t],
 * formed on the device -- one fp64 product per entry, the same bits as the host array -- instead of a 0.96 GB host table and
 * its copy per species.  Otherwise as hx_rt_set_species / hx_rt_set_premixed_tables (the reference reads its tables from
 * HDF5 files, source/read.py:1041-1103; these two have no counterpart there). */
int hx_rt_set_species_separable(hx_rt* rt, int s, const double* kxy, const double* ftp, const double* scat_cross,
                                double weight, int is_h2o, int is_cia, int in_mu);
int hx_rt_set_premixed_separable(hx_rt* rt, const double* kxy, const double* ftp, const double* opac_scat_cross,
                                 const double* opac_meanmass);
/* Further premixed table sets (a sweep over metallicity or C/O on the premixed path: one k-table file per chemistry).  A batch
 * holds ntab >= 1 sets -- k-table, weighted Rayleigh cross-sections, mean molecular mass, laid out as for
 * hx_rt_set_premixed_tables, which fills set 0 -- all on the grid of hx_rt_set_grid; each is resident once, whatever the number
 * of columns that read it.  hx_rt_add_premixed_tables appends a set and returns its index (the first set of a batch without one
 * gets index 0); sets are added before the first refresh.  hx_rt_set_column_table assigns a set to a column (col < 0: all
 * columns; default: set 0), in effect from the column's next refresh; the map is device data, so captured graphs stay valid.
 * Until that refresh the column's coefficients and what hx_rt_get returns for its opacities and Rayleigh cross-sections stay the
 * previous set's (a column whose loop has ended is not refreshed again); hx_rt_conv_adjust, which re-evaluates the mean
 * molecular mass of the current profile itself, reads the set assigned at its call.
 * hx_rt_get(rt, col, "premixed_table") reads a column's index back, hx_rt_get(rt, -1, "premixed_table_count") the number of
 * sets (one int32 each).  Errors (index out of range, an on-the-fly object, a set added after the first refresh, no device
 * memory for a further set) name the index and the count; the batch stays usable and destroyable. */
int hx_rt_add_premixed_tables(hx_rt* rt, const double* opac_k, const double* opac_scat_cross,
                              const double* opac_meanmass, int* out_index);
int hx_rt_set_column_table(hx_rt* rt, int col, int index);
/* A6 on the device: calculate_vmr_for_all_species + interpolate_grid_to_lay_or_int (source/host_functions.py:874-910).
 * vmr_pretab[p + npress * t] on the opacity tables' (T, P) grid, as source/read.py keeps it per FastChem species
 * (Species.vmr_pretab); the species' profile is then interpolated at every refresh from the device's temperatures,
 * bilinear in (T, log10 P), clamped at the table edges.  NULL returns the species to hx_rt_set_column_vmr's profiles. */
int hx_rt_set_species_vmr_table(hx_rt* rt, int s, const double* vmr_pretab);
/* the same per column: a parameter sweep gives every column its own chemistry (FastChem directory, metallicity, C/O --
 * source/read.py:577-606 reads one table per species and run), so the device keeps one table per (species, column);
 * col < 0 = all columns (what hx_rt_set_species_vmr_table does).  A column of a tabulated species that never received a
 * table reads zeros. */
int hx_rt_set_column_vmr_table(hx_rt* rt, int col, int s, const double* vmr_pretab);
/* per-column host inputs; col < 0 broadcasts to all columns.  vmr_* : [nspecies][nlayer] / [nspecies][ninterface] */
int hx_rt_set_column_profile(hx_rt* rt, int col, const double* p_lay, const double* p_int,
                             const double* T_lay, const double* surf_albedo,
                             const double* starflux);
int hx_rt_set_column_vmr(hx_rt* rt, int col, const double* vmr_lay, const double* vmr_int);
int hx_rt_set_column_clouds(hx_rt* rt, int col, const double* abs_cross_lay,
                            const double* abs_cross_int, const double* scat_cross_lay,
                            const double* scat_cross_int, const double* g_0_lay,
                            const double* g_0_int);
int hx_rt_set_column_heating(hx_rt* rt, int col, const double* F_add_heat_lay,
                             const double* F_add_heat_sum);
/* Cloud decks built on the device (helios_amd/csrc/clouds.hip), the counterpart of Cloud.cloud_pre_processing for the columns
 * of a batch.  hx_rt_add_mie_table makes one aerosol's Mie table resident -- lamda_mie[nw] in cm, strictly ascending;
 * scat[nr][nw] and absorb[nr][nw], one row per particle radius -- once per batch, however many columns or decks use it, and
 * returns its index.  hx_rt_set_column_cloud_decks describes the ndecks decks of column col (col < 0: all columns): per deck the
 * index of its Mie table, the radius weights radius_weight[ndecks][nr] (size-distribution density times radius interval) and the
 * mixing-ratio profiles f_lay[ndecks][nlayer], f_int[ndecks][ninterface] (f_int = NULL with iso = 1: the interface planes stay as
 * they are).  It forms the weighted sums over the radii, re-bins them onto the bins of hx_rt_set_grid under the contract of
 * tools.convert_spectrum with int_lambda = opac_interwave (absorption and scattering: type "log", evaluated as exp of a sum of
 * logarithms; the third spectrum, the scattering-weighted sum again: type "linear") and writes the column's six cloud planes:
 * sums over the decks in deck order of f * a, f * s and f * (g * s), products and sums rounded separately, the last divided by
 * the scattering sum where that is > 0.  The number of decks is fixed by the batch's first call.  Whichever of this call and
 * hx_rt_set_column_clouds comes last owns a column's planes.
 * hx_rt_get reads back "mie_table_count" (col = -1, one int32), the six planes under their names "abs_cross_all_clouds_lay",
 * "scat_cross_all_clouds_lay", "g_0_all_clouds_lay" ([nlayer][nbin]) and "..._int" ([ninterface][nbin]), and
 * "cloud_deck_spectra" ([ndecks][3][nbin]: absorption, scattering, third spectrum of the column's last deck call).
 * Errors name the offending value -- a table index out of range, nr not matching the table, clouds = 0 in the batch's flags,
 * wavelengths not ascending -- and launch nothing; the batch stays usable and destroyable. */
int hx_rt_add_mie_table(hx_rt* rt, const double* lamda_mie, int nw, const double* scat, const double* absorb, int nr,
                        int* out_index);
int hx_rt_set_column_cloud_decks(hx_rt* rt, int col, int ndecks, const int* mie_index, const double* radius_weight, int nr,
                                 const double* f_lay, const double* f_int);
int hx_rt_set_temperatures(hx_rt* rt, int col, const double* T_lay);
int hx_rt_set_convergence_limit(hx_rt* rt, int col, double limit);
/* builds the Planck table (+ incident-energy correction) on the device */
int hx_rt_build_planck_table(hx_rt* rt, int energy_correction);
int hx_rt_refresh(hx_rt* rt);
/* itervalue is the reference's quant.iter_value; step_temperature = 0 skips C5 (post-processing) */
int hx_rt_step(hx_rt* rt, int itervalue, int step_temperature);
/* nsteps iterations starting at `itervalue`, refreshing whenever iter % 10 == 0; no host sync */
int hx_rt_run(hx_rt* rt, int itervalue, int nsteps);
/* Convection loop (computation.py:992-1174) without host round trips.  One iteration = hx_rt_conv_adjust (convective
 * adjustment of the profile: host_functions.py:337-635 run by one workgroup per column) + hx_rt_conv_advance (T_int,
 * Planck, [refresh], sweeps, totals, mark_convective_layers, check_for_radiative_eq, conv_temp_iter).  The two halves
 * are separate so that a host step (FastChem mixing ratios of the adjusted profile) can sit between them; hx_rt_conv_run
 * chains them.  When the reference's loop condition turns false the column is frozen ("done" = 1, "iters_done" = the
 * reference's final iter_value).  Inputs beyond the radiation loop's: hx_rt_set_state "kappa_lay", "kappa_int",
 * "conv_layer" (flags persist between iterations), "dampara" (<= 0: the reference's automatic choice). */
/* kappa (= delad) and c_p tables of `kappa value = file | water_atmo` (read.py:1105-1193), value[p + npress * t]; with
 * them kappa_lay / kappa_int / c_p_lay follow the profile on the device (kappa_interpol, cp_interpol) */
int hx_rt_set_kappa_table(hx_rt* rt, const double* entr_temp, int entr_ntemp, const double* entr_press,
                          int entr_npress, const double* entr_kappa, const double* entr_c_p);
/* kappa and c_p of every column at its current temperatures (one column: Compute.interpolate_kappa_and_cp,
 * computation.py:199-250); the convection loop refreshes them itself every 10th iteration */
int hx_rt_kappa_cp_refresh(hx_rt* rt);
int hx_rt_conv_adjust(hx_rt* rt, int itervalue);
int hx_rt_conv_advance(hx_rt* rt, int itervalue);
int hx_rt_conv_run(hx_rt* rt, int itervalue, int nsteps);
/* number of layers (+ghost layer) per column whose convergence flag is set: out[ncol] (blocks) */
int hx_rt_converged_layers(hx_rt* rt, int* out_counts);
/* named read-back in the reference's layout: "T_lay","T_int","F_up_band","F_down_band",
 * "F_dir_band","F_up_tot","F_down_tot","F_net","F_net_diff","planckband_lay","planckband_int",
 * "opac_wg_lay","opac_wg_int","scat_cross_lay","scat_cross_int","meanmolmass_lay",
 * "meanmolmass_int","F_up_wg","F_down_wg","Fc_up_wg","Fc_down_wg","F_dir_wg","Fc_dir_wg","abort",
 * "delta_z_lay","z_lay","g_0_tot_lay","g_0_tot_int","delta_t_prefactor","T_store","F_smooth_sum",
 * "conv_layer","conv_unstable","marked_red" (int32[nlayer+1]),"done","iters_done","boa_source_factor" (the surface-emission
 * factor (1 - w0) / (E - w0) of the bottom half-layer per spectral point, [y + ny x], as the last refresh left it);
 * host-side, any column (-1):
 * "totals_chunks" (int32, the number of bin chunks the wavelength totals are summed in).
 * `out` is a HOST buffer of `out_bytes`; returns HX_E_ARG if the name is unknown or the size wrong. */
int hx_rt_get(hx_rt* rt, int col, const char* name, void* out, size_t out_bytes);
/* named write of host data into the batch: "T_lay", "c_p_lay", "delta_t_prefactor", "T_store", "done", "kappa_lay",
 * "kappa_int", "conv_layer", "conv_unstable", "add_heat_dens", "dampara" (per column, col = -1: all), "planck_grid",
 * "keep_down" (int32), and "restart" (int32): every column back to the state of a fresh batch -- the sweeps' flux state,
 * the time-step state and the convergence flags zeroed; temperatures stay the caller's. */
int hx_rt_set_state(hx_rt* rt, int col, const char* name, const void* in, size_t in_bytes);
/* device pointer of a named internal array (column `col`) for use with the per-stage entry points */
int hx_rt_device_ptr(hx_rt* rt, int col, const char* name, void** out_dptr);
/* the tiling hx_rt_create would choose for the flux kernel -- lanes per spectral point and half-layer rows per lane, i.e.
 * the instantiation k_rt_flux<rows, lanes> -- for a batch of `ncol` columns of `nlayer` layers (`iso`: one segment per
 * layer; `dir_beam`: the direct beam adds two planes per tile and favours fewer rows per lane).  Host only, no device
 * needed: tests hold the choice to the code objects' register notes. */
int hx_rt_flux_geometry(int nlayer, int iso, int dir_beam, int ny, int nbin, int ncol, int* out_lanes, int* out_rows);
/* algorithmic / actual HBM byte counts of the last refresh and step (for the roofline report) */
int hx_rt_traffic_model(hx_rt* rt, double* step_bytes_algorithmic, double* step_bytes_actual,
                        double* refresh_bytes_algorithmic, double* refresh_bytes_actual);
/* per-kernel HIP-event timing of the fused path: enable, then read the averages (ms) */
int hx_rt_profile(hx_rt* rt, int enable);
int hx_rt_profile_read(hx_rt* rt, const char* kernel, double* out_avg_ms, int* out_count);

/* ---- (5) premixed k-tables from the on-the-fly species set (csrc/premix.hip) -------------------------------------------------
 * Where every species' mixing ratio is a constant or a (T, P) table, the on-the-fly mix of a level is a function of (T, P)
 * alone; hx_premix_* evaluates it on the nodes of the species tables -- each cell of that grid divided into refine_t x
 * refine_p cells, uniform in T and log10 P -- with the refresh's own species loop (k_rt_mix_species: correlated-k for the
 * first absorber and CIA pairs, random overlap otherwise, or correlated-k throughout), and writes the tables a premixed run
 * reads: kpoints[t][p][x][y], the weighted Rayleigh cross-sections [t][p][x] and the mean molecular mass [t][p] in amu.
 * Works on the context: no batch, Planck table or columns.
 *
 *   hx_premix_create       dimensions; the species tables have ntemp x npress nodes, the output (ntemp-1)*refine_t+1 by
 *                          (npress-1)*refine_p+1.  correlated_k = 1: `kcoeff_mixing = correlated-k`
 *   hx_premix_set_grid     wave[nbin], Gauss points and weights [ny], the species tables' nodes (uniform in T and log10 P)
 *   hx_premix_set_species  as hx_rt_set_species (pretab NULL: no absorber; scat_cross NULL: no fixed Rayleigh cross-section),
 *                          with the mixing ratio as vmr_table[p + npress * t] on the species' nodes, or NULL and vmr_const.
 *                          Tables stay on the device between runs: a second chemistry needs hx_premix_set_species_vmr only
 *   hx_premix_run          builds the tables slab by slab (rows of temperature nodes; hx_premix_set_slab_rows: 0 = as many as
 *                          fit) into host memory; cell_error = 1 also evaluates the mix at every output cell's centre and
 *                          compares it with the premixed look-up's bilinear value there: max and mean over (x, y) of
 *                          |k_table - k_otf| / k_otf per cell (deterministic: tree reductions in a fixed order)
 *   hx_premix_get          "temperatures" [nT], "pressures" [nP], "kpoints", "scat_cross", "meanmolmass" (amu),
 *                          "cell_error_max", "cell_error_mean" [(nT-1)(nP-1), p fastest], "timing_ms" (double[4]: node
 *                          records, mixing launches, Rayleigh table, cell error incl. its mixing launches), "dims" (int32[2])
 */
typedef struct hx_premix hx_premix;
int hx_premix_create(hx_context* ctx, int nbin, int ny, int ntemp, int npress, int nspecies, int refine_t, int refine_p,
                     int correlated_k, hx_premix** out_pm);
int hx_premix_destroy(hx_premix* pm);
int hx_premix_set_grid(hx_premix* pm, const double* wave, const double* gauss_y, const double* gauss_w, const double* ktemp,
                       const double* kpress);
int hx_premix_set_species(hx_premix* pm, int s, const double* pretab, const double* scat_cross, const double* vmr_table,
                          double vmr_const, double weight, int absorbing, int scattering, int is_h2o, int is_cia, int in_mu);
/* synthetic species table kappa[t][p][x][y] = kxy[y + ny*x] * ftp[p + npress*t], formed on the device (hx_rt_set_species_separable) */
int hx_premix_set_species_separable(hx_premix* pm, int s, const double* kxy, const double* ftp);
int hx_premix_set_species_vmr(hx_premix* pm, int s, const double* vmr_table, double vmr_const);
int hx_premix_set_slab_rows(hx_premix* pm, int rows);
int hx_premix_run(hx_premix* pm, int cell_error);
int hx_premix_get(hx_premix* pm, const char* name, void* out, size_t out_bytes);

/* ---- (6) per-species k-tables from HELIOS-K opacities (csrc/ktable.hip; host logic in helios_amd/ktable.py) -------------------
 * Stage 1 of the reference's k-table tool: per wavelength bin and (T, P) point the opacities are floored at 1e-15, sorted by
 * (log10 k, weight w), the mid-points of w accumulated to y and log10 k interpolated linearly in y at the Gauss abscissae
 * (clamped to the end values).  The host decides once per species which points a bin holds and refuses an interior bin
 * without points; a bin with none is filled with the floor here, one with a single point takes its value.
 *
 *   hx_ktable_create    n_points of the spectral axis, bins, Gauss points, (T, P) points of the table, slabs per launch, and
 *                       the number of points up to which a bin is sorted in LDS (a power of two <= 16384; longer bins go
 *                       through a device scratch of 8 B per point)
 *   hx_ktable_set_grid  lamda[n_points] ascending (cm), per bin the range [bin_start, bin_end) of its points in lamda,
 *                       interfaces[n_bins + 1], gauss_y[n_gauss] on (0, 1).  The ranges ascend and are disjoint
 *                       (bin_start[x] >= bin_end[x - 1]); anything else is refused with HX_E_ARG
 *   hx_ktable_run       n_tp slabs of fp32 opacities [n_tp][n_points] in ascending WAVENUMBER (as HELIOS-K writes them: point
 *                       j of lamda is entry n_points - 1 - j) into the nodes first_tp ... of the table.  Returns when the
 *                       slabs are on the device; the kernel may still run
 *   hx_kt_run_device    the same for slabs [n_tp][n_points] that are on the device already (hx_lines_device_ptr): no upload, the
 *                       same checks and bookkeeping; a null pointer is refused.  The launch goes onto the context's stream, behind
 *                       the kernels that wrote the slabs and in front of those that overwrite them.  Returns when it is queued.  (The
 *                       name: the suite holds the set hx_ktable_* to the seven calls of the file route)
 *   hx_ktable_put       a table kpoints[n_tp][n_bins][n_gauss] made elsewhere, in place of hx_ktable_run's
 *   hx_ktable_regrid    bilinear in T and log10 P onto nt_new x np_new nodes (table node = p + np_old * t); per target node
 *                       the left source node and whether the axis is clamped there, as the reference's routine finds them
 *   hx_ktable_get       "kpoints" [y + ny*x + ny*nx*node], "kpoints_ip" (the same on the target nodes), "timing_ms"
 *                       (double[4]: ms in k_ktable_bins, its launches, ms in the re-gridding, (T, P) points done)
 */
typedef struct hx_ktable hx_ktable;
int hx_ktable_create(hx_context* ctx, int n_points, int n_bins, int n_gauss, int n_tp, int max_tp_per_launch, int lds_points,
                     hx_ktable** out_kt);
int hx_ktable_destroy(hx_ktable* kt);
int hx_ktable_set_grid(hx_ktable* kt, const double* lamda, const int* bin_start, const int* bin_end, const double* interfaces,
                       const double* gauss_y);
int hx_ktable_run(hx_ktable* kt, const void* opac_f32, int n_tp, int first_tp);
int hx_kt_run_device(hx_ktable* kt, const void* d_opac_f32, int n_tp, int first_tp);
int hx_ktable_put(hx_ktable* kt, const double* kpoints);
int hx_ktable_regrid(hx_ktable* kt, int nt_old, int np_old, int nt_new, int np_new, const int* t_left, const int* t_reduced,
                     const int* p_left, const int* p_reduced, const double* temp_old, const double* logp_old,
                     const double* temp_new, const double* logp_new);
int hx_ktable_get(hx_ktable* kt, const char* name, void* out, size_t out_bytes);

/* ---- (7) the analytic containers of the k-table tool: H- bound-free, H- free-free, He- (csrc/ktable.hip, k_ktable_continuum;
 * the contract and the host side are helios_amd/continuum.py) --------------------------------------------------------------------
 * Fills `rows` (T, P) rows of a container kpoints[t][p][x][y] from row first_row on (row = p + npress * t) into out[rows][nbin][ny]:
 * the opacity of bin x at (T, P), repeated over y.  All arrays are DEVICE arrays: wave[nbin] bin centres in cm, temp[ntemp],
 * press[npress], and the kind's coefficients (helios_amd/continuum_data.py holds the numbers):
 *   kind 0, H- bound-free   9:   m_H [g], mu_min, mu_0 [micron], C_0 .. C_5
 *   kind 1, H- free-free    76:  m_H, mu_min, mu_split, 5040 K, then for mu < mu_split and for the rest A[6], B[6], ..., F[6]
 *   kind 2, He-             302: m_He, the least and the greatest mu whose log10 lies in the table, log10 k outside it, 12
 *                                temperatures, 22 log10 mu, log10 k [12][22]
 * At most 65535 rows per call; the call returns when the kernel is launched.
 */
int hx_continuum_table(hx_context* ctx, int kind, const double* coef, int ncoef, const double* wave, int nbin, int ny,
                       const double* temp, int ntemp, const double* press, int npress, double* out, int first_row, int rows);

/* ---- (8) stellar spectra from model grids, re-binned onto the opacity grid (csrc/star.hip; the contract and the host side are
 * helios_amd/star.py) -----------------------------------------------------------------------------------------------------------
 * The reference's star tool: a star's spectrum is the blend of up to eight corner spectra of a model grid (or a spectrum put as
 * it is), re-binned onto the opacity grid by the linear mode of its convert_spectrum, bins that the table does not cover taking
 * pi x the analytic Planck integral over the bin.  All stars of one handle share the tabulated wavelengths and the grid.
 *
 *   hx_star_create      tabulated wavelengths, corner slots, stars, bins, and the number of trapezoids of a long bin that are
 *                       staged and summed at a time (a power of two of 64 ... 2048; part of the result's definition: a bin of
 *                       more than 16 points is the in-order sum of its chunks' tree sums, a shorter one the plain running sum)
 *   hx_star_add_corner  fp32 flux[n_points] of one corner file into a slot; a file that several stars use is added once
 *   hx_star_set_grid    lamda[n_points] ascending (cm), interfaces[n_bins + 1] ascending, and per interface: state 0 when it lies
 *                       below the first or above the last tabulated wavelength (its value stays 0), else 1 with p_bot = the
 *                       number of tabulated wavelengths below it, less one (-1 on the first one: the index wraps, as the
 *                       reference's does).  Indices that would read outside the table are refused with HX_E_ARG
 *   hx_star_set_star    star s = (sum over n_terms of ((f[slots[k]] * w[3k]) * w[3k + 1]) * w[3k + 2]) / divisor, in that order,
 *                       fp64; 1, 2, 4 or 8 terms, factors a branch does not have are 1
 *   hx_star_put_flux    fp64 flux[n_points] of star s as it is, in place of a blend
 *   hx_star_run         stages 1 (blend), 2 (Planck values at bb_temp[s]; 0 K: none, the values are 0; bb_prefactor[s] is
 *                       2 (k/h)^3 k T^4 / c^2 as the host forms it, hc and kb the host's constants), 4 (re-binning), or their
 *                       sum, for the stars 0 ... n_stars - 1.  Returns when the kernels are launched
 *   hx_star_get         "flux" [s][n_points], "converted" and "planck" [s][n_bins], "timing_ms" (double[4]: ms in k_star_blend,
 *                       in k_star_planck_bins, in the re-binning kernels; runs)
 */
typedef struct hx_star hx_star;
int hx_star_create(hx_context* ctx, int n_points, int n_corners, int n_stars, int n_bins, int chunk, hx_star** out_st);
int hx_star_destroy(hx_star* st);
int hx_star_add_corner(hx_star* st, int slot, const void* flux_f32);
int hx_star_set_grid(hx_star* st, const double* lamda, const double* interfaces, const int* p_bot, const int* state);
int hx_star_set_star(hx_star* st, int s, int n_terms, const int* slots, const double* weights, double divisor);
int hx_star_put_flux(hx_star* st, int s, const double* flux);
int hx_star_run(hx_star* st, int n_stars, const double* bb_temp, const double* bb_prefactor, double hc, double kb, int stages);
int hx_star_get(hx_star* st, const char* name, void* out, size_t out_bytes);

/* ---- (9) the mixing stage of the k-table tool: premixed tables by weighted sum (csrc/ktable_mix.hip; the contract and the host
 * side are helios_amd/ktable_mix.py) ------------------------------------------------------------------------------------------
 * Stage 2 of the reference's k-table tool (combination.py): kpoints[t][p][x][y] = sum over the absorbers, in slot order, of
 * m_s[t,p] * k_s[t][p][x][y], and scat[t][p][x] = sum over the scattering species, in slot order, of x_s[t,p] * sigma_s; one
 * rounded product and one rounded add per term.  The species' tables on the final grid stay on the device: a further chemistry
 * is one hx_ktmix_run.
 *
 *   hx_ktmix_create              bins, Gauss points, nodes of the final grid (node = p + np * t), species slots.  Allocates the
 *                                accumulator and the Rayleigh table, each with one guard row behind it that no kernel touches;
 *                                a species' slot is allocated when its table arrives.  An allocation that the device's free
 *                                memory cannot hold is refused with the number of bytes in the message
 *   hx_ktmix_set_grid            wave[nbin] bin centres (cm), temp[nt] (K), press[np] (dyne cm^-2), all > 0
 *   hx_ktmix_set_species         a table [nt][np][nbin][ny] on the final grid into slot s, uploaded in pieces of 64 MiB; NULL: the
 *                                species does not absorb (its slot is freed)
 *   hx_ktmix_set_species_native  a table on its own nt_old x np_old nodes: uploaded, re-gridded into the slot by k_ktable_regrid
 *                                (hx_ktable_regrid's plan arrays and its kernel), the native copy freed
 *   hx_ktmix_set_rayleigh        sigma[nbin] of slot s; is_h2o = 1 (with sigma NULL): water vapour, evaluated per node and bin
 *                                by stage 2's own formula; NULL and 0: the species contributes nothing
 *   hx_ktmix_run                 one chemistry: mmr[nspecies][nt * np] (the mass mixing ratios, read for the absorbing slots)
 *                                and vmr_scat[nspecies][nt * np]; both tables are refilled from zeros
 *   hx_ktmix_get                 "kpoints", "scat_cross", "species_<s>" (the slot), "kpoints_guard" [nbin * ny] and
 *                                "scat_cross_guard" [nbin] (the guard rows: every double the bit pattern 0x7ff8dead0badbeef),
 *                                "timing_ms" (double[4]: ms in k_ktmix_sum and in k_ktmix_scat of the last run, ms in
 *                                k_ktable_regrid so far, runs)
 */
typedef struct hx_ktmix hx_ktmix;
int hx_ktmix_create(hx_context* ctx, int nbin, int ny, int nt, int np, int nspecies, hx_ktmix** out_km);
int hx_ktmix_destroy(hx_ktmix* km);
int hx_ktmix_set_grid(hx_ktmix* km, const double* wave, const double* temp, const double* press);
int hx_ktmix_set_species(hx_ktmix* km, int s, const double* k_on_final_grid);
int hx_ktmix_set_species_native(hx_ktmix* km, int s, const double* k_native, int nt_old, int np_old, const int* t_left,
                                const int* t_reduced, const int* p_left, const int* p_reduced, const double* temp_old,
                                const double* logp_old, const double* temp_new, const double* logp_new);
int hx_ktmix_set_rayleigh(hx_ktmix* km, int s, const double* sigma, int is_h2o);
int hx_ktmix_run(hx_ktmix* km, const double* mmr, const double* vmr_scat);
int hx_ktmix_get(hx_ktmix* km, const char* name, void* out, size_t out_bytes);

/* ---- (10) Lorenz-Mie series per (size parameter, refractive index) pair (csrc/mie.hip; the contract and the host side are
 * helios_amd/mie.py) ----------------------------------------------------------------------------------------------------------
 * Per pair: N = floor(x + 4.05 x^(1/3) + 2) terms of a_n, b_n with D_n(m x) started at N from Lentz's continued fraction, taken
 * downward and kept in a bounded device buffer laid out [n][lane] per wavefront; Q_ext, Q_sca and g from the upward sums.  One
 * thread per pair, a wavefront's pairs consecutive in `order`; the buffer is filled and k_mie launched as often as the pairs need.
 *
 *   hx_mie_create   pairs per run at most, and the bytes of the D buffer (16 per term and pair, and 16 more per pair)
 *   hx_mie_run      x[n_pairs] finite and > 0, m_re > 0, m_im >= 0, order[n_pairs] a permutation of 0 ... n_pairs - 1: the
 *                   sequence in which the pairs are dealt to lanes (by N, descending, for wavefronts of equal loop lengths).
 *                   Refused with HX_E_ARG and the offending value in the message, before anything is launched: a value outside
 *                   these ranges, an order that is no permutation, a pair whose D_n alone exceed the buffer.  The handle stays
 *                   usable.  Returns when the results are there
 *   hx_mie_get      "q_ext", "q_sca", "g" (the first out_bytes / 8 pairs, in the order of the input), "guard" (double[5]: the
 *                   double behind each of the three result arrays and the two behind the D buffer, every one the bit pattern
 *                   0x7ff8dead0badbeef), "timing_ms" (double[2]: ms in k_mie and its launches, of the last run)
 */
typedef struct hx_mie hx_mie;
int hx_mie_create(hx_context* ctx, int n_pairs_max, size_t scratch_bytes, hx_mie** out_mie);
int hx_mie_destroy(hx_mie* mie);
int hx_mie_run(hx_mie* mie, int n_pairs, const double* x, const double* m_re, const double* m_im, const int* order);
int hx_mie_get(hx_mie* mie, const char* name, void* out, size_t out_bytes);

/* ---- (11) Line-by-line opacities of a line list on a spectral grid (csrc/lines.hip; the contract and the host side are
 * helios_amd/lines.py) -----------------------------------------------------------------------------------------------------------
 * Per (T, P) node: k_lines_prepare_nodes writes nu_0', s = S(T) a / sqrt pi, a = sqrt(ln 2) / alpha_D and y = max(a gamma_L, 1e-8) of
 * every line; k_lines_sum_nodes gives a workgroup a tile of consecutive points nu_i = nu_first + i dnu and adds, per point and in the
 * order of the list, s K(a (nu_i - nu_0'), y) of the lines with |nu_i - nu_0'| <= cutoff, K = Re w(x + i y) in four regions of |z|.
 * The host finds a tile's lines by binary search on nu_0, widened by cutoff + max |delta_air| P_atm.  No atomics.  The node is a grid
 * dimension: a launch takes up to nodes_per_launch nodes into fp32 slabs that stay on the device, for a consumer there
 * (hx_kt_run_device), and a row does not depend on the nodes beside it.
 *
 *   hx_lines_create     the largest number of lines, of spectral points, of nodes per launch and of nodes the handle holds: params
 *                       [nodes_per_launch][4][n_lines_max], the fp32 slabs [nodes_per_launch][n_points_max], with want_fp64 the
 *                       same rows before rounding, and the records of n_nodes_max nodes.  An allocation the device does not give is
 *                       refused with its byte count
 *   hx_lines_set_lines  the seven per-line arrays, sorted by nu0 (ties in any order the caller fixed); they stay resident.
 *                       Refused with HX_E_ARG and the line: a value that is not finite, nu0 <= 0, s_ref < 0, a list that is not
 *                       sorted, more lines than the handle holds
 *   hx_lines_set_nodes  T [K], P [dyne cm^-2], Q(T) per node and what the nodes share: Q(296), the molar mass [g/mol], the
 *                       self-broadening fraction, the cut-off [cm^-1], nu of point 0, dnu, the number of points.  A grid larger
 *                       than the handle holds or a value out of range is refused, with the node and the value.  The tiles' line
 *                       ranges are searched once per distinct pressure and go to the device with the records: the only upload of
 *                       a table
 *   hx_lines_run_nodes  queues the prepare and the sum of the nodes first_node ... first_node + n_nodes - 1, n_nodes <=
 *                       nodes_per_launch, on the context's stream: slab rows 0 ... n_nodes - 1, row stride n_points.  No copy and
 *                       no wait; the timers settle in the next call or in hx_lines_get.  Nodes beyond hx_lines_set_nodes' count or
 *                       more than the handle holds per launch are refused before any launch, with the counts
 *   hx_lines_device_ptr "slabs32": the slab buffer's device address
 *   hx_lines_get        of the rows of the last hx_lines_run_nodes: "slabs32" (float [rows][n_points], cm^2 g^-1), "kappa64" (double
 *                       [rows][n_points], want_fp64 only: a slab is it rounded once), "line_params" (double [rows][4][n_lines]:
 *                       nu_0', s, a, y); "timing_ms" (double[2]: ms in the two kernels summed since hx_lines_set_nodes)
 *   hx_lines_voigt      the sum's own K(x, y) at n pairs of host arrays, for the tests
 */
typedef struct hx_lines hx_lines;
int hx_lines_create(hx_context* ctx, int n_lines_max, int n_points_max, int nodes_per_launch, int n_nodes_max, int want_fp64,
                    hx_lines** out_lines);
int hx_lines_destroy(hx_lines* lines);
int hx_lines_set_lines(hx_lines* lines, int n_lines, const double* nu0, const double* s_ref, const double* gamma_air,
                       const double* gamma_self, const double* e_low, const double* n_air, const double* delta_air);
int hx_lines_set_nodes(hx_lines* lines, int n_nodes, const double* temp, const double* press, const double* q_t, double q_ref,
                       double molar_mass, double x_self, double cutoff, double nu_first, double dnu, int n_points);
int hx_lines_run_nodes(hx_lines* lines, int first_node, int n_nodes);
int hx_lines_device_ptr(hx_lines* lines, const char* name, void** out_dptr);
int hx_lines_get(hx_lines* lines, const char* name, void* out, size_t out_bytes);
int hx_lines_voigt(hx_context* ctx, int n, const double* x, const double* y, double* out);

/* ---- (12) Collision-induced absorption from the blocks of a HITRAN CIA file (csrc/cia.hip; the contract and the host side are
 * helios_amd/cia.py) -------------------------------------------------------------------------------------------------------------
 * A block is one temperature's table nu [cm^-1], k [cm^5 molecule^-2]; the blocks of one spectral range form a band, ordered by T.
 * Per (T, P) node and point nu_i = nu_first + i dnu: the band that holds nu_i, its two blocks around T (one beyond the band's
 * temperatures), each interpolated linearly in nu with both weights from differences and 0 outside its own points, the two
 * combined linearly in T, times (P / (K_B T)) N_A / M: cm^2 per gram of the partner of molar mass M.  k_cia_nodes takes the node as
 * a grid dimension, gives a workgroup a tile of consecutive points and stages the blocks' windows for the tile through LDS.
 *
 *   hx_cia_create      the largest number of tabulated values (all blocks together), of blocks and of spectral points, the nodes
 *                      per launch and in all; with_fp64 != 0: the handle also keeps the rows before rounding.  An allocation the
 *                      device does not give is refused with its byte count
 *   hx_cia_set_blocks  block b holds the values block_off[b] ... block_off[b + 1] - 1 of nu and k and stands at block_temp[b];
 *                      band n holds the blocks band_first[n] ... band_first[n + 1] - 1 and covers band_numin[n] ... band_numax[n].
 *                      Refused with HX_E_ARG and the place: a block of fewer than 2 points, nu that does not strictly ascend, a
 *                      value that is not finite, k < 0, temperatures of a band that do not strictly ascend, bands that are not in
 *                      ascending order or that overlap or touch, more than the handle holds.  The table stays resident
 *   hx_cia_set_nodes   T [K] and P [dyne cm^-2] per node, the partner's molar mass [g/mol], nu of point 0, dnu, the number of
 *                      points; a refusal names the node and the value.  The nodes' blocks and weights go to the device here
 *   hx_cia_run_nodes   queues the nodes first_node ... first_node + n_nodes - 1, n_nodes <= nodes_per_launch, on the context's
 *                      stream: rows 0 ... n_nodes - 1, row stride n_points.  No copy and no wait; the timer settles in the next
 *                      call or in hx_cia_get.  Nodes beyond hx_cia_set_nodes' count or more than the handle holds per launch are
 *                      refused before any launch, with the counts
 *   hx_cia_device_ptr  "slabs32": the fp32 slab buffer's device address (hx_kt_run_device)
 *   hx_cia_get         "slabs32" (float [n_nodes of the last hx_cia_run_nodes][n_points]), "kappa64" (double, the same rows
 *                      before rounding; with_fp64 only), "timing_ms" (double[2]: ms in k_cia_nodes and its launches since
 *                      hx_cia_set_nodes)
 */
typedef struct hx_cia hx_cia;
int hx_cia_create(hx_context* ctx, int n_values_max, int n_blocks_max, int n_points_max, int nodes_per_launch, int n_nodes_max,
                  int with_fp64, hx_cia** out_cia);
int hx_cia_destroy(hx_cia* cia);
int hx_cia_set_blocks(hx_cia* cia, int n_blocks, const int* block_off, const double* nu, const double* k, const double* block_temp,
                      int n_bands, const int* band_first, const double* band_numin, const double* band_numax);
int hx_cia_set_nodes(hx_cia* cia, int n_nodes, const double* temp, const double* press, double partner_mass, double nu_first,
                     double dnu, int n_points);
int hx_cia_run_nodes(hx_cia* cia, int first_node, int n_nodes);
int hx_cia_device_ptr(hx_cia* cia, const char* name, void** out_dptr);
int hx_cia_get(hx_cia* cia, const char* name, void* out, size_t out_bytes);

/* ---- (13) Opacities from an ExoMol line list: states, transitions and broadening per J'' (csrc/exomol.hip; the contract and the
 * host side are helios_amd/exomol.py) --------------------------------------------------------------------------------------------
 * A transition is (upper state, lower state, A); E, g and 2 J live in the state table, nu_0 = E[up] - E[low].  Per (T, P) node:
 * S = g' A / (8 pi c nu_0^2) exp(-c2 E'' / T) (1 - exp(-c2 nu_0 / T)) / Q(T); a transition is kept iff S >= S_min; of the kept ones,
 * in list order, nu_0, s = S a / sqrt pi, a = sqrt(ln 2) / alpha_D and y = max(a gamma_L, 1e-8) with gamma_L = P_bar sum_b x_b
 * gamma_b[2 J''] (296 / T)^n_b[2 J''] go to the node's params; the sum over them is section 11's (lines_sum_tile), so a row has the
 * bits hx_lines gives for the same four numbers.  k_exomol_count flags and counts per workgroup, k_exomol_scan turns the counts
 * into offsets (one workgroup per node, no atomics), k_exomol_prepare writes the kept transitions to their positions,
 * k_exomol_ranges searches per tile the compacted nu_0 for the lines within the cut-off, k_exomol_sum adds.  The node is a grid
 * dimension of all five, and nothing goes through the host between them.
 * Super-lines (hx_exomol_set_superlines; off unless set): a kept transition with S >= S_sl is strong and keeps its profile, one
 * with S_min <= S < S_sl is weak; the weak ones of a cell c = floor(nu_0 / d) become one super-line with S_c = sum S, gamma_c =
 * sum (S gamma) / S_c (0 where S_c = 0), nu_c = (c + 0.5) d and a, y, s by the statements above.  The node's list is the strong
 * transitions and the super-lines by the key (cell, kind, position), a cell's super-line before its strong transitions, never
 * longer than the kept list.  In place of count, scan and prepare: k_exomol_classify (S once per transition, strong and weak
 * counts per workgroup), k_exomol_cells (a wavefront per occupied cell: lane-strided sums in list order, a butterfly of shuffles
 * -- no atomics, one order in every launch -- and the mask of the cells that hold a weak transition), k_exomol_scan over the strong
 * counts and over the cells' counts, k_exomol_merge (every strong transition and every super-line to its position), then
 * k_exomol_ranges with a reach wider by d, since nu ascends only from cell to cell, and k_exomol_sum as it is.
 *
 *   hx_exomol_create          the largest number of states, transitions, broadeners and spectral points, the nodes per launch and
 *                             in all; want_fp64 != 0: the handle also keeps the rows before rounding.  Resident per launch row:
 *                             params [4][n_trans_max], the block counts and offsets, the tile ranges, the fp32 slab row.  An
 *                             allocation the device does not give is refused with its byte count
 *   hx_exomol_set_states      E [cm^-1], g and jidx = 2 J per state, in the order of the ids.  Refused with the state: a value that is
 *                             not finite, g < 0, jidx outside 0 ... 2^20, more states than the handle holds.  Transitions,
 *                             broadening and nodes set before are dropped
 *   hx_exomol_set_broadening  fraction [n_broadeners] and table [n_broadeners][n_jidx][gamma at 296 K and 1 bar, n]; n_jidx is the
 *                             states' largest jidx + 1.  Refused with the place: a fraction that is not > 0, gamma < 0, a value that
 *                             is not finite, another n_jidx, more broadeners than the handle holds
 *   hx_exomol_set_transitions up, low (0-based) and A [s^-1], sorted by nu_0 (ties in any order the caller fixed); they stay
 *                             resident, 24 bytes per transition with nu_0.  Refused with HX_E_ARG and the index: an id outside
 *                             the table, A that is not finite or < 0, nu_0 <= 0, a list that is not sorted, more transitions than
 *                             the handle holds.  Super-lines set before are dropped
 *   hx_exomol_set_superlines  after hx_exomol_set_transitions: S_sl [cm / molecule, >= 0, +inf makes every kept transition weak] and
 *                             the cell width d [cm^-1]; step = 0 turns super-lines off.  The host finds the occupied cells of the
 *                             resident list once; the arrays of this mode (S per transition and launch row, the cells' sums,
 *                             masks and counts) are allocated here, none without this call.  Nodes set before are dropped.
 *                             Every refusal but that of a handle without transitions leaves super-lines off and the nodes dropped.
 *                             Refused with the value: S_sl that is NaN or < 0, a step that is not finite or < 0, a largest
 *                             nu_0 / d at or above 2^31; hx_exomol_set_nodes refuses a step greater than its cut-off
 *   hx_exomol_set_nodes       T, P [dyne cm^-2], Q(T) per node, and what the nodes share: the molar mass [g/mol], the cut-off
 *                             [cm^-1], S_min [cm / molecule, >= 0], nu of point 0, dnu, the number of points.  A refusal names the
 *                             node and the value
 *   hx_exomol_run_nodes       queues the five steps for the nodes first_node ... first_node + n_nodes - 1, n_nodes <=
 *                             nodes_per_launch, on the context's stream: rows 0 ... n_nodes - 1, row stride n_points.  No copy and
 *                             no wait; the timers settle in the next call or in hx_exomol_get.  Nodes beyond hx_exomol_set_nodes'
 *                             count or more than the handle holds per launch are refused before any launch, with the counts
 *   hx_exomol_device_ptr      "slabs32": the fp32 slab buffer's device address (hx_kt_run_device)
 *   hx_exomol_get             of the last hx_exomol_run_nodes: "slabs32" (float [rows][n_points]), "kappa64" (double, the same
 *                             rows before rounding; want_fp64 only), "kept" (int per row), "line_params" (row after row,
 *                             double[4][kept[row]]: nu_0, s, a, y of the kept transitions), "tile_ranges" (int [rows][tiles][2]:
 *                             first and one past the last kept transition a tile walks); "timing_ms" (double[2]: ms in count +
 *                             scan + prepare + ranges and in the sum, summed since hx_exomol_set_nodes).  With super-lines:
 *                             "kept" is strong + weak, "superline_counts" (int [rows][3]: strong, weak, super-lines),
 *                             "line_params" holds double[4][strong + super-lines] per row in the list's order, "tile_ranges"
 *                             the widened ranges, and the new steps count into the first slot of "timing_ms"
 */
typedef struct hx_exomol hx_exomol;
int hx_exomol_create(hx_context* ctx, int n_states_max, int n_trans_max, int n_broadeners_max, int n_points_max,
                     int nodes_per_launch, int n_nodes_max, int want_fp64, hx_exomol** out_exomol);
int hx_exomol_destroy(hx_exomol* exomol);
int hx_exomol_set_states(hx_exomol* exomol, int n_states, const double* energy, const double* g, const int* jidx);
int hx_exomol_set_broadening(hx_exomol* exomol, int n_broadeners, int n_jidx, const double* fraction, const double* table);
int hx_exomol_set_transitions(hx_exomol* exomol, int n_trans, const int* up, const int* low, const double* a);
int hx_exomol_set_superlines(hx_exomol* exomol, double s_sl, double step);
int hx_exomol_set_nodes(hx_exomol* exomol, int n_nodes, const double* temp, const double* press, const double* q_t, double molar_mass,
                        double cutoff, double s_min, double nu_first, double dnu, int n_points);
int hx_exomol_run_nodes(hx_exomol* exomol, int first_node, int n_nodes);
int hx_exomol_device_ptr(hx_exomol* exomol, const char* name, void** out_dptr);
int hx_exomol_get(hx_exomol* exomol, const char* name, void* out, size_t out_bytes);

/* ---- (14) Equilibrium chemistry of the analytic C-H-O network (csrc/chem.hip; the contract and the host side are
 * helios_amd/chem.py) --------------------------------------------------------------------------------------------------------------
 * Per (chemistry, T, P) node: dG of the three net reactions linear in T between the rows of the table, K1 = exp(-dG1 / (R T)) / P / P,
 * K2 = exp(-dG2 / (R T)), K3 = exp(-dG3 / (R T)) / P / P with P in bar, the quintic in x = n_CH4 with the coefficients of chem.py,
 * its root in [x_min, 2 n_C] by bisection on the bit patterns of the ends, water from the oxygen balance, CO, CO2 and C2H2 from x and
 * water, the seven volume mixing ratios and mu.  k_chem_nodes: a thread per node, the chemistry is blockIdx.y, the rows go through
 * LDS once per workgroup, eight planes of results.  fp64, nothing contracted, no atomics.
 *
 *   hx_chem_create      the largest number of Gibbs rows (2 ... 1024, what the kernel stages in LDS), of nodes and of chemistries
 *                       per launch.  The results' allocation, when the device does not give it, is refused with its byte count
 *   hx_chem_set_table   T [K] strictly ascending and dG1, dG2, dG3 [J/mol] per row, and the gas constant [J/mol/K].  Refused with
 *                       the row: a value that is not finite, T that does not ascend, fewer than 2 rows, more than the handle
 *                       holds.  Nodes set before are dropped
 *   hx_chem_set_nodes   T [K] and P [bar] per node.  Refused with the node and the value: T outside the table's rows, P that is
 *                       not a finite number > 0, more nodes than the handle holds
 *   hx_chem_run         queues k_chem_nodes for n_chem abundance pairs (n_O, n_C per chemistry), He/H and the seven molar weights
 *                       (H2, He, H2O, CO, CH4, CO2, C2H2) on the context's stream.  Refused before any launch, with the value: an
 *                       abundance that is not a finite number > 0, He/H < 0, more chemistries than the handle holds, no nodes.  A
 *                       refused run leaves no result
 *   hx_chem_get         "vmr" (double [n_chem of the last hx_chem_run][8][n_nodes]: H2, He, H2O, CO, CH4, CO2, C2H2, mu),
 *                       "timing_ms" (double[2]: ms in k_chem_nodes and its launches, summed since hx_chem_set_nodes)
 */
typedef struct hx_chem hx_chem;
int hx_chem_create(hx_context* ctx, int max_rows, int max_nodes, int max_chem, hx_chem** out_chem);
int hx_chem_destroy(hx_chem* chem);
int hx_chem_set_table(hx_chem* chem, int n_rows, const double* temp, const double* dg1, const double* dg2, const double* dg3,
                      double gas_constant);
int hx_chem_set_nodes(hx_chem* chem, int n_nodes, const double* temp, const double* press_bar);
int hx_chem_run(hx_chem* chem, int n_chem, const double* o_abund, const double* c_abund, double he_to_h, const double* weights);
int hx_chem_get(hx_chem* chem, const char* name, void* out, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif
