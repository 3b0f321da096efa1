// k_rt_coef (fp64 coefficient planes) and k_rt_coef_f32 (fp32, `precision = single`: every value computed in fp64 and
// rounded to nearest once, when it is stored -- see plane_code.h): one source, included twice by rt_kernels.h (as
// rt_flux_kernel.inc).
// A third inclusion defines HX_COEF_FLAG so that the batch's flags are compile-time values (k_rt_coef_plain, rt_kernels.h):
// the same statements, of which the compiler then keeps one path.
#ifndef HX_COEF_FLAG
#define HX_COEF_FLAG(name) a.name
#define HX_COEF_FROM_TABLE a.from_table
#define HX_COEF_TEMPLATE template <int ROWS, int COEF_TPB>
#define HX_COEF_FLAG_DEFAULTS
#endif
HX_COEF_TEMPLATE
__global__ void __launch_bounds__(64 * COEF_TPB) HX_COEF_KERNEL(KArgs a HX_PLANE_ARG) {
    using CT = HX_PLANE_T;
    extern __shared__ __align__(16) double smem[];
    const int col = blockIdx.y;
    if (a.done[col]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntiles = a.nblk_x * a.nparts * a.NW;
    const int TS = COEF_TPB * a.S;                  // spectral points staged per workgroup
    const int TSP = TS;                             // row pitch of the staged opacities (padding it was measured: slower)
    const int NBX = a.coef_nbx;                     // bins this workgroup's tiles can touch (upper bound)
    double* sh_lay = smem;                          // [L][TSP]  opacity at layer centres
    double* sh_int = sh_lay + (size_t)a.L * TSP;    // [I][TSP]  opacity at interfaces
    double* sh_ray = sh_int + (size_t)a.I * TSP;    // [H][NBX]  Rayleigh cross-section of the half-layers
    double* sh_mu = sh_ray + (size_t)a.H * NBX;     // [H]       mean molecular mass of the half-layers
    double* sh_dc = sh_mu + a.H;                    // [H]       column mass of the half-layers
    // clouds: asymmetry parameter, absorption and scattering cross-sections of the half-layers, [H][NBX] each.  They do
    // not depend on the Gauss point; read per lane from the band arrays (level-strided: one 64-byte sector per double)
    // they were 18 scattered loads per half-layer -- config 5's k_rt_coef 7.4 ms per refresh against 2.9 ms expected
    // from config 2's rate
    const size_t ncl = HX_COEF_FLAG(cloud_lds) ? (size_t)a.H * NBX : 0;
    double* sh_g0 = sh_dc + a.H;
    double* sh_cab = sh_g0 + ncl;
    double* sh_csc = sh_cab + ncl;
    int* c_of_q = (int*)(sh_csc + ncl);             // [TS] global spectral-point index or -1
    int* x_of_q = c_of_q + TS;
    const size_t nc = (size_t)a.Y * a.X;
    const size_t wgI = nc * a.I;
    const int x_base = (blockIdx.x * COEF_TPB) / (a.NW * a.nparts) * a.nxb;  // first bin of the first tile
    // spectral points of this workgroup's tiles
    for (int q = threadIdx.x; q < TS; q += blockDim.x) {
        const int tl = blockIdx.x * COEF_TPB + q / a.S, s_in_wave = q % a.S;
        int c = -1, xq = x_base;
        if (tl < ntiles) {
            const int wv = tl % a.NW, part = (tl / a.NW) % a.nparts, bx = tl / (a.NW * a.nparts);
            const int s_local = wv * a.S + s_in_wave;
            const int xl = s_local / a.ypb, yl = s_local - xl * a.ypb;
            const int x = bx * a.nxb + xl, y = part * a.ypb + yl;
            if (s_local < a.G && x < a.X) { c = y + a.Y * x; xq = x; }
        }
        c_of_q[q] = c;
        x_of_q[q] = xq;
    }
    // per-level quantities of the half-layers.  Lower half h = 2i averages (interface i, centre i),
    // upper half h = 2i+1 (centre i, interface i+1); the sums are commutative, so one form serves both.
    {
        const double* mml = a.mmm_lay + (size_t)col * a.I;
        const double* mmi = a.mmm_int + (size_t)col * a.I;
        const double* dcu = a.dcol_u + (size_t)col * a.L;
        const double* dcl = a.dcol_l + (size_t)col * a.L;
        const double* pint = a.p_int + (size_t)col * a.I;
        const double grav = a.colpar[col].g;
        for (int h = threadIdx.x; h < a.H; h += blockDim.x) {
            if (HX_COEF_FLAG(iso)) {  // whole layers (calc_trans_iso, kernels.cu:1015-1104): delta_colmass of host_functions.py:733
                sh_mu[h] = mml[h];
                sh_dc[h] = (pint[h] - pint[h + 1]) / grav;
            } else {
                const int i = h >> 1, ii = i + (h & 1);
                sh_mu[h] = (mmi[ii] + mml[i]) / 2.0;
                sh_dc[h] = (h & 1) ? dcu[i] : dcl[i];
            }
        }
        // bin-major rows written by k_rt_half_bands: consecutive threads read consecutive half-layers of a bin
        for (int t = threadIdx.x; t < a.H * NBX; t += blockDim.x) {
            const int xs = t / a.H, h = t - xs * a.H, x = min(x_base + xs, a.X - 1);
            const size_t src = ((size_t)col * a.X + x) * a.H + h;
            sh_ray[(size_t)h * NBX + xs] = a.half_ray[src];
            if (HX_COEF_FLAG(cloud_lds)) {
                sh_g0[(size_t)h * NBX + xs] = a.half_g0[src];
                sh_cab[(size_t)h * NBX + xs] = a.half_cab[src];
                sh_csc[(size_t)h * NBX + xs] = a.half_csc[src];
            }
        }
    }
    __syncthreads();
    {
        // thread -> (staged point q0, a run of consecutive levels): consecutive levels mostly fall into
        // the same (T, P) cell of the table, whose four corners then stay in registers.  TS divides the
        // workgroup size (both are powers of two).
        const int q0 = threadIdx.x % TS, nrun = blockDim.x / TS, run = threadIdx.x / TS;
        const int cq = c_of_q[q0];
        if (HX_COEF_FROM_TABLE) {
            // premixed k-table look-up done while staging (kernels.cu:561-608): the opacity arrays of
            // the reference are not materialised on this path (hx_rt_get rebuilds them on demand)
            const size_t sp = nc, st = nc * a.npress;
            const double* ktable = a.coltab[col].k;   // the k-table of this column's set: col is uniform, one scalar load
            for (int pass = 0; pass < (HX_COEF_FLAG(iso) ? 1 : 2); pass++) {
                const int nlev = pass == 0 ? a.L : a.I;
                const TPIndex* tp = (pass == 0 ? a.tp_lay : a.tp_int) + (size_t)col * a.I;
                double* dst = pass == 0 ? sh_lay : sh_int;
                const int per = (nlev + nrun - 1) / nrun;
                const int l0 = run * per, l1 = min(nlev, l0 + per);
                int ktd = -1, ktu = -1, kpd = -1, kpu = -1;
                double c00 = 0, c01 = 0, c10 = 0, c11 = 0;
                // (the cell of the next level is requested while this level's corners are on their way: the look-up was a
                // chain of two dependent requests per level)
                TPIndex knext = tp[min(l0, nlev - 1)];
                for (int lev = l0; lev < l1; lev++) {
                    double v = 0.0;
                    const TPIndex k = knext;
                    knext = tp[min(lev + 1, nlev - 1)];
                    if (cq >= 0) {
                        if (k.tdown != ktd || k.tup != ktu || k.pdown != kpd || k.pup != kpu) {
                            const double* t0 = ktable + (size_t)cq + st * k.tdown;
                            const double* t1 = ktable + (size_t)cq + st * k.tup;
                            c00 = t0[sp * k.pdown];
                            c01 = t0[sp * k.pup];
                            c10 = t1[sp * k.pdown];
                            c11 = t1[sp * k.pup];
                            ktd = k.tdown; ktu = k.tup; kpd = k.pdown; kpu = k.pup;
                        }
                        v = blend_tp(c00, c01, c10, c11, k, false);
                    }
                    dst[(size_t)lev * TSP + q0] = v;
                }
            }
        } else {
            const double* opl = a.opac_wg_lay + col * wgI;
            const double* opi = a.opac_wg_int + col * wgI;
            for (int lev = run; lev < a.L; lev += nrun)
                sh_lay[(size_t)lev * TSP + q0] = cq >= 0 ? opl[(size_t)cq + nc * lev] : 0.0;
            if (!HX_COEF_FLAG(iso))
                for (int lev = run; lev < a.I; lev += nrun)
                    sh_int[(size_t)lev * TSP + q0] = cq >= 0 ? opi[(size_t)cq + nc * lev] : 0.0;
        }
    }
    __syncthreads();
    const int tl = blockIdx.x * COEF_TPB + wave;
    if (tl >= ntiles) return;
    const int j = lane % a.k, q = wave * a.S + lane / a.k;
    const int c = c_of_q[q], x = x_of_q[q], xs = x - x_base;
    const bool valid = c >= 0;
    const hx_rt_column cp = a.colpar[col];
    CT* ctile = HX_PLANES + col * a.coef_col + (size_t)tl * a.nplane * ROWS * 64;   // (strides in elements of CT)
    const double nmu = -cp.mu_star;
    const bool plain = HX_COEF_FLAG(clouds) != 1 && HX_COEF_FLAG(scat_corr) != 1 && HX_COEF_FLAG(g_0) == 0.0 && HX_COEF_FLAG(dir_beam) != 1;
    // The beam at the nodes of this lane's half-layers.  Half-layer h spans the nodes h (bottom) and h + 1 (top) -- even
    // nodes are interfaces (F_dir_wg), odd ones layer centres (Fc_dir_wg); isothermal: node = interface -- so the top value
    // of one row is the bottom value of the next: ONE load per row instead of two, requested a whole row of arithmetic
    // (divisions, exp, sqrt) before it is used.  (Loaded where they were used, the compiler sent all of a tile's beam
    // loads through one register pair, each waited for in turn: DESIGN.md section 4, tools/code_object_notes.py.)
    const double* Fd = a.F_dir_wg + col * wgI;
    const double* Fc = a.Fc_dir_wg + col * wgI;
    auto beam_at_node = [&](int n) -> double {
        if (!(HX_COEF_FLAG(dir_beam) == 1 && valid && n <= a.H)) return 0.0;
        if (HX_COEF_FLAG(iso)) return Fd[(size_t)c + nc * n];
        return (n & 1) ? Fc[(size_t)c + nc * (n >> 1)] : Fd[(size_t)c + nc * (n >> 1)];
    };
    double F_here = beam_at_node(j * ROWS), F_above = beam_at_node(j * ROWS + 1);
    // `flux calculation method = matrix`: a spectral point none of whose (half-)layers scatters (w0 <= w_0_scat_limit in all
    // of them: scat_trigger stays 0, kernels.cu:1102, :1240-1241) takes the solver's pure-absorption branch (:1969-2021,
    // :2286-2421): F_out = T F_in + 2 pi eps P' -- the same affine form with alpha = T, beta = 0 and sources that are again
    // u' B_near + v' B_far, so the planes serve both branches.  The trigger is a property of the whole column: the k lanes of a
    // point vote before any of them writes a coefficient.
    bool scatters = true;
    if (HX_COEF_FLAG(matrix)) {
        bool mine = false;
#pragma unroll 1
        for (int r = 0; r < ROWS; r++) {
            const int h = j * ROWS + r;
            if (valid && h < a.H) {
                const int i = HX_COEF_FLAG(iso) ? h : h >> 1;
                const bool lower = HX_COEF_FLAG(iso) || (h & 1) == 0;
                const int ii = lower ? i : i + 1;
                double ray = 0.0, csc = 0.0, cab = 0.0;
                if (HX_COEF_FLAG(cloud_lds)) {
                    cab = sh_cab[(size_t)h * NBX + xs];
                    csc = sh_csc[(size_t)h * NBX + xs];
                } else if (HX_COEF_FLAG(clouds) == 1) {
                    const size_t src = ((size_t)col * a.X + x) * a.H + h;
                    cab = a.half_cab[src];
                    csc = a.half_csc[src];
                }
                if (a.scat == 1) ray = sh_ray[(size_t)h * NBX + xs];
                const double o_l = sh_lay[(size_t)i * TSP + q], o_i = HX_COEF_FLAG(iso) ? o_l : sh_int[(size_t)ii * TSP + q];
                const double kap = HX_COEF_FLAG(iso) ? o_l : (lower ? (o_i + o_l) / 2.0 : (o_l + o_i) / 2.0);
                mine = mine || single_scat_albedo(ray + csc, kap * sh_mu[h] + cab, a.w_0_limit) > a.w_0_scat_limit;
            }
        }
        const unsigned long long votes = __ballot(mine);
        const unsigned long long group = a.k >= 64 ? ~0ull : ((1ull << a.k) - 1ull) << (lane - j);
        scatters = (votes & group) != 0ull;
        if (valid && j == 0) a.trigger[col * nc + c] = scatters ? 1 : 0;
    }
    for (int r = 0; r < ROWS; r++) {
        const int h = j * ROWS + r;
        double alpha = 1.0, beta = 0.0, up = 0.0, vp = 0.0, dd = 0.0, du = 0.0;
        const double Fbot = F_here, Ftop = F_above;
        F_here = F_above;
        F_above = beam_at_node(h + 2);      // the next row's top node: in flight during this row's arithmetic
        if (valid && h < a.H) {
            const int i = HX_COEF_FLAG(iso) ? h : h >> 1;
            const bool lower = HX_COEF_FLAG(iso) || (h & 1) == 0;
            // lower half averages (interface i, centre i); upper half (centre i, interface i+1); isothermal layers take
            // the layer-centre values as they are
            const int ii = lower ? i : i + 1;
            double g0 = HX_COEF_FLAG(g_0), ray = 0.0, csc = 0.0, cab = 0.0;
            if (HX_COEF_FLAG(cloud_lds)) {
                g0 = sh_g0[(size_t)h * NBX + xs];
                cab = sh_cab[(size_t)h * NBX + xs];
                csc = sh_csc[(size_t)h * NBX + xs];
            } else if (HX_COEF_FLAG(clouds) == 1) {  // the staged image would not fit the LDS: from the bin-major rows
                const size_t src = ((size_t)col * a.X + x) * a.H + h;
                g0 = a.half_g0[src];
                cab = a.half_cab[src];
                csc = a.half_csc[src];
            }
            if (a.scat == 1) ray = sh_ray[(size_t)h * NBX + xs];
            const double o_l = sh_lay[(size_t)i * TSP + q], o_i = HX_COEF_FLAG(iso) ? o_l : sh_int[(size_t)ii * TSP + q];
            const double kap = HX_COEF_FLAG(iso) ? o_l : (lower ? (o_i + o_l) / 2.0 : (o_l + o_i) / 2.0);
            const double mu = sh_mu[h], dcol = sh_dc[h];
            const double w0 = single_scat_albedo(ray + csc, kap * mu + cab, a.w_0_limit);
            // (ray / mu does not depend on the Gauss point.  k_rt_half_bands storing the quotient for k_rt_coef_plain to read was
            // measured: 404-414 -> 428-433 us per refresh, and 4 us more in k_rt_half_bands -- the kernel is not at the issue rate)
            const double dtau_gas = dcol * (kap + ray / mu);
            // `plain` (wave-uniform): no clouds, no I2S correction, g0 = 0, no beam -- the cloud term is an exact zero and
            // E (1 - w0 g0) an exact one: the general formulas minus their no-ops, same bits (two_stream.h)
            const double dtau = plain ? dtau_gas : dtau_gas + dcol * (cab + csc) / mu;
            const Slab s = plain ? slab_coeffs_plain(w0, dtau, a.epsi)
                                 : slab_coeffs(w0, dtau, g0, a.epsi, a.epsi2, cp.mu_star, HX_COEF_FLAG(scat_corr), a.i2s, HX_COEF_FLAG(dir_beam) == 1);
            if (HX_COEF_FLAG(diag) != nullptr && HX_COEF_FLAG(dir_beam) == 1) {  // G_limiter's warning (kernels.cu:217-231) as a count
                if (s.nlim) atomicAdd(HX_COEF_FLAG(diag) + HX_DIAG_G_LIMITED, (unsigned long long)s.nlim);
            }
            double invM = 1.0 / s.M;
            alpha = s.P * invM;
            beta = -s.N * invM;
            double K = 2.0 * HX_PI * a.epsi * (1.0 - w0) / (s.E - w0);
            double u, v;
            if (!scatters) {
                // pure absorption (matrix method, see above): down P' = B_b - T B_t + eps (T - 1) (B_b - B_t) / dtau, up the
                // same with the nodes exchanged (kernels.cu:2300-2316, :2376-2411); thin or isothermal: (1 - T) (B_b + B_t) / 2
                alpha = s.trans;
                beta = 0.0;
                invM = 1.0;
                K = 2.0 * HX_PI * a.epsi;
                if (HX_COEF_FLAG(iso) || dtau < a.dtau_limit) {
                    u = v = (1.0 - s.trans) / 2.0;
                } else {
                    const double gq = a.epsi * (s.trans - 1.0) / dtau;
                    u = 1.0 + gq;
                    v = -s.trans - gq;
                }
            } else if (HX_COEF_FLAG(iso) || dtau < a.dtau_limit) {  // isothermal source: B (N + M - P) (kernels.cu:1442, :1640-1643)
                u = v = (s.N + s.M - s.P) / 2.0;
            } else {
                const double qq = (plain ? a.epsi : a.epsi / (s.E * (1.0 - w0 * g0))) * (s.P - s.M + s.N) / dtau;
                u = (s.M + s.N) + qq;
                v = -s.P - qq;
            }
            up = K * u * invM;
            vp = K * v * invM;
            if (HX_COEF_FLAG(dir_beam) == 1 && scatters) {
                // beam at node h (bottom) and h+1 (top) of this half-layer: Fbot, Ftop from above
                const double dn = Fbot / nmu * (s.Gm * s.M + s.Gp * s.N) - Ftop / nmu * s.Gm * s.P;
                const double upw = Ftop / nmu * (s.Gm * s.N + s.Gp * s.M) - Fbot / nmu * s.P * s.Gp;
                dd = dmin(0.0, dn) * invM;
                du = dmin(0.0, upw) * invM;
            }
            if (h == 0) {
                a.boaK[col * nc + c] = scatters ? (1.0 - w0) / (s.E - w0) : 1.0;   // (pure absorption: (1 - A) pi B_surf, :2349)
                a.Fdir0[col * nc + c] = HX_COEF_FLAG(dir_beam) == 1 ? (a.F_dir_wg + col * wgI)[c] : 0.0;
            }
        }
        const size_t off = plane_off(r, lane, ROWS);
        // written once per refresh, streamed by k_rt_flux afterwards: past the L2
        if constexpr (sizeof(CT) == sizeof(double)) {
            __builtin_nontemporal_store(alpha, ctile + 0 * ROWS * 64 + off);
            __builtin_nontemporal_store(beta, ctile + 1 * ROWS * 64 + off);
            __builtin_nontemporal_store(up, ctile + 2 * ROWS * 64 + off);
            if (HX_COEF_FLAG(has_vp)) __builtin_nontemporal_store(vp, ctile + (size_t)a.pl_vp * ROWS * 64 + off);
        } else {   // fp32: see plane_code.h (the rows without a half-layer: alpha = 1, beta = 0, rest -0.0)
            __builtin_nontemporal_store(plane0_code(alpha, beta), ctile + 0 * ROWS * 64 + off);
            __builtin_nontemporal_store(plane1_code(beta), ctile + 1 * ROWS * 64 + off);
            __builtin_nontemporal_store((CT)up, ctile + 2 * ROWS * 64 + off);
            if (HX_COEF_FLAG(has_vp)) __builtin_nontemporal_store((CT)(up + vp), ctile + (size_t)a.pl_vp * ROWS * 64 + off);
        }
        if (HX_COEF_FLAG(dir_beam) == 1) {
            __builtin_nontemporal_store((CT)dd, ctile + (size_t)a.pl_dd * ROWS * 64 + off);
            __builtin_nontemporal_store((CT)du, ctile + (size_t)(a.pl_dd + 1) * ROWS * 64 + off);
        }
    }
}
#ifdef HX_COEF_FLAG_DEFAULTS
#undef HX_COEF_FLAG
#undef HX_COEF_FROM_TABLE
#undef HX_COEF_TEMPLATE
#undef HX_COEF_FLAG_DEFAULTS
#endif
