// The body of k_rt_flux (fp64 coefficient planes) and of k_rt_flux_f32 (fp32, `precision = single`): one source, included
// twice by rt_kernels.h with HX_FLUX_HEAD (the function it is the body of), HX_PLANE_T (the planes' element type CT) and
// HX_PLANES set.  k_rt_flux is this function itself -- compiled as the body of an inlined device function its code changed
// and config 2's step took 2 % longer --; for k_rt_flux_f32 it is such a device function, with which the tilings of 12-14
// rows hold their registers (as the body of the kernel itself they spilled 2-7 VGPRs).
template <int ROWS, int K = 0, bool MATRIX = false>
HX_FLUX_HEAD {
    using CT = HX_PLANE_T;
    extern __shared__ __align__(16) double smem[];
    const int col = a.reverse ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y;
    if (a.done[col]) return;
    const int bx = a.reverse ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;
    // the workgroups this launch dispatches last leave their up-flux state in the Infinity Cache for the next launch
    const bool keep_state_cached = (int)(blockIdx.y * gridDim.x + blockIdx.x) >= a.cache_state_from;
    const int NN = a.H + 3, I = a.I;
    double* sB = smem;                               // [nxb][NN]  Planck function at the nodes
    double* acc = sB + (size_t)a.nxb * NN;           // [nxb][2][I] band fluxes being accumulated
    double* stage = acc + (size_t)a.nxb * 2 * I;     // [ypb][nxb][2][I]
    const hx_rt_column cp = a.colpar[col];
    const size_t nc = (size_t)a.Y * a.X;
    const int k = K ? K : a.k;

    for (int t = threadIdx.x; t < a.nxb * NN; t += blockDim.x) {
        const int xl = t / NN, n = t - xl * NN, x = bx * a.nxb + xl;
        sB[t] = x < a.X ? a.Bn[((size_t)col * a.X + x) * NN + n] : 0.0;
    }
    for (int t = threadIdx.x; t < a.nxb * 2 * I; t += blockDim.x) acc[t] = 0.0;
    __syncthreads();

    for (int part = 0; part < a.nparts; part++) {
        const LaneMap m = lane_map(a, bx, part, opaque_tid());
        // coefficient planes and up-flux state -> registers.  The tiles are streamed once per launch: non-temporal
        // loads AND stores together keep them from displacing the node and band arrays the neighbouring kernels and
        // the next workgroups find in the L2 (same-box A/B: k_rt_flux 400 -> 386 us, k_rt_nodes 16 -> 14.4,
        // k_rt_totals_a 16 -> 12.7; either hint alone changes nothing)
        const size_t toff = m.tile * (size_t)ROWS * 64 + m.lane;
        const CT* ctile = HX_PLANES + col * a.coef_col + m.tile * (size_t)a.nplane * ROWS * 64 + m.lane;   // (elements of CT)
        double* utile = a.Utile + col * a.flux_col + toff;
        double al[ROWS], be[ROWS], sd[ROWS], su[ROWS], Uo[ROWS], Do[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            al[r] = __builtin_nontemporal_load(ctile + (0 * ROWS + r) * 64);
            be[r] = __builtin_nontemporal_load(ctile + (1 * ROWS + r) * 64);
            sd[r] = __builtin_nontemporal_load(ctile + (2 * ROWS + r) * 64);  // u' for now
            if (!MATRIX) Uo[r] = __builtin_nontemporal_load(utile + r * 64);
        }
        if constexpr (sizeof(CT) == sizeof(double)) {
            if (a.has_vp) {
#pragma unroll
                for (int r = 0; r < ROWS; r++) su[r] = __builtin_nontemporal_load(ctile + (a.pl_vp * ROWS + r) * 64);  // v' for now
            } else {
#pragma unroll
                for (int r = 0; r < ROWS; r++) su[r] = a.Kconst * ((1.0 - al[r]) - be[r]) - sd[r];
            }
        } else {   // fp32 planes (plane_code.h): al, be hold the codes until they are decoded here
            if (a.has_vp) {
#pragma unroll
                for (int r = 0; r < ROWS; r++) su[r] = __builtin_nontemporal_load(ctile + (a.pl_vp * ROWS + r) * 64);  // u' + v' for now
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const double rest = plane_decode(al[r], be[r]);
                su[r] = (a.has_vp ? su[r] : a.Kconst * rest) - sd[r];
            }
        }
        double U0 = 0.0, boaK = 0.0, Fdir0 = 0.0, albedo = 0.0;
        if (m.valid && m.j == 0) {
            if (!MATRIX) U0 = a.U0[col * nc + m.sp];
            boaK = a.boaK[col * nc + m.sp];
            Fdir0 = a.Fdir0[col * nc + m.sp];
            albedo = a.surf_albedo[(size_t)col * a.X + m.x];
        }
        // the quadrature weight is requested here, with the tiles: asked for after the sweeps it was a dependent load
        // into a saturated memory system, several microseconds per tile with nothing to hide behind
        const double w = m.valid ? 0.5 * a.gauss_w[m.y] : 0.0;
        const double* Bx = sB + (size_t)(m.valid ? m.xl : 0) * NN;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const int h = min(m.j * ROWS + r, a.H - 1);
            const double Bb = Bx[h], Bt = a.iso ? Bb : Bx[h + 1], upc = sd[r], vpc = su[r];
            sd[r] = upc * Bb + vpc * Bt;
            su[r] = upc * Bt + vpc * Bb;
        }
        if (a.dir_beam == 1) {
            // The rows of the two beam planes are requested in groups that are in flight together, and only then added: left
            // to the scheduler, the loads came out as ONE register pair loaded and added once per row -- 14 (7 rows) or 26
            // (13 rows) dependent memory round trips per tile; k_rt_flux<7, 64> took 3.70 instead of 3.40 ms per launch at
            // config 5 (whether it happened depended on unrelated code: round 3's build had the 14 in flight together).
            // Up to 8 rows per lane all at once; 13 rows in groups of BEAM_GROUP (the register file is full there).
            constexpr int BEAM_GROUP = ROWS <= 8 ? ROWS : HX_BEAM_GROUP;
#pragma unroll
            for (int r0 = 0; r0 < ROWS; r0 += BEAM_GROUP) {
                double bd[BEAM_GROUP], bu[BEAM_GROUP];
#pragma unroll
                for (int u = 0; u < BEAM_GROUP; u++)
                    if (r0 + u < ROWS) {
                        bd[u] = __builtin_nontemporal_load(ctile + (a.pl_dd * ROWS + r0 + u) * 64);
                        bu[u] = __builtin_nontemporal_load(ctile + ((a.pl_dd + 1) * ROWS + r0 + u) * 64);
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < BEAM_GROUP; u++)
                    if (r0 + u < ROWS) {
                        sd[r0 + u] += bd[u];
                        su[r0 + u] += bu[u];
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const double rs = cp.R_star / cp.a;
        const double D_toa = (1.0 - a.dir_beam) * cp.f_factor * (rs * rs) * HX_PI * Bx[a.H + 1];
        const double B_surf = Bx[a.H + 2];

        // rows (r even, r odd) of this lane whose up-flux the reference makes positive when it is tiny: the odd nodes
        const bool odd0 = (m.j * ROWS) & 1;
        const double thr_even = (a.iso || odd0) ? 1e-100 : 0.0, thr_odd = (a.iso || !odd0) ? 1e-100 : 0.0;
        if constexpr (MATRIX) {
            // which values the reference makes positive: with scattering (Thomas, non-isothermal) every x < 1e-100 of the back-
            // substitution becomes |x| (kernels.cu:2268), with isothermal layers none (:1967); in the pure-absorption sweeps tiny
            // values do (:2329, :2351, :2418, and -- isothermal -- :1990, :2018), the up-flux at the layer centres excepted (:2394)
            const bool scatters = m.valid ? a.trigger[col * nc + m.sp] != 0 : false;
            const bool flip_negative = scatters && !a.iso;
            const double tiny_d = scatters ? 0.0 : 1e-100;
            const double tiny_u_even = scatters ? 0.0 : ((a.iso || odd0) ? 1e-100 : 0.0), tiny_u_odd = scatters ? 0.0 : ((a.iso || !odd0) ? 1e-100 : 0.0);
            auto patch = [&](double v, double tiny) { return flip_negative ? (v < 1e-100 ? fabs(v) : v) : tiny_abs_below(v, tiny); };
            // ---------------- rho: surface -> TOA ----------------
            // The Moebius map of a half-layer, rho -> alpha^2 rho / (1 - beta rho) + beta, is composed in the variable
            // e = 1 - rho: [[alpha^2 + beta (1 - beta), (1 - beta - alpha) (1 - beta + alpha)], [beta, 1 - beta]].  Its entries are
            // formed without cancellation and are not negative (alpha + beta <= 1), so neither the products nor the final
            // quotient cancel: e comes out to a few ulps.  In rho itself ([[alpha^2 - beta^2, beta], [-beta, 1]]) a deep stack
            // of nearly conservative scatterers -- the two fixed points 5e-5 apart -- lost nine digits of rho in the product:
            // 5.5e-5 of the fluxes at 200 half-layers of w0 = 1 - 1e-10, dtau = 700 (tests/test_gpu_coef_edges.py).
            // (the tiles' padding rows and lanes hold alpha = 1, beta = 0: the identity)
            Moebius P = {1.0, 0.0, 0.0, 1.0};
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const double omb = 1.0 - be[r];
                const double m11 = fma(al[r], al[r], be[r] * omb), m12 = (omb - al[r]) * (omb + al[r]);
                const double n11 = fma(m11, P.p11, m12 * P.p21), n12 = fma(m11, P.p12, m12 * P.p22);
                P.p21 = fma(be[r], P.p11, omb * P.p21);
                P.p22 = fma(be[r], P.p12, omb * P.p22);
                P.p11 = n11;
                P.p12 = n12;
            }
            {   // entries near one before the lanes are combined: a stack of thick, nearly conservative scatterers shrinks the
                // product by 4e-5 per row, and only the ratios matter
                const double sc = 1.0 / fmax(fmax(fabs(P.p11), fabs(P.p12)), fmax(fabs(P.p21), fabs(P.p22)));
                P.p11 *= sc; P.p12 *= sc; P.p21 *= sc; P.p22 *= sc;
            }
            moebius_scan_up<K>(P, m.j, k);
            double e11 = K ? below_fixed<K>(P.p11) : from_lane_below<1>(P.p11, k), e12 = K ? below_fixed<K>(P.p12) : from_lane_below<1>(P.p12, k);
            double e21 = K ? below_fixed<K>(P.p21) : from_lane_below<1>(P.p21, k), e22 = K ? below_fixed<K>(P.p22) : from_lane_below<1>(P.p22, k);
            const double alb = K ? group_first_lane<K>(albedo, m.lane) : __shfl(albedo, 0, k);
            double rho = 1.0 - fma(e11, 1.0 - alb, e12) / fma(e21, 1.0 - alb, e22);   // at this lane's lowest node
            if (m.j == 0) rho = alb;
            // per row: a = alpha / (1 - beta rho_b) -- the factor of BOTH affine recurrences --, the constant of the sigma
            // recurrence s_up + a rho_b s_down, what the D recurrence needs: beta / (1 - beta rho_b), s_down / (1 - beta rho_b),
            // and rho at the row's top node (kept where the sweeps keep their up-flux)
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const double inv = HX_MATRIX_RCP(1.0 - be[r] * rho), aa = al[r] * inv;
                su[r] = fma(aa * rho, sd[r], su[r]);
                rho = fma(aa * al[r], rho, be[r]);
                Uo[r] = rho;
                be[r] *= inv;
                sd[r] *= inv;
                al[r] = aa;
            }
            // ---------------- sigma: surface -> TOA ----------------
            double sigma0 = 0.0;
            if (m.j == 0) sigma0 = albedo * Fdir0 + (1.0 - albedo) * HX_PI * boaK * B_surf;
            sigma0 = K ? group_first_lane<K>(sigma0, m.lane) : __shfl(sigma0, 0, k);
            {
                double A = 1.0, Bc = 0.0;
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    Bc = fma(al[r], Bc, su[r]);
                    A *= al[r];
                }
                if (K) {
                    scan_up_fixed<K>(A, Bc, m.j);
                } else if (k == 32) {
                    scan32_up(A, Bc, m.j);
                } else {
                    scan_step_up<1>(A, Bc, m.j, k);
                    scan_step_up<2>(A, Bc, m.j, k);
                    scan_step_up<4>(A, Bc, m.j, k);
                    scan_step_up<8>(A, Bc, m.j, k);
                    scan_step_up<16>(A, Bc, m.j, k);
                    scan_step_up<32>(A, Bc, m.j, k);
                }
                double sg = K ? below_fixed<K>(fma(A, sigma0, Bc)) : from_lane_below<1>(fma(A, sigma0, Bc), k);
                if (m.j == 0) sg = sigma0;
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    sd[r] = fma(be[r], sg, sd[r]);      // constant of the D recurrence: (beta sigma_bottom + s_down) / (1 - beta rho_b)
                    sg = fma(al[r], sg, su[r]);
                    su[r] = sg;                         // sigma at the row's top node
                }
            }
            // ---------------- D: TOA -> surface, and U = rho D + sigma ----------------
            {
                double A = 1.0, Bc = 0.0;
#pragma unroll
                for (int r = ROWS - 1; r >= 0; r--) {
                    Bc = fma(al[r], Bc, sd[r]);
                    A *= al[r];
                }
                if (K) {
                    scan_down_fixed<K>(A, Bc, m.j, m.lane);
                } else if (k == 32) {
                    scan32_down(A, Bc, m.j, m.lane);
                } else {
                    scan_step_down<1>(A, Bc, m.j, k);
                    scan_step_down<2>(A, Bc, m.j, k);
                    scan_step_down<4>(A, Bc, m.j, k);
                    scan_step_down<8>(A, Bc, m.j, k);
                    scan_step_down<16>(A, Bc, m.j, k);
                    scan_step_down<32>(A, Bc, m.j, k);
                }
                double D = K ? above_fixed<K>(fma(A, D_toa, Bc)) : from_lane_above<1>(fma(A, D_toa, Bc), k);
                if (m.j == k - 1) D = D_toa;
#pragma unroll
                for (int r = ROWS - 1; r >= 0; r--) {
                    Uo[r] = patch(fma(Uo[r], D, su[r]), (r & 1) ? tiny_u_odd : tiny_u_even);   // U at the top node, D there still in hand
                    D = patch(fma(al[r], D, sd[r]), tiny_d);
                    Do[r] = D;
                }
            }
            if (m.j == 0) U0 = patch(fma(albedo, Do[0], sigma0), 0.0);
        } else
        for (int sweep = 0; sweep < a.nsweep; sweep++) {
            // ---------------- down: TOA -> BOA ----------------
            {
                double Ubelow = K ? below_fixed<K>(Uo[ROWS - 1]) : from_lane_below<1>(Uo[ROWS - 1], k);  // U at the bottom node of this chunk
                if (m.j == 0) Ubelow = U0;
                double A = 1.0, Bc = 0.0;
#pragma unroll
                for (int r = ROWS - 1; r >= 0; r--) {
                    const double Uh = r > 0 ? Uo[r - 1] : Ubelow;
                    const double t = fma(be[r], Uh, sd[r]);
                    Bc = fma(al[r], Bc, t);
                    A *= al[r];
                }
                // inclusive suffix composition over the k lanes of this spectral point
                if (K) {
                    scan_down_fixed<K>(A, Bc, m.j, m.lane);
                } else if (k == 32) {
                    scan32_down(A, Bc, m.j, m.lane);
                } else {
                    scan_step_down<1>(A, Bc, m.j, k);
                    scan_step_down<2>(A, Bc, m.j, k);
                    scan_step_down<4>(A, Bc, m.j, k);
                    scan_step_down<8>(A, Bc, m.j, k);
                    scan_step_down<16>(A, Bc, m.j, k);
                    scan_step_down<32>(A, Bc, m.j, k);
                }
                double Din = K ? above_fixed<K>(fma(A, D_toa, Bc)) : from_lane_above<1>(fma(A, D_toa, Bc), k);
                if (m.j == k - 1) Din = D_toa;
                double D = Din;
#pragma unroll
                for (int r = ROWS - 1; r >= 0; r--) {
                    const double Uh = r > 0 ? Uo[r - 1] : Ubelow;
                    D = tiny_abs(fma(al[r], D, fma(be[r], Uh, sd[r])));
                    Do[r] = D;
                }
            }
            // ---------------- BOA boundary ----------------
            if (m.j == 0) U0 = albedo * (Fdir0 + Do[0]) + (1.0 - albedo) * HX_PI * boaK * B_surf;
            const double Ubc = K ? group_first_lane<K>(U0, m.lane) : __shfl(U0, 0, k);
            // ---------------- up: BOA -> TOA ----------------
            {
                double Dabove = K ? above_fixed<K>(Do[0]) : from_lane_above<1>(Do[0], k);  // D at the top node of this chunk
                if (m.j == k - 1) Dabove = D_toa;
                double A = 1.0, Bc = 0.0;
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    const double Dh = r < ROWS - 1 ? Do[r + 1] : Dabove;
                    const double t = fma(be[r], Dh, su[r]);
                    Bc = fma(al[r], Bc, t);
                    A *= al[r];
                }
                if (K) {
                    scan_up_fixed<K>(A, Bc, m.j);
                } else if (k == 32) {
                    scan32_up(A, Bc, m.j);
                } else {
                    scan_step_up<1>(A, Bc, m.j, k);
                    scan_step_up<2>(A, Bc, m.j, k);
                    scan_step_up<4>(A, Bc, m.j, k);
                    scan_step_up<8>(A, Bc, m.j, k);
                    scan_step_up<16>(A, Bc, m.j, k);
                    scan_step_up<32>(A, Bc, m.j, k);
                }
                double Uin = K ? below_fixed<K>(fma(A, Ubc, Bc)) : from_lane_below<1>(fma(A, Ubc, Bc), k);
                if (m.j == 0) Uin = Ubc;
                double U = Uin;
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    const double Dh = r < ROWS - 1 ? Do[r + 1] : Dabove;
                    U = fma(al[r], U, fma(be[r], Dh, su[r]));
                    // interface nodes only (reference quirk, kernels.cu:1763; isothermal layers: every node, :1509)
                    if (K) U = tiny_abs_below(U, (r & 1) ? thr_odd : thr_even);
                    else if (a.iso || ((m.j * ROWS + r) & 1)) U = tiny_abs(U);
                    Uo[r] = U;
                }
            }
        }

        // Gauss quadrature of the interface fluxes: stage[yl][xl][dir][i], summed over yl in order.
        // The lane map is derived afresh (e for "epilogue"): carried across the sweeps it lived in scratch
        const LaneMap e = lane_map(a, bx, part, opaque_tid());
#ifdef HX_PROFILING  // HELIOS_RT_DEBUG_SKIP: bit 0 no quadrature, bit 1 no state stores -- not in the shipped library
        const int debug_skip = a.debug_skip;
#else
        constexpr int debug_skip = 0;
#endif
        auto store_state = [&]() {
            const size_t eoff = e.tile * (size_t)ROWS * 64 + e.lane;
            if (!(debug_skip & 2) && (!MATRIX || a.keep_up)) {   // (a direct solve has no state: its spectral fluxes are
                double* ut = a.Utile + col * a.flux_col + eoff;   //  written where somebody asks for them, hx_rt_get)
#pragma unroll
                for (int r = 0; r < ROWS; r++) {
                    // (write-through store that leaves the line in the Infinity Cache: agent scope = `sc1`; see launch_flux)
                    if (keep_state_cached) __hip_atomic_store(ut + r * 64, Uo[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else __builtin_nontemporal_store(Uo[r], ut + r * 64);
                }
            }
            if (a.keep_down) {
                double* dtile = a.Dtile + col * a.flux_col + eoff;
#pragma unroll
                for (int r = 0; r < ROWS; r++) __builtin_nontemporal_store(Do[r], dtile + r * 64);
            }
            if (e.valid && e.j == 0) a.U0[col * nc + e.sp] = U0;
        };
        if (!(debug_skip & 1)) {
            if (e.valid) {
                // Row r of this lane is node h = h0 + r.  Staggered grid: an even node gives D at interface h/2, an odd
                // one U at interface (h+1)/2 -- with the lane's parity p folded into two base pointers the rows use
                // compile-time offsets (26 separately computed LDS addresses did not fit the register file: they were
                // reloaded from scratch, one memory round trip per row and tile)
                const int h0 = e.j * ROWS, nrow = a.H - h0;
                double* st = stage + ((size_t)e.yl * a.nxb + e.xl) * 2 * I;
                if (a.iso) {                                            // every node is an interface
                    double *pd = st + h0, *pu = st + I + h0 + 1;
#pragma unroll
                    for (int r = 0; r < ROWS; r++)
                        if (r < nrow) {
                            pd[r] = w * Do[r];
                            pu[r] = w * Uo[r];
                        }
                } else {
                    const bool p = h0 & 1;
                    const int q = (h0 + (p ? 1 : 0)) >> 1;
                    double* pe = st + q + (p ? I : 0);                  // rows 0, 2, ...: D (p = 0) or U (p = 1)
                    double* po = st + q + (p ? -1 : I);                 // rows 1, 3, ...: U (p = 0) or D (p = 1)
#pragma unroll
                    for (int r = 0; r < ROWS; r++)
                        if (r < nrow) {
                            if ((r & 1) == 0) pe[r >> 1] = w * (p ? Uo[r] : Do[r]);
                            else po[(r + 1) >> 1] = w * (p ? Do[r] : Uo[r]);
                        }
                }
                if (e.j == 0) st[I + 0] = w * U0;
                if (h0 <= a.H - 1 && a.H - 1 < h0 + ROWS) st[a.L] = w * D_toa;
            }
            __syncthreads();
            for (int t = threadIdx.x; t < a.nxb * 2 * I; t += blockDim.x) {
                const int xl = t / (2 * I), rest = t - xl * 2 * I;
                double s = acc[t];
                for (int yl = 0; yl < a.ypb; yl++) s += stage[((size_t)yl * a.nxb + xl) * 2 * I + rest];
                acc[t] = s;
            }
            __syncthreads();
        }
        store_state();
    }
    // band fluxes of this workgroup's bins, internal layout [x][i]
    for (int t = threadIdx.x; t < a.nxb * 2 * I; t += blockDim.x) {
        const int xl = t / (2 * I), rest = t - xl * 2 * I, x = bx * a.nxb + xl;
        if (x >= a.X) continue;
        const int dir = rest / I, i = rest - dir * I;
        (dir == 0 ? a.F_down_band_n : a.F_up_band_n)[((size_t)col * a.X + x) * I + i] = acc[t];
    }
}
