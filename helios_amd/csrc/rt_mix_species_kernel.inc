// The species-loop kernel of rt_species.h, included once per random-overlap mixer:
//   RT_MIX_KERNEL, RT_MIX_ATTR   the kernel's name and its occupancy attribute
//   RT_MIX_INIT(sh, lane, a)     sets the mixer's LDS image up; what it returns is handed to every RT_MIX call
//   RT_MIX(sh, ln, lane, mix, add, cnt)   one random-overlap problem
__global__ void __launch_bounds__(64) RT_MIX_ATTR RT_MIX_KERNEL(MixArgs a) {
    __shared__ ro::Shared sh;
    // what the species loop needs per absorber, staged once per wavefront: table base, correlated-k flag, and -- per
    // level -- the factor vmr * mass / mu.  (Read straight from the argument block these were chains of dependent
    // global loads inside the loop: the scalar registers are all taken, so the compiler fetched them through the
    // vector memory path and waited for each; same-box A/B 68.6 -> 67.7 ms per refresh at config 3.)
    __shared__ const double* s_tab[MIX_MAX_ABSORBERS];
    __shared__ double s_fac[MIX_MAX_ABSORBERS];
    __shared__ int s_info[MIX_MAX_ABSORBERS];  // species index << 1 | random-overlap flag
    // the level's bilinear weights (pup - p, p - pdown, tup - t, t - tdown): wave-uniform fp64 values that the compiler
    // otherwise carries in ten VGPRs through the species loop and, at the 128-register cap, parks in scratch around it --
    // 16 bytes per lane and point written and read back (2.1 GB of the 2.5 GB WRITE_SIZE of round 2's launch)
    __shared__ double s_blend[4];
    const int lane = threadIdx.x;
    const auto ln = RT_MIX_INIT(sh, lane, a);   // what the mixer keeps per lane (ro::mix), the number of Gauss points (ro::mix_ny)
    const int nabs = a.nabs;
    if (lane < nabs) {
        const int s = a.abs_list[lane];
        s_tab[lane] = a.sp[s].pretab;
        s_info[lane] = s << 1 | ((s == 0 || a.sp[s].ro == 0) ? 0 : 1);  // correlated-k: first species, CIA (:3302-3310)
    }
    ro::Counters cnt;
    const long long nlev = a.L + a.I, per_col = nlev * a.X, npair = per_col * a.C;
    const long long chunk = (npair + gridDim.x - 1) / gridDim.x;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = min(npair, p0 + chunk);
    const size_t nc = (size_t)a.Y * a.X, st_p = nc, st_t = nc * a.npress;
    long long lev_cur = -1;
    int tcase = 0;  // bit 0: two pressure nodes, bit 1: two temperature nodes (the four cases of :617-644)
    TPIndex tp = {};
    double* out_level = nullptr;
    size_t pl_dd = 0, pl_ud = 0, pl_du = 0, pl_uu = 0;  // table planes of the level's four (T, P) corners: wave-uniform
    bool skip = false;
    // Three groups of 20 lanes fetch three absorbers at a time: lane 20 g + y holds Gauss point y of absorber kb + g.
    // The next triple's table corners are requested before the present triple is mixed, so that even a run of negligible
    // absorbers (a few dozen instructions each) does not wait for memory.
    const int grp = lane / ro::NY, y = lane - grp * ro::NY;
    const bool loader = grp < 3 && y < a.Y;
    // (bin, level, column) of the run's first point by division, then counted up: no 64-bit division per point
    long long cl = p0 < p1 ? p0 / a.X : 0;  // column * nlev + level
    int x = (int)(p0 - cl * a.X) - 1;
    int col = (int)(cl / nlev), lev = (int)(cl - (long long)col * nlev);
    for (long long pair = p0; pair < p1; pair++) {
        if (++x == a.X) {
            x = 0;
            cl++;
            if (++lev == (int)nlev) {
                lev = 0;
                col++;
            }
        }
        if (cl != lev_cur) {  // wave-uniform: a new level (or column)
            lev_cur = cl;
            const bool lay = lev < a.L;
            const int i = lay ? lev : lev - a.L;
            skip = __builtin_amdgcn_readfirstlane(a.done[col]) != 0;
            tp = (lay ? a.tp_lay : a.tp_int)[(size_t)col * a.I + i];
            const double* fac = (lay ? a.fac_lay : a.fac_int) + ((size_t)col * a.I + i) * a.S;
            out_level = (lay ? a.opac_wg_lay : a.opac_wg_int) + (size_t)col * nc * a.I + nc * i;
            // the level's table nodes are the same in every lane: as scalars (the loads above came through the vector path), so
            // that the four plane offsets are scalar arithmetic and live in scalar registers
            const int pdown = __builtin_amdgcn_readfirstlane(tp.pdown), pup = __builtin_amdgcn_readfirstlane(tp.pup);
            const int tdown = __builtin_amdgcn_readfirstlane(tp.tdown), tup = __builtin_amdgcn_readfirstlane(tp.tup);
            pl_dd = st_p * pdown + st_t * tdown;
            pl_ud = st_p * pup + st_t * tdown;
            pl_du = st_p * pdown + st_t * tup;
            pl_uu = st_p * pup + st_t * tup;
            ro::sync();
            int ls = lane;
            asm volatile("" : "+v"(ls));  // addresses derived from the lane id are rebuilt here, once per level, instead of
                                          // occupying a register (at the cap: a scratch slot) through the whole kernel
            if (ls < nabs) s_fac[ls] = fac[s_info[ls] >> 1];
            if (lane == 0) {
                s_blend[0] = tp.pup - tp.p; s_blend[1] = tp.p - tp.pdown;
                s_blend[2] = tp.tup - tp.t; s_blend[3] = tp.t - tp.tdown;
            }
            tcase = (pdown != pup ? 1 : 0) | (tdown != tup ? 2 : 0);
            ro::sync();
        }
        if (skip) continue;
        const unsigned off = (unsigned)(a.Y * x + y);  // inside a table plane: the same for all corners of all species
        double c_dd = 0.0, c_ud = 0.0, c_du = 0.0, c_uu = 0.0;
        int gl = grp;
        asm volatile("" : "+v"(gl));  // the LDS address of this lane's table pointer is rebuilt per point (no register, no scratch slot)
        if (loader && grp < nabs) {
            const double* tab = s_tab[gl];
            c_dd = (tab + pl_dd)[off]; c_ud = (tab + pl_ud)[off]; c_du = (tab + pl_du)[off]; c_uu = (tab + pl_uu)[off];
        }
        double mixv = 0.0;  // nullify_opac_scat_arrays (host_functions.py:1050-1056)
        if (a.carry_on && lane < a.Y) mixv = out_level[off];   // (wave-uniform flag: a species list of more than 48 absorbers)
        for (int kb = 0; kb < nabs; kb += 3) {
            // blend_tp(..., species = true) with the level's weights re-read from LDS (same products in the same order)
            asm volatile("" ::: "memory");  // the weights are not to be carried in registers across the mixes
            double raw_mine = c_dd;
            if (tcase == 3)
                raw_mine = c_dd * s_blend[0] * s_blend[2] + c_ud * s_blend[1] * s_blend[2] + c_du * s_blend[0] * s_blend[3] +
                           c_uu * s_blend[1] * s_blend[3];
            else if (tcase == 1) raw_mine = c_dd * s_blend[0] + c_ud * s_blend[1];
            else if (tcase == 2) raw_mine = c_du * s_blend[3] + c_dd * s_blend[2];
            if (loader && kb + 3 + grp < nabs) {
                const double* tab = s_tab[kb + 3 + grp];
                c_dd = (tab + pl_dd)[off]; c_ud = (tab + pl_ud)[off]; c_du = (tab + pl_du)[off]; c_uu = (tab + pl_uu)[off];
            }
            for (int j = 0; j < 3 && kb + j < nabs; j++) {
                const double raw = ro::shfl((ro::NY * j + y) << 2, raw_mine);  // lanes 0..19: from group j
                const double add = s_fac[kb + j] * raw;
                if ((s_info[kb + j] & 1) == 0) mixv += add;
                else mixv = RT_MIX(sh, ln, lane, mixv, add, cnt);
            }
        }
        if (lane < a.Y) out_level[off] = mixv;
    }
    ro::flush(cnt, lane, a.diag);
}
