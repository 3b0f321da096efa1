"""The super-line contract of helios_amd/exomol.py, restated one transition, one cell and one point at a time: `long_double(...)`
in np.longdouble (the checker of both backends) and `plain_fp64(...)`, the same statements in fp64 (the yardstick of what fp64 can
hold).  S, the four numbers of a transition, K and its regions are tests/exomol_reference.py's and tests/lines_reference.py's.

Per node, S and gamma as in exomol_reference, S_sl the threshold and d the cell width:
    dropped iff S < S_min;  strong iff S >= S_min and S >= S_sl;  weak otherwise
    c = floor(nu_0 / d): one fp64 division, an integer -- a DECISION, so it is taken on the fp64 values in both restatements,
        as the cut-off and K's region are.  The classes are decided by each restatement on its own S; the cases keep every S a
        relative 1e-9 away from S_min and S_sl and every nu_0 / d that far from a whole number (`assert_clear`), so the classes and
        the cells are one set on every backend.
    a cell with at least one weak transition yields one super-line:
        S_c = sum S_j, G_c = sum S_j * gamma_j over its weak transitions in list order, both from 0
        gamma_c = G_c / S_c if S_c > 0 else 0;  nu_c = (c + 0.5) * d
        alpha = (nu_c / C) * sqrt(2 * ln 2 * N_A * K_B * T / M),  a = sqrt(ln 2) / alpha,  y = max(a * gamma_c, 1e-8),
        s = S_c * a * (1 / sqrt pi)
    the list: strong transitions and super-lines by the key (cell, kind, position), the super-line (kind 0, position: the cell's
        first transition) before the cell's strong transitions (kind 1); the sum over it is exomol_reference.sum_over.
"""
import numpy as np

import exomol_reference as er
import lines_reference as lr

CLEAR = 1e-9


def cells_of(nu0, step):
    """floor(nu_0 / d) per transition, on the fp64 values"""
    return np.floor(np.asarray(nu0, np.float64) / np.float64(step)).astype(np.int64)


def gamma_of(jx, broadening, temp, press, T):
    """gamma of one transition with the lower-state index jx, in T"""
    x, table = broadening
    total = T(0.0)
    for b in range(len(x)):
        total = total + T(x[b]) * T(table[b, jx, 0]) * (T(lr.T_REF) / T(temp)) ** T(table[b, jx, 1])
    return (T(press) / T(er.BAR)) * total


def superline_numbers(s_c, g_c, cell, step, temp, molar_mass, T):
    """(nu_c, s, a, y) of one super-line from its sums, in T"""
    ln2, inv_sqrt_pi = lr.constants(T)
    gamma_c = g_c / s_c if s_c > 0 else T(0.0)
    nu_c = (T(cell) + T(0.5)) * T(step)
    alpha = (nu_c / T(lr.C)) * np.sqrt(T(2.0) * ln2 * T(lr.N_A) * T(lr.K_B) * T(temp) / T(molar_mass))
    a = np.sqrt(ln2) / alpha
    y = max(a * gamma_c, T(lr.Y_MIN))
    return nu_c, s_c * a * inv_sqrt_pi, a, y


def node_list(states, trans, broadening, temp, press, q_t, molar_mass, s_min, s_sl, step, T):
    """{"params": [4][entries] in T; "keys": [entries][cell, kind, position]; "kept", "strong", "weak": indices in the list;
    "cells", "S_c", "G_c": per super-line; "S": per transition}"""
    s_all = er.strengths(states, trans, temp, q_t, T)
    nu0 = trans["nu0"]
    n = len(nu0)
    cell = cells_of(nu0, step)
    keep = s_all >= T(s_min)
    is_strong = keep & (s_all >= T(s_sl))
    is_weak = keep & ~is_strong
    columns, keys, cells, sums_s, sums_g = [], [], [], [], []
    j = 0
    while j < n:
        end = j
        while end < n and cell[end] == cell[j]:
            end += 1
        s_c, g_c, any_weak = T(0.0), T(0.0), False
        for i in range(j, end):
            if is_weak[i]:
                jx = int(states["jidx"][int(trans["low"][i])])
                s_c = s_c + s_all[i]
                g_c = g_c + s_all[i] * gamma_of(jx, broadening, temp, press, T)
                any_weak = True
        if any_weak:
            columns.append(superline_numbers(s_c, g_c, int(cell[j]), step, temp, molar_mass, T))
            keys.append((int(cell[j]), 0, j))
            cells.append(int(cell[j])); sums_s.append(s_c); sums_g.append(g_c)
        for i in range(j, end):
            if is_strong[i]:
                jx = int(states["jidx"][int(trans["low"][i])])
                columns.append(er.transition_numbers(s_all[i], nu0[i], jx, broadening, temp, press, molar_mass, T))
                keys.append((int(cell[j]), 1, i))
        j = end
    params = np.empty((4, len(columns)), T)
    for k, col in enumerate(columns):
        params[:, k] = col
    return {"params": params, "keys": np.array(keys, np.int64).reshape(-1, 3), "kept": np.nonzero(keep)[0],
            "strong": np.nonzero(is_strong)[0], "weak": np.nonzero(is_weak)[0], "cells": np.array(cells, np.int64),
            "S_c": np.array(sums_s, T), "G_c": np.array(sums_g, T), "S": s_all}


def opacity(states, trans, broadening, temp, press, q_t, molar_mass, s_min, s_sl, step, cutoff, nu_first, dnu, n_points, T, points=None):
    """(kappa in T, the node's list in T): the fp64 list decides the cut-off and the regions, the list in T computes"""
    l64 = node_list(states, trans, broadening, temp, press, q_t, molar_mass, s_min, s_sl, step, np.float64)
    lt = l64 if T is np.float64 else node_list(states, trans, broadening, temp, press, q_t, molar_mass, s_min, s_sl, step, T)
    assert np.array_equal(lt["keys"], l64["keys"]), "the cases keep S clear of S_min and S_sl: one list"
    return er.sum_over(l64["params"], lt["params"], cutoff, nu_first, dnu, n_points, molar_mass, T, points), lt


def long_double(*args, **kw):
    return opacity(*args, T=np.longdouble, **kw)


def plain_fp64(*args, **kw):
    return opacity(*args, T=np.float64, **kw)


def assert_clear(states, trans, nodes, q, s_min, s_sl, step, on_purpose=()):
    """no long-double S within a relative 1e-9 of S_min or S_sl at any node (T, P) of `nodes`; no nu_0 / d within 1e-9 of a whole
    number, unless nu_0 is listed in `on_purpose` and the hit is exact"""
    for temp in sorted(set(n[0] for n in nodes)):
        s = er.strengths(states, trans, temp, q(temp), np.longdouble)
        for name, level in (("S_min", s_min), ("S_sl", s_sl)):
            if level > 0 and np.isfinite(level):
                gap = np.abs(s / np.longdouble(level) - 1)
                assert gap.min() > CLEAR, (name, temp, float(gap.min()))
    ratio = trans["nu0"].astype(np.longdouble) / np.longdouble(step)
    off = np.abs(ratio - np.rint(ratio))
    for j in np.nonzero(off <= CLEAR)[0]:
        assert off[j] == 0 and float(trans["nu0"][j]) in on_purpose, (j, float(trans["nu0"][j]), float(off[j]))
