"""tests/chem_reference.py, the long-double restatement of chem.py's contract, against mpmath at 60 digits on a handful of nodes
(where mpmath is installed): the root and every result within a few long-double roundings, and water from the oxygen balance
where the reference script's difference form has lost its digits.  No GPU."""
import numpy as np
import pytest

import chem_reference as cr

WEIGHTS = (2.01588, 4.0026, 18.0153, 28.01, 16.04, 44.01, 26.04)
NODES = [(800.0, 1.0, 5e-4, 0.55), (3000.0, 1e-6, 5e-4, 10.0), (500.0, 1e3, 5e-4, 0.55), (500.0, 10.0, 5e-2, 2.0),
         (3000.0, 1e-9, 5e-5, 0.01), (1234.5, 1e-3, 5e-4, 1.0), (1650.0, 1.0, 5e-3, 1.001)]


@pytest.mark.parametrize("temp,press,n_o,c_to_o", NODES)
def test_the_restatement_against_60_digits(temp, press, n_o, c_to_o):
    mp = pytest.importorskip("mpmath")
    table, gas = cr.golden_table(), float(cr.golden()["gas_constant"])
    args = (table, temp, press, n_o, c_to_o * n_o, 0.085, gas, WEIGHTS)
    ld, exact = cr.node(*args), cr.with_mpmath(*args)
    eps = float(np.finfo(np.longdouble).eps)
    for k in cr.ALL:
        hi, lo = np.longdouble(float(exact[k])), np.longdouble(float(exact[k] - mp.mpf(float(exact[k]))))
        dev = float(abs((ld[k] - hi) - lo) / abs(hi))
        print("%s: %.3e" % (k, dev))
        # |dG / (R T)| reaches 64 here: the exponent's rounding alone is 64 eps in K, and the root follows K
        assert dev <= 2000 * eps, (k, dev)


def test_water_as_a_difference_loses_its_digits_in_fp64():
    """3000 K, 1e-6 bar, C/O = 10: `2 K3 x^2 + x + 2 (n_O - n_C)` in fp64 against the oxygen balance in long double"""
    table, gas = cr.golden_table(), float(cr.golden()["gas_constant"])
    n_o, n_c = 5e-4, 10 * 5e-4
    pf = cr.plain_fp64(table, 3000.0, 1e-6, n_o, n_c, 0.085, gas, WEIGHTS)
    ld = cr.node(table, 3000.0, 1e-6, n_o, n_c, 0.085, gas, WEIGHTS)
    with np.errstate(all="ignore"):
        k3 = cr.constants(np.float64, table, 3000.0, 1e-6, gas, np.exp)[2]
    x = pf["n_CH4"]
    difference = 2.0 * k3 * x * x + x + 2.0 * (n_o - n_c)
    want = ld["H2O"] / ld["H2"]
    assert cr.deviation(difference, want) > 1e-7
    assert cr.deviation(pf["H2O"] / pf["H2"], want) < 1e-14
