"""What the REFERENCE's analytic chemistry computes (tests/golden/chem/reference.npz).

    python tests/golden/make_chem_golden.py /path/to/reference

The reference's script `supplementary/reproducing_Fig4_of_Malik2017/TEA_compendium/chem_analytical.py` plots on import, so its
function definitions are taken out of it with `ast` and run here.  Stored, as data only: the temperatures and dG values its
functions interpolate in (26 rows), its gas constant, and its five abundances for the 200 cases of its figure -- 800 K and
3000 K at 1 bar, n_O = 5e-4, 100 values of C/O from 0.1 to 10 -- with the largest imaginary part of the roots it picked.
Nothing of the reference's text.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "chem", "reference.npz")
SCRIPT = "supplementary/reproducing_Fig4_of_Malik2017/TEA_compendium/chem_analytical.py"


def main(reference):
    tree = ast.parse(open(os.path.join(reference, SCRIPT)).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    space = {"np": np}
    for name in ("mean", "arange", "zeros", "polynomial", "array", "interp", "exp"):
        space[name] = getattr(np, name)
    exec(compile(ast.Module(body=defs, type_ignores=[]), "<reference functions>", "exec"), space)

    def local(function, name):
        """the value a function assigns to one of its local names"""
        for n in ast.walk([d for d in defs if d.name == function][0]):
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id == name:
                return eval(compile(ast.Expression(n.value), "<reference value>", "eval"), space)
        raise KeyError((function, name))

    temps = np.asarray(local("kprime", "temperatures"), np.float64)
    for f in ("kprime2", "kprime3"):
        assert np.array_equal(temps, np.asarray(local(f, "temperatures"), np.float64))
    runiv = [float(local(f, "runiv")) for f in ("kprime", "kprime2", "kprime3")]
    assert len(set(runiv)) == 1
    out = {"gibbs_temperatures": temps, "gas_constant": np.float64(runiv[0]),
           "gibbs_dg1": np.asarray(local("kprime", "dg"), np.float64),
           "gibbs_dg2": np.asarray(local("kprime2", "dg2"), np.float64),
           "gibbs_dg3": np.asarray(local("kprime3", "dg3"), np.float64)}
    n_o, pbar = 5e-4, 1.0
    n_c = np.logspace(-1., 1., 100) * n_o
    case_t = np.array([800.0, 3000.0])
    names = (("n_CH4", "n_methane"), ("n_H2O", "n_water"), ("n_CO", "n_cmono"), ("n_CO2", "n_cdio"), ("n_C2H2", "n_acet"))
    imag = 0.0
    for key, fn in names:
        vals = np.zeros((len(case_t), len(n_c)))
        for it, t in enumerate(case_t):
            for ic, c in enumerate(n_c):
                v = space[fn](n_o, c, t, pbar)
                imag = max(imag, abs(complex(v).imag))
                vals[it, ic] = complex(v).real
        out[key] = vals
    out.update(case_temperatures=case_t, case_pressure_bar=np.float64(pbar), case_n_o=np.float64(n_o), case_n_c=n_c,
               largest_imaginary_part=np.float64(imag))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez(OUT, **out)
    print("wrote %s: %d Gibbs rows, R = %r, %d cases, largest imaginary part of a picked root %.3e"
          % (OUT, len(temps), runiv[0], vals.size, imag))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
