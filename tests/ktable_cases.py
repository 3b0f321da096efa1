"""The HELIOS-K goldens of tests/golden/ktable (made by tests/golden/make_ktable_golden.py) as directories and grids."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ktable")


def load(case):
    return np.load(os.path.join(GOLDEN, case + ".npz"))


def files_of(g):
    return {str(n): g["data_%d" % i] for i, n in enumerate(g["files"])}


def write_dir(root, g, text=False, scale=None):
    """the case's HELIOS-K files; text: 17 digits, so that the parsed value is the fp32 value"""
    os.makedirs(root, exist_ok=True)
    for name, data in files_of(g).items():
        if scale is not None:
            data = (data * np.float32(scale)).astype(np.float32)
        if text:
            parts = name.split("_")
            numin, numax = int(parts[-4]), int(parts[-3])
            nu = numin + (numax - numin) * np.arange(len(data)) / len(data)
            with open(os.path.join(root, name.replace(".bin", ".dat")), "w") as f:
                for n, k in zip(nu, data):
                    f.write("%.5f %.17e\n" % (n, float(k)))
        else:
            np.asarray(data, np.float32).tofile(os.path.join(root, name))
    return root


def interfaces(g):
    from helios_amd import ktable
    if "wavelength_grid" in g.files:
        return ktable.wavelength_grid("fixed_resolution", g["wavelength_grid"])
    return np.asarray(g["interfaces"], np.float64)


# (case, key suffix of the expected table, Gauss points, text)
CASES = [("a", "", 20, False), ("a", "_ng1", 1, False), ("a", "_ng8", 8, False), ("b", "", 20, False), ("b", "_text", 20, True),
         ("c", "", 20, False)]


def check(g, suffix, got, what, record=None):
    """|log10 k - log10 k_ref| <= max(1e-13, 8 eps_ref) over the whole table and -- stricter -- over the bins the reference
    itself computed in double (make_ktable_golden.py), where eps_ref is its scan's noise alone.  Prints before it asserts."""
    ref = np.asarray(g["kpoints" + suffix], np.float64)
    got = np.asarray(got, np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    dev = np.abs(np.log10(got) - np.log10(ref))
    eps = float(g["eps_ref" + suffix])
    tol = max(1e-13, 8 * eps)
    line = "%s%s: deviation %.3e, eps_ref %.3e, bound %.3e" % (what, suffix, dev.max(), eps, tol)
    rec = {"eps_ref": eps, "deviation": float(dev.max()), "bound": tol}
    if "eps_ref_floored_bins" + suffix in g.files:
        mask = np.asarray(g["floored_bins"], bool)
        eps_fl = float(g["eps_ref_floored_bins" + suffix])
        dev_fl = dev.reshape(len(mask), -1)[mask].max()
        tol_fl = max(1e-13, 8 * eps_fl)
        line += "; bins in double: deviation %.3e, eps_ref %.3e, bound %.3e" % (dev_fl, eps_fl, tol_fl)
        rec.update(eps_ref_double_bins=eps_fl, deviation_double_bins=float(dev_fl), bound_double_bins=tol_fl)
    print(line)
    if record is not None:
        record[what + suffix] = rec
    assert np.all(np.isfinite(dev)) and dev.max() <= tol, line
    if "eps_ref_floored_bins" + suffix in g.files:
        assert dev_fl <= tol_fl, line
    return rec
