"""Published coefficient sets behind the analytic tables of helios_amd/continuum.py: Rayleigh scattering of H2, He, H, CO2,
CO, O2, N2 and e-, the H- continuum (John 1988, A&A 193, 189) and the He- free-free table (John 1994, MNRAS 269, 871).

Numbers only.  Wavelengths are in cm for the Rayleigh fits (wavenumbers in cm^-1) and in micron for the continuum, as the
papers give them.  The values are those the reference's k-table tool uses, including where it departs from a paper (see the
README, "Continuum and Rayleigh tables").
"""

# ---- Rayleigh: n - 1 as a fit in nu^2 = lambda^-2 [cm^-2], the reference number density n_ref [cm^-3], the King factor ------
# forms of n - 1:  "cauchy"     scale * (1 + b * nu^2)
#                  "sellmeier"  scale * (a + b / (c - nu^2))                       (one resonance)
#                  "sum"        scale * sum_k b_k / (c_k - nu^2)                   (CO2, five resonances)
# King factor:     k0 + k1 * nu + k2 * nu^2 + k4 * nu^4
RAYLEIGH = {
    "H2": {"form": "cauchy", "scale": 13.58e-5, "b": 7.52e-11, "n_ref": 2.65163e19, "king": (1.0, 0.0, 0.0, 0.0)},
    "He": {"form": "sellmeier", "scale": 1e-8, "a": 2283.0, "b": 1.8102e13, "c": 1.5342e10, "n_ref": 2.546899e19,
           "king": (1.0, 0.0, 0.0, 0.0)},
    "CO": {"form": "sellmeier", "scale": 1e-8, "a": 22851.0, "b": 0.456e14, "c": 71427.0 ** 2, "n_ref": 2.546899e19,
           "king": (1.0, 0.0, 0.0, 0.0)},
    "O2": {"form": "sellmeier", "scale": 1e-8, "a": 20564.8, "b": 2.480899e13, "c": 4.09e9, "n_ref": 2.68678e19,
           "king": (1.09, 0.0, 1.385e-11, 1.448e-20)},
    # N2 changes its fit at nu = 21 360 cm^-1: "red" at and below, "blue" above
    "N2": {"form": "sellmeier", "scale": 1e-8, "a": 6498.2, "b": 307.4335e12, "c": 14.4e9, "n_ref": 2.546899e19,
           "king": (1.034, 3.17e-12, 0.0, 0.0), "split_nu": 21360.0, "a_blue": 5677.465, "b_blue": 318.81874e12},
    "CO2": {"form": "sum", "scale": 1.1427e3, "b": (5799.25, 120.05, 5.3334, 4.3244, 0.1218145e-6),
            "c": (128908.9 ** 2, 89223.8 ** 2, 75037.5 ** 2, 67837.7 ** 2, 2418.136 ** 2), "n_ref": 2.546899e19,
            "king": (1.1364, 0.0, 25.3e-12, 0.0)},
}

# atomic hydrogen (Lee & Kim 2004): sigma_T' (lambda_L / lambda)^4 sum_k c_k (lambda_L / lambda)^(2k), with the rounded Thomson
# cross-section and Lyman limit the reference uses there
H_SERIES = (1.26563, 3.73828125, 8.813930935, 19.15379502, 39.92303232, 81.10881152, 161.9089166, 319.0231631, 622.2679809,
            1203.891509)
H_SERIES_SIGMA_T = 0.665e-24          # cm^2
H_SERIES_LYMAN = 91.2e-7              # cm

RAYLEIGH_SPECIES = ("H2", "He", "H", "CO2", "CO", "O2", "N2", "e-")

# ---- H- bound-free (John 1988, eq. 4-5): sigma = 1e-18 lambda^3 x^1.5 sum_k C_k x^(k/2), x = 1/lambda - 1/lambda_0 -----------
HM_BF_LAMBDA_MIN = 0.125              # micron; below: 0
HM_BF_LAMBDA_0 = 1.6419               # micron; above: 0
HM_BF_C = (152.519, 49.534, -118.858, 92.536, -34.194, 4.982)

# ---- H- free-free (John 1988, eq. 6, tables 3a and 3b) ------------------------------------------------------------------------
# k = 1e-29 sum_n theta^((n+1)/2) (A_n lambda^2 + B_n + C_n / lambda + D_n / lambda^2 + E_n / lambda^3 + F_n / lambda^4), n = 1 .. 6
HM_FF_LAMBDA_MIN = 0.1823             # micron; below: 0
HM_FF_LAMBDA_SPLIT = 0.3645           # micron; "short" below, "long" at and above
HM_FF = {
    "short": {"A": (518.1021, 473.2636, -482.2089, 115.5291, 0.0, 0.0),
              "B": (-734.8666, 1443.4137, -737.1616, 169.6374, 0.0, 0.0),
              "C": (1021.1775, -1977.3395, 1096.8827, -245.6490, 0.0, 0.0),
              "D": (-479.0721, 922.3575, -521.1341, 114.2430, 0.0, 0.0),
              "E": (93.1373, -178.9275, 101.7963, -21.9972, 0.0, 0.0),
              "F": (-6.4285, 12.3600, -7.0571, 1.5097, 0.0, 0.0)},
    "long": {"A": (0.0, 2483.3460, -3449.8890, 2200.0400, -696.2710, 88.2830),
             "B": (0.0, 285.8270, -1158.3820, 2427.7190, -1841.4000, 444.5170),
             "C": (0.0, -2054.2910, 8746.5230, -13651.1050, 8624.9700, -1863.8640),
             "D": (0.0, 2827.7760, -11485.6320, 16755.5240, -10051.5300, 2095.2880),
             "E": (0.0, -1341.5370, 5303.6090, -7510.4940, 4400.0670, -901.7880),
             "F": (0.0, 208.9520, -812.9390, 1132.7380, -655.0200, 132.9850)},
}
THETA_K = 5040.0                      # theta = 5040 K / T

# ---- He- free-free (John 1994, table 2), in 1e-26 cm^4 dyne^-1 ------------------------------------------------------------------
HEM_UNIT = 1e-26
HEM_LAMBDA = (0.5063, 0.5695, 0.6509, 0.7594, 0.9113, 1.1391, 1.5188, 1.8225, 2.2782, 3.0376, 3.6451, 4.5564, 6.0751, 9.1127,
              11.3909, 15.1878)       # micron
# rows in descending theta, which is ascending temperature
HEM_THETA = (3.6, 2.8, 2.0, 1.8, 1.6, 1.4, 1.2, 1.0, 0.8, 0.6, 0.5)
HEM_K = (
    (0.121, 0.145, 0.178, 0.227, 0.305, 0.444, 0.737, 1.030, 1.574, 2.765, 3.979, 6.234, 11.147, 25.268, 39.598, 70.580),
    (0.100, 0.120, 0.148, 0.190, 0.258, 0.380, 0.643, 0.910, 1.405, 2.490, 3.592, 5.632, 10.059, 22.747, 35.606, 63.395),
    (0.078, 0.094, 0.117, 0.152, 0.210, 0.316, 0.547, 0.782, 1.218, 2.167, 3.126, 4.897, 8.728, 19.685, 30.782, 54.757),
    (0.072, 0.087, 0.109, 0.143, 0.198, 0.300, 0.522, 0.747, 1.165, 2.073, 2.990, 4.681, 8.338, 18.795, 29.384, 52.262),
    (0.066, 0.081, 0.102, 0.133, 0.186, 0.283, 0.495, 0.710, 1.108, 1.971, 2.842, 4.448, 7.918, 17.838, 27.882, 49.583),
    (0.061, 0.074, 0.094, 0.124, 0.173, 0.266, 0.466, 0.670, 1.045, 1.860, 2.681, 4.193, 7.460, 16.798, 26.252, 46.678),
    (0.055, 0.067, 0.086, 0.114, 0.160, 0.247, 0.435, 0.625, 0.977, 1.737, 2.502, 3.910, 6.955, 15.653, 24.461, 43.488),
    (0.049, 0.061, 0.077, 0.103, 0.147, 0.227, 0.400, 0.576, 0.899, 1.597, 2.299, 3.593, 6.387, 14.372, 22.456, 39.921),
    (0.043, 0.053, 0.069, 0.092, 0.131, 0.204, 0.360, 0.518, 0.808, 1.435, 2.065, 3.226, 5.733, 12.897, 20.151, 35.882),
    (0.036, 0.045, 0.059, 0.079, 0.113, 0.176, 0.311, 0.447, 0.698, 1.239, 1.783, 2.784, 4.947, 11.128, 17.386, 30.907),
    (0.033, 0.041, 0.053, 0.072, 0.102, 0.159, 0.282, 0.405, 0.632, 1.121, 1.614, 2.520, 4.479, 10.074, 15.739, 27.979),
)
# the long-wavelength extension: k = HEM_LONG[row] lambda^2 at these wavelengths
HEM_LAMBDA_LONG = (30.0, 50.0, 80.0, 120.0, 160.0, 200.0)
HEM_LONG = (0.307, 0.275, 0.238, 0.227, 0.215, 0.202, 0.189, 0.173, 0.155, 0.134, 0.121)
# a row at theta = 100.8 (50 K) below the table, holding the values of the table's coldest row
HEM_THETA_FLOOR = 100.8
HEM_FILL_LOG10 = -30.0                # log10 k outside the table in T or lambda
