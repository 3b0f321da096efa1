#!/usr/bin/env python3
"""Makes stellar spectrum files on the opacity grid, on the device (helios_amd/star.py).

    python star.py -data_format phoenix -name gj1214 -temp 3026 -log_g 4.944 -m 0.39 -phoenix_directory phoenix/ \\
        -convert_to r50_kdistr -opac_file_for_lambdagrid opac/H2O_opac_ip_kdistr.h5 -output_file star/star_2022.h5
    python star.py -data_format ascii -name sun -source_file sun_gueymard_2003.txt -w_conversion_factor 1e-7 \\
        -flux_conversion_factor 1e10 -temp 5772 -opac_file_for_lambdagrid ... -output_file ...
    python star.py -star_list stars.dat -phoenix_directory phoenix/ -opac_file_for_lambdagrid ... -output_file ...

`-phoenix_directory` holds WAVE_PHOENIX-ACES-AGSS-COND-2011.fits and the corner files `TTTTT_G.GG_M.M.fits`; a file that is
not there is an error that names it -- nothing is fetched.  `-data_format muscles` and `btsettl` read FITS files with
-source_file and the conversion factors (muscles: -distance_from_Earth in pc and -R_star in solar radii as well).
`-bb_extrapolation automatic` (the default) fits the black body that fills the bins beyond the spectrum, `fixed` takes -BB_temp
or -temp, `none` leaves those bins 0.  A star list has one star per line, `key=value` pairs with the same keys; all its stars
go onto the grid in one call.  The result is the data set `/<convert_to>/<data_format>/<name>` that
`helios.py -stellar_spectral_model file -dataset_in_stellar_spectrum_file ...` reads; an existing file is extended.
`-backend numpy` computes the same on the CPU; an -output_file that does not end in `.h5` is written as `.npz`.
"""
import sys

from helios_amd import star


def main(argv=None):
    return star.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
