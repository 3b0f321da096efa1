#!/usr/bin/env python3
"""Makes the Mie directory of an aerosol from its optical constants, on the device (helios_amd/mie.py).

    python mie.py -refractive_index_file nk.dat -output_directory miedir/
    python mie.py -refractive_index_file nk.dat -header_lines 2 -wavelength_grid "200 0.3 200" -output_directory miedir/

The file holds the columns wavelength [micron], n, k (m = n + i k, k >= 0); `#` lines and the first -header_lines lines are
skipped.  The directory receives the 51 files `r{radius:.6f}.dat` of the radius grid 10^-2 ... 10^3 micron that
`helios.py -path_to_mie_files miedir/` reads.  `-wavelength_grid "nw lo hi"` asks for nw wavelengths evenly spaced in log lambda
instead of the file's own; a wavelength outside the file is refused.  The tool prints the wavelength range it covers: opacity
bins with an interface outside it get no cloud opacity.  `-backend numpy` computes the same on the CPU.
"""
import sys

from helios_amd import mie


def main(argv=None):
    return mie.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
