#!/usr/bin/env python3
"""Makes the line-by-line opacity files of a species from a HITRAN line list, on the device (helios_amd/lines.py).

    python lines.py -name H2O -line_list h2o.par -partition_function q1.txt -temperatures "300 900 1500" \
        -pressure_codes "n300 p000" -numin 0 -numax 30000 -dnu 0.01 -output_directory opac/H2O/

The directory receives one file `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` per (chunk, temperature, pressure code): fp32
opacities in cm^2 g^-1 at numin + i dnu, which `ktable.py` reads as it reads HELIOS-K's.  `-chunk_width W` splits the range into
files of W cm^-1, `-output_format text` writes `.dat` files of two columns, `-isotopologue`, `-molar_mass`, `-self_fraction` and
`-cutoff` (25 cm^-1) set what their names say, `-backend numpy` computes the same on the CPU.  The pipeline is
lines.py -> ktable.py -> helios.py.
"""
import sys

from helios_amd import lines


def main(argv=None):
    return lines.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
