#!/usr/bin/env python3
"""Makes the collision-induced absorption of a pair from a HITRAN CIA file, on the device (helios_amd/cia.py).

    python cia.py -name CIA_H2H2 -cia_file H2-H2_2011.cia -temperatures "300 900 1500" -pressure_codes "n300 p000" \
        -numax 30000 -dnu 0.1 -output_directory opac/CIA_H2H2/
    python cia.py -name CIA_H2H2 -cia_file H2-H2_2011.cia -temperatures "300 900 1500" -pressure_codes "n300 p000" \
        -numax 30000 -dnu 0.1 -ktable yes -wavelength_grid "50 0.34 200" -directory_with_individual_files tables/

The first form writes one file `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` per (chunk, temperature, pressure code): fp32
opacities in cm^2 per gram of the second partner at numin + i dnu, which `ktable.py` reads as it reads HELIOS-K's.  The second
writes `<name>_opac_kdistr` and `<name>_opac_ip_kdistr` without the files; its grid options are ktable.py's.  `-chunk_width W`
splits the range into files of W cm^-1, `-output_format text` writes `.dat` files of two columns, `-partner_mass` and `-bands`
set the molar mass the opacity is per gram of and the bands of the file to take, `-backend numpy` computes the same on the CPU.
The pipeline is cia.py -> ktable.py -> helios.py.
"""
import sys

from helios_amd import cia


def main(argv=None):
    return cia.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
