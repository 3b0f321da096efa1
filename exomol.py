#!/usr/bin/env python3
"""Makes the opacities of a species from an ExoMol line list, on the device (helios_amd/exomol.py).

    python exomol.py -name H2O -states 1H2-16O.states -trans "a.trans b.trans" -partition_function 1H2-16O.pf \
        -broadeners "H2:0.85:H2.broad He:0.15:He.broad" -temperatures "1000 1500" -pressure_codes "n300 p000" \
        -numax 30000 -dnu 0.01 -strength_cutoff 1e-30 -output_directory opac/H2O/
    python exomol.py ... -ktable yes -wavelength_grid "50 0.34 200" -directory_with_individual_files tables/

The first form writes one file `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` per (chunk, temperature, pressure code): fp32
opacities in cm^2 g^-1 at numin + i dnu, which `ktable.py` reads as it reads HELIOS-K's.  The second writes `<name>_opac_kdistr`
and `<name>_opac_ip_kdistr` without the files; its grid options are ktable.py's.  `-trans` takes one or more files, concatenated
in the order given; `.bz2` files are read as they are.  `-broadeners` names each broadener's fraction and `.broad` file,
`-default_broadening "gamma n"` what a J'' without a row takes, `-strength_cutoff S_min` leaves out, per node, the transitions
weaker than S_min at the node's temperature.  `-superline_threshold S_sl` merges, per node, the kept transitions weaker than S_sl
into one super-line per cell of `-superline_step d` cm^-1 (default: `-dnu`), so that no strength is thrown away.  `-numin`,
`-chunk_width`, `-output_format`, `-cutoff`, `-molar_mass`, `-backend numpy` and `-nodes_per_launch` work as in lines.py.
The pipeline is exomol.py -> ktable.py -> helios.py.
"""
import sys

from helios_amd import exomol


def main(argv=None):
    return exomol.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
