#!/usr/bin/env python3
"""Builds per-species k-tables from HELIOS-K output on the device (helios_amd/ktable.py).

    python ktable.py -path_to_individual_species_file species_dirs.dat -wavelength_grid "50 0.34 200" \\
        -number_of_gaussian_points 20 -directory_with_individual_files opac/
    python ktable.py ... -grid_format file -path_to_grid_file interfaces.dat -helios_k_output_format text -interpolate no

The species file has a header line, then `name directory` per species; a directory holds HELIOS-K's
`Out_[<name>_]<numin>_<numax>_<T>_<pcode>.bin` (or `.dat`) files, the first chunk starting at 0 cm^-1.  Written per species:
`<name>_opac_kdistr.h5` on the files' own (T, P) nodes and, unless `-interpolate no`, `<name>_opac_ip_kdistr.h5` on the
reference's final grid (or -temperature_grid / -pressure_grid) -- the container helios.py's on-the-fly mixing and premix.py
read.  `-backend numpy` computes the same on the CPU; `-container npz` writes .npz.  Only the k-distribution format is built.

    python ktable.py -continuum_species "H-,He-" -rayleigh_species "H2,He" -grid_like opac/H2O_opac_ip_kdistr.h5 \\
        -directory_with_individual_files opac/

writes the analytic tables next to them: `H-_bf`, `H-_ff` and `He-` containers and `scat_cross_sections.h5`, on the grid of
the container named (without -grid_like: on the grid the options above define).
"""
import sys

from helios_amd import ktable


def main(argv=None):
    return ktable.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
