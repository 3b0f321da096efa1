#!/usr/bin/env python3
"""Builds a premixed k-table on the device from the on-the-fly species set (helios_amd/premix.py).

    python premix.py -path_to_species_file species.dat -directory_with_opacity_files opac/ \
        -directory_with_fastchem_files chem/ -premix_output solar.h5 [-premix_refine 2,2] [-premix_cell_error yes|no]
    python premix.py ... -premix_output grid.h5 -sweep "directory_with_fastchem_files=solar/,10xsolar/"

The on-the-fly options are helios.py's (species file, opacity directory, FastChem directory, k_coefficients_mixing_method).
With -sweep one table per chemistry is built from species tables uploaded once, written to grid_0.h5, grid_1.h5, ..., and the
list is printed in the form sweep.py's `-sweep "path_to_opacity_file=..."` takes.  Every mixing ratio must be a constant or
FastChem; the species tables' nodes must be uniform in T and log10 P.
"""
import sys

from helios_amd import premix


def main(argv=None):
    return premix.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
