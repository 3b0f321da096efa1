#!/usr/bin/env python3
"""Makes a FastChem output directory from the analytic C-H-O equilibrium chemistry, on the device (helios_amd/chem.py).

    python chem.py -gibbs_file gibbs_cho.dat -temperature_grid "500 3000 50" -pressure_grid "-6 3 28" \
        -output_directory chem/solar/
    python chem.py -gibbs_file gibbs_cho.dat -grid_like tables/H2O_opac_ip_kdistr.h5 -output_directory chem/grid \
        -sweep "c_to_o=0.3,0.55,1.1;metallicity=1,10"

The first form writes `chem/solar/chem.dat`: the mixing ratios of H2, He, H2O, CO, CH4, CO2, C2H2 and the mean molecular mass on
the (T, P) nodes given, pressures in bar.  The second takes the nodes of an opacity container, writes `chem/grid_0/` ...
`chem/grid_5/` (the first key slowest) from one kernel launch and prints the list as `sweep.py -sweep` and `premix.py -sweep`
take it.  `-gibbs_file` holds T [K] and the Gibbs free energies of the three net reactions [J/mol]; a node temperature outside it
is refused.  `-o_to_h`, `-metallicity`, `-c_to_o` and `-he_to_h` set the abundances, `-backend numpy` computes the same on the CPU.
The pipeline is exomol.py -ktable yes -> chem.py -> ktable.py -mixed_table_production or premix.py -> helios.py / sweep.py.
"""
import sys

from helios_amd import chem


def main(argv=None):
    return chem.main(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
