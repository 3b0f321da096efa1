"""Cloud sweeps, the host side: the host's Cloud path against the long-double restatement of a deck's spectra, the new sweep
keys, the deck description next to cloud_pre_processing, the Mie cache and the HELIOS_CLOUD_DECKS switch."""
import numpy as np
import pytest

import cloud_reference as cr


@pytest.fixture(scope="module")
def edge_mie(tmp_path_factory):
    lam_um, scat, absorb, g = cr.synthetic_mie(cr.NW_EDGE, seed=5)
    path = cr.write_mie_directory(str(tmp_path_factory.mktemp("mie") / "aerosol"), lam_um, scat, absorb, g)
    return path, cr.table_of(lam_um, scat, absorb)


def test_the_edge_grids_contain_every_case_of_the_contract(edge_mie):
    lam = edge_mie[1]["lamda_mie"]
    feats = [cr.grid_features(lam, cr.bin_grid(lam, n)) for n in (1, 63, 65, 257)]
    for key in ("below", "above", "empty", "ten", "on_point", "ends_on_last", "on_first"):
        assert any(f[key] for f in feats), key


@pytest.mark.parametrize("nbin", [1, 63, 65, 257])
def test_host_cloud_path_is_held_to_the_long_double_restatement(edge_mie, nbin):
    """absorption, scattering and the third spectrum of one deck by Cloud.calc_weighted_cross_sections_... against the
    restatement within max(1e-13, 8 eps_plain); zeros exact"""
    cr.require_extended_precision()
    path, table = edge_mie
    # what the reader makes of the files is the table the restatement is given
    from helios_amd.clouds import Cloud
    read = Cloud.mie_table(path)
    for n in ("lamda_mie", "scat", "absorb"):
        np.testing.assert_array_equal(read[n], table[n])
    inter = cr.bin_grid(table["lamda_mie"], nbin)
    w = cr.radius_weight(2.0, 1.8)
    ref = cr.reference_spectra(table, w, inter)
    plain = cr.plain_spectra(table, w, inter)
    host = cr.host_spectra(cr.host_cloud([path], [2.0], [1.8]), 0, cr.Quant(inter))
    assert np.any(ref[1] == 0) or nbin == 1
    assert np.any(ref > 0)
    cr.hold(host, ref, plain, "host path, nbin = %d" % nbin)


def test_expand_sweep_takes_the_cloud_keys_and_still_refuses_the_layers():
    from helios_amd.sweep import CLOUD_OPTIONS, PER_COLUMN_OPTIONS, expand_sweep
    for key in ("path_to_mie_files", "aerosol_radius_mode", "aerosol_radius_geometric_std_dev", "cloud_bottom_pressure",
                "cloud_bottom_mixing_ratio", "cloud_to_gas_scale_height_ratio", "path_to_file_with_cloud_data", "aerosol_name"):
        assert key in PER_COLUMN_OPTIONS and key in CLOUD_OPTIONS
        assert expand_sweep(key + "=a,b") == [{key: "a"}, {key: "b"}]
    cols = expand_sweep("aerosol_radius_mode=1 5,10 5;cloud_bottom_pressure=1e5 1e3")
    assert cols == [{"aerosol_radius_mode": "1 5", "cloud_bottom_pressure": "1e5 1e3"},
                    {"aerosol_radius_mode": "10 5", "cloud_bottom_pressure": "1e5 1e3"}]
    with pytest.raises(ValueError):
        expand_sweep("number_of_layers=10,20")
    with pytest.raises(ValueError):
        expand_sweep("number_of_cloud_decks=1,2")


def test_space_separated_decks_reach_the_reader_from_the_command_line():
    from helios_amd import quantities, read
    reader, keeper = read.Read(), quantities.Store()
    reader.read_param_file_and_command_line(keeper, reader.cloud, [
        "-parameter_file", "/nonexistent", "-number_of_cloud_decks", "2", "-aerosol_radius_mode", "1 5",
        "-aerosol_radius_geometric_std_dev", "2", "-cloud_bottom_pressure", "1e5 1e3", "-path_to_mie_files", "a/ b/"])
    assert list(reader.cloud.cloud_r_mode) == [1.0, 5.0] and list(reader.cloud.p_cloud_bot) == [1e5, 1e3]
    assert list(reader.cloud.cloud_r_std_dev) == [2.0] and reader.cloud.mie_path == ["a/", "b/"]


def _cloud_file(path, press, names, rng):
    with open(path, "w") as f:
        f.write("cloud data\n")
        f.write("Pressure " + " ".join(names) + "\n")
        for p in press:
            f.write("%.9e " % p + " ".join("%.9e" % v for v in 10.0 ** rng.uniform(-14, -9, len(names))) + "\n")


@pytest.mark.parametrize("setting,iso", [("manual", 0), ("manual", 1), ("file", 0), ("file", 1)])
def test_deck_description_reproduces_profiles_and_weights_bit_for_bit(edge_mie, tmp_path, setting, iso):
    """radius weights, f_lay / f_int per deck and the total mixing ratio of the description path against lognorm_pdf,
    create_cloud_deck and cloud_pre_processing"""
    from helios_amd.clouds import DELTA_R, R_VALUES, Cloud
    path, table = edge_mie
    quant = cr.Quant(cr.bin_grid(table["lamda_mie"], 63), nlayer=11, iso=iso, p_boa=1e7, p_toa=10.0)

    def cloud():
        c = cr.host_cloud([path, path], [1.5, 7.0], [1.6, 2.2], p_bot=(3e5, 2e3), f_bot=(1e-11, 4e-13), ratio=(0.5, 0.25))
        if setting == "file":
            c.cloud_mixing_ratio_setting = "file"
            c.cloud_vmr_file = str(tmp_path / "clouds.txt")
            c.cloud_vmr_file_header_lines, c.cloud_file_press_name, c.cloud_file_press_units = 1, "Pressure", "cgs"
            c.cloud_file_species_name = ["Aerosol2", "Aerosol1"]
        return c
    if setting == "file":      # a profile shorter than the column at both ends
        _cloud_file(str(tmp_path / "clouds.txt"), np.geomspace(2e6, 50.0, 9), ["Aerosol1", "Aerosol2"], np.random.default_rng(2))
    want, desc_cloud = cloud(), cloud()
    decks = desc_cloud.cloud_deck_description(quant)
    total_lay, total_int = quant.f_all_clouds_lay.copy(), quant.f_all_clouds_int.copy()
    assert decks is quant.cloud_decks and decks["radius_weight"].shape == (2, len(R_VALUES))
    for d in range(2):
        want.create_cloud_deck(d, quant)
        np.testing.assert_array_equal(decks["f_lay"][d], want.f_one_cloud_lay)
        np.testing.assert_array_equal(decks["f_int"][d], want.f_one_cloud_int)
        np.testing.assert_array_equal(decks["radius_weight"][d],
                                      Cloud.lognorm_pdf(R_VALUES, want.cloud_r_mode[d], want.cloud_r_std_dev[d]) * DELTA_R)
        assert np.any(decks["f_lay"][d] > 0) and (iso == 1 or np.any(decks["f_int"][d] > 0))
    assert not np.array_equal(decks["f_lay"][0], decks["f_lay"][1])
    want.cloud_pre_processing(quant)
    np.testing.assert_array_equal(total_lay, quant.f_all_clouds_lay)
    np.testing.assert_array_equal(total_int, quant.f_all_clouds_int)


def test_a_mie_directory_is_read_once_for_several_columns(edge_mie, monkeypatch):
    from helios_amd.clouds import R_VALUES, Cloud
    path, table = edge_mie
    calls = []
    read_one = Cloud.read_mie_file
    monkeypatch.setattr(Cloud, "read_mie_file", staticmethod(lambda f: calls.append(f) or read_one(f)))
    cache = {}
    descs = []
    for r_mode in (1.0, 3.0, 9.0):        # three columns of two decks, all on one directory (once with a different spelling)
        quant = cr.Quant(cr.bin_grid(table["lamda_mie"], 63), nlayer=5)
        c = cr.host_cloud([path, path.rstrip("/") + "/./"], [r_mode, 2 * r_mode], [2.0, 2.0], p_bot=(1e4, 1e3),
                          f_bot=(1e-12, 1e-12), ratio=(0.5, 0.5))
        descs.append(c.cloud_deck_description(quant, cache))
    assert len(calls) == len(R_VALUES) and len(cache) == 1
    assert all(t is descs[0]["tables"][0] for d in descs for t in d["tables"])
    Cloud.mie_table(path)                  # without a cache every call reads
    assert len(calls) == 2 * len(R_VALUES)


def test_helios_cloud_decks_switch(monkeypatch):
    from helios_amd.sweep import cloud_deck_mode, expand_sweep
    cloudy, plain = expand_sweep("aerosol_radius_mode=1,2;f_factor=0.25,0.5"), expand_sweep("f_factor=0.25,0.5")
    monkeypatch.delenv("HELIOS_CLOUD_DECKS", raising=False)
    assert cloud_deck_mode(cloudy) == "device" and cloud_deck_mode(plain) == "host"
    for mode in ("host", "device"):
        monkeypatch.setenv("HELIOS_CLOUD_DECKS", mode)
        assert cloud_deck_mode(cloudy) == mode and cloud_deck_mode(plain) == mode
    monkeypatch.setenv("HELIOS_CLOUD_DECKS", "bogus")
    with pytest.raises(ValueError, match="HELIOS_CLOUD_DECKS=bogus"):
        cloud_deck_mode(cloudy)
    from helios_amd import sweep as sw
    with pytest.raises(ValueError, match="HELIOS_CLOUD_DECKS=bogus"):
        sw.run_sweep(["-parameter_file", "/nonexistent"], cloudy)
