"""tests/golden/sites.npz (scripts/gen_site_golden.py) records the reference's own normalize_data, format_single_frame,
calc_projection_points and calc_fade_square under eight sites' constants.  Here, without a GPU: the C oracle's normalisation and
the `utils` restatements of the output step meet the recording bit for bit under each site, make_sites builds the values a
config built from the same constants holds, and (where the reference exists) a fresh run of the generator writes the same
arrays.  The device path replays the recording in tests/test_gpu_sites_golden.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sites.npz")
N_SITES = 8


def site_kw(row):
    """A recorded site row -> keyword arguments of _lib.default_config / _lib.make_sites."""
    keys = ("s_height", "s_tilt", "intensity_mu", "intensity_std", "m_x", "m_y", "m_z", "v_screen_fade_size_max", "v_screen_fade_size_min",
            "v_screen_fade_weight")
    return {k: float(v) for k, v in zip(keys, row)}


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def format_single_frame_np(frames, mean, std_dev, ring=3):
    """Utils.format_single_frame (Utils.py:468-520) restated: per frame the columns (x, y, z, doppler, intensity), the intensity
    normalised as (I - mean) / std_dev, cut / zero-padded to 64 rows, sorted by x (ties by row position, as the device sorts),
    -> (ring, 8, 8, 5) float64.  Pinned to the recording below; the device's feature maps are held against it in
    tests/test_gpu_sites_golden.py."""
    out = np.zeros((ring, 64, 5))
    for k, fr in enumerate(frames):
        rows = np.asarray(fr, np.float64).reshape(-1, 8)[:, [0, 1, 2, 6, 7]].copy()
        rows[:, 4] = (rows[:, 4] - mean) / std_dev
        pad = np.zeros((64, 5))
        m = min(64, len(rows))
        pad[:m] = rows[:m]
        out[k] = pad[np.argsort(pad[:, 0], kind="stable")]
    return out.reshape(ring, 8, 8, 5)


def test_feature_restatement_meets_the_recording_under_every_sites_intensity_scale():
    from tests._golden import assert_feat_equal
    g = np.load(GOLD)
    scales = set()
    for i in range(N_SITES):
        kw = site_kw(g["sites"][i])
        scales.add((kw["intensity_mu"], kw["intensity_std"]))
        cloud, cn = g[f"cloud_{i}"], g[f"cloud_n_{i}"]
        got = format_single_frame_np([cloud[k, : cn[k]] for k in range(3)], kw["intensity_mu"], kw["intensity_std"])
        want = g[f"feat_{i}"]
        assert want.shape == (3, 8, 8, 5) and np.abs(want[..., 4]).max() > 0
        # (the reference's argsort is not stable: rows with equal x may swap -- tests/_golden.py's comparison knows that; the
        #  values themselves are compared as float64 first, then as the float32 the device stores)
        assert_feat_equal(got.astype(np.float32), want.astype(np.float32), ctx=f"site {i}")
        assert np.array_equal(np.sort(got.reshape(3, 64, 5)[..., 4], axis=1), np.sort(want.reshape(3, 64, 5)[..., 4], axis=1)), i
    assert len(scales) >= 2


def test_recording_covers_the_sites_and_the_edges():
    g = np.load(GOLD)
    sites = g["sites"]
    assert sites.shape == (N_SITES, 11) and len({tuple(r[:2]) for r in sites}) >= 7
    assert np.array_equal(sites[7, :2], sites[0, :2]) and not np.array_equal(sites[7, 2:], sites[0, 2:])
    for i in range(N_SITES):
        raw, norm = g[f"raw_{i}"], g[f"norm_{i}"]
        assert 0 < len(norm) < len(raw) and 0 < len(g[f"norm32_{i}"]) < len(g[f"raw32_{i}"])   # keeps a row, drops a row
        assert np.isnan(raw[:, :3]).any() and np.isposinf(raw[:, :3]).any() and np.isneginf(raw[:, :3]).any()
        assert np.isnan(raw[:, 3]).any() and np.isinf(raw[:, 3]).any()
        assert (np.all(raw[:, :3] == 0, axis=1)).any()                       # r == 0
        assert (norm[:, 2] == 2.5).any(), i                                  # a row exactly on the upper edge is kept
        # the rows on the lower edges are DROPPED, so they show in the raw rows only: by the arithmetic normalize_rows shares with
        # the oracle (which the next test holds against this recording bit for bit) some raw row lands exactly on z' == 0 and
        # one on y' == 0, and the latter has a neighbour one step inside
        a = np.radians(sites[i, 1])
        c, s, h = np.cos(a), np.sin(a), sites[i, 0]
        with np.errstate(all="ignore"):
            yp, zp = c * raw[:, 1] + (-s) * raw[:, 2], (s * raw[:, 1] + c * raw[:, 2]) + h
        assert ((zp == 0.0) & (yp > 0)).any() and ((zp == 2.5) & (yp > 0)).any(), i
        assert ((yp == 0.0) & (np.abs(raw[:, :3]).sum(axis=1) > 0)).any(), i
        assert ((yp > 0) & (yp < 1e-300)).any(), i
        assert np.isnan(norm[:, 3:6]).any()                                  # a non-finite doppler on a kept row
        assert g[f"raw32_{i}"].astype(np.float32).astype(np.float64).tobytes() == g[f"raw32_{i}"].tobytes()


def test_c_oracle_normalize_meets_the_recording_under_every_site():
    from oracle import c_oracle as co
    g = np.load(GOLD)
    for i in range(N_SITES):
        kw = site_kw(g["sites"][i])
        cfg = co.default_config(s_height=kw["s_height"], s_tilt=kw["s_tilt"])
        for raw, want in ((g[f"raw_{i}"], g[f"norm_{i}"]), (g[f"raw32_{i}"], g[f"norm32_{i}"])):
            got = co.normalize(cfg, raw)
            assert same_bits(got, want), (i, got.shape, want.shape)


def test_utils_output_step_meets_the_recording_under_every_site(monkeypatch):
    """utils.calc_projection_points / fade_squares read the constants module: with a site's M_* / V_SCREEN_FADE_* they give
    the reference's values -- the restatement tests/test_gpu_sites_golden.py holds the track table against."""
    from mmwave_msc_amd import constants as const
    from mmwave_msc_amd import utils
    g = np.load(GOLD)
    for i in range(N_SITES):
        kw = site_kw(g["sites"][i])
        for name, key in (("M_X", "m_x"), ("M_Y", "m_y"), ("M_Z", "m_z"), ("V_SCREEN_FADE_SIZE_MAX", "v_screen_fade_size_max"),
                          ("V_SCREEN_FADE_SIZE_MIN", "v_screen_fade_size_min"), ("V_SCREEN_FADE_WEIGHT", "v_screen_fade_weight")):
            monkeypatch.setattr(const, name, kw[key])
        pp = g[f"proj_in_{i}"]
        got = np.array([utils.calc_projection_points(*p) for p in pp])
        assert same_bits(got, g[f"proj_out_{i}"]), i
        px, pz, size = utils.fade_squares(g[f"fade_x_{i}"], g[f"fade_kp_{i}"])
        assert same_bits(np.stack([px, pz, size], axis=1), g[f"fade_out_{i}"]), i


def test_make_sites_builds_what_a_config_of_the_same_constants_holds():
    from mmwave_msc_amd import _lib
    g = np.load(GOLD)
    kws = [site_kw(r) for r in g["sites"]]
    cols = {k: [kw[k] for kw in kws] for k in kws[0]}
    sites = _lib.make_sites(_lib.default_config(), N_SITES, **cols)
    assert sites.dtype == _lib.SITE_DTYPE and sites.itemsize == 96 and np.all(sites["reserved_"] == 0)
    for i, kw in enumerate(kws):
        cfg = _lib.default_config(**kw)
        for f in _lib.SITE_FIELDS:
            assert sites[f][i] == getattr(cfg, f), (i, f)
    one = _lib.make_sites(_lib.default_config(s_height=2.0), 3, s_tilt=-20.0)
    assert np.all(one["s_height"] == 2.0) and np.all(one["tilt_cos"] == float(np.cos(np.radians(-20.0))))
    with pytest.raises(AttributeError):
        _lib.make_sites(_lib.default_config(), 2, tr_gate=1.0)
    with pytest.raises(ValueError):
        _lib.make_sites(_lib.default_config(), 2, s_height=[1.0, 2.0, 3.0])


@pytest.mark.reference
def test_recording_is_what_the_generator_writes(tmp_path):
    out = str(tmp_path / "sites.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_site_golden.py"), out], check=True, capture_output=True, timeout=600)
    a, b = np.load(out), np.load(GOLD)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
