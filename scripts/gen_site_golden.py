"""Records tests/golden/sites.npz from the reference's own functions under per-site constants (runs only where the reference
sources exist: oracle.ref_import).

    python scripts/gen_site_golden.py [out.npz]

For each of eight sites -- the default one, six mountings (height 0.6 .. 2.9, tilt -35 .. 12.5 and -5.0000001) and one where
only the intensity scale and the window differ -- it stores
  raw_i       raw sensor rows [n, 5] (x, y, z, doppler, peakVal): random rows plus NaN / +-inf coordinates and dopplers, r == 0,
              and rows on the edges of the scene filter for THAT mounting (z' == 2.5, z' == 0, y' == 0) and one step either side
  norm_i      normalize_data(raw_i) with const.S_HEIGHT / const.S_TILT set to the site
  raw32_i / norm32_i   the same for the rows of raw_i that are exactly representable in float32
  cloud_i, cloud_n_i   a track cloud: 3 frames x 64 rows x 8 and their row counts
  feat_i      format_single_frame(cloud, mean, std_dev) for the site's intensity scale
  proj_in_i / proj_out_i   calc_projection_points under the site's M_X, M_Y, M_Z
  fade_x_i, fade_kp_i / fade_out_i   calc_fade_square under the site's M_* and V_SCREEN_FADE_* (Visualizer.py cannot be imported:
              the function is compiled on its own, as oracle/gen_golden.py does)
and `sites` [8, 11]: s_height, s_tilt (degrees), intensity_mu, intensity_std, m_x, m_y, m_z, fade max, min, weight, 0.
Only inputs and recorded outputs are written."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = ("S_HEIGHT", "S_TILT", "INTENSITY_MU", "INTENSITY_STD", "M_X", "M_Y", "M_Z", "V_SCREEN_FADE_SIZE_MAX", "V_SCREEN_FADE_SIZE_MIN",
        "V_SCREEN_FADE_WEIGHT")


def site_table(const):
    d = [float(getattr(const, c)) for c in COLS]
    rows = [list(d)]
    for h, t in ((0.6, 12.5), (1.1, -12.0), (1.5, 3.0), (2.2, -20.0), (2.9, -35.0), (1.8, -5.0000001)):
        rows.append([h, t] + d[2:])
    rows.append(d[:2] + [40.0, 55.5, -0.5, -1.25, 0.9, 0.5, 0.1, 0.02])
    return np.array(rows)


def _normalize(utils, raw):
    det = {"x": list(raw[:, 0]), "y": list(raw[:, 1]), "z": list(raw[:, 2]), "doppler": list(raw[:, 3]), "peakVal": list(raw[:, 4])}
    with np.errstate(all="ignore"):
        return np.asarray(utils.normalize_data(det), dtype=np.float64).reshape(-1, 8)


def raw_rows(rng, h, tilt):
    n = 96
    raw = np.zeros((n, 5))
    raw[:, 0] = rng.uniform(-3, 3, n)
    raw[:, 1] = rng.uniform(-0.5, 7, n)
    raw[:, 2] = rng.uniform(-3.5, 2.5, n)
    raw[:, 3] = rng.normal(0, 0.6, n)
    raw[:, 4] = rng.integers(0, 300, n)
    raw = raw.astype(np.float32).astype(np.float64)
    a = np.radians(tilt)
    c, s = np.cos(a), np.sin(a)
    edge = []
    step = lambda v, k: float(np.nextafter(v, np.inf if k > 0 else -np.inf)) if k else float(v)
    # z' = (s * y + c * z) + h on its edges 2.5 and 0, for a y that keeps y' > 0; y' = c * y - s * z on its edge 0
    # (fl(s * y) + fl(c * z) moves two grid points of the sum per step of z for some y -- and then never lands on the target --,
    #  so several y are tried)
    for target in (2.5, 0.0):
        y = zc = None
        for y_try in (2.0, 1.75, 2.25, 1.5, 2.5, 3.0, 1.25, 2.125, 1.875, 2.75, 3.5, 1.0):
            z0 = (target - h - s * y_try) / c
            cands, up, dn = [z0], z0, z0
            for _ in range(200):
                up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
                cands += [up, dn]
            hit = [z for z in cands if (s * y_try + c * z) + h == target and c * y_try + (-s) * z > 0]
            if hit:
                y, zc = y_try, hit[0]
                break
        assert zc is not None, f"no double lands z' exactly on {target} for h = {h}, tilt = {tilt}"   # (an edge row must BE on the edge)
        for k in (-1, 0, 1):
            edge.append([0.25, y, step(zc, k), 0.1, 50.0])
    for k in (-1, 0, 1):
        edge.append([1.0, step(0.0, k), 0.0, 0.2, 60.0])           # y' == 0 (and r == |x|)
    edge.append([0.0, 0.0, 0.0, 0.7, 10.0])                        # r == 0
    edge.append([0.0, 0.0, float(np.nextafter(0.0, 1.0)), 0.7, 10.0])
    nan, inf = np.nan, np.inf
    for bad in ([nan, 1, 0, 0.1, 5], [1, inf, 0, 0.1, 5], [1, 1, -inf, 0.1, 5], [0.5, 2, -0.2, nan, 5], [0.5, 2, -0.2, inf, 5],
                [0.5, 2, -0.2, -inf, 5], [inf, 2, -0.2, nan, 5]):
        edge.append([float(v) for v in bad])
    return np.vstack([raw[:48], np.array(edge), raw[48:]])


def main(out_path):
    from oracle.gen_golden import _reference_functions
    from oracle.ref_import import load_reference
    const, utils, _ = load_reference()
    saved = {c: getattr(const, c) for c in COLS}
    sites = site_table(const)
    fade = _reference_functions(os.path.join(os.path.dirname(const.__file__), "Visualizer.py"), {"calc_fade_square"},
                                {"const": const, "calc_projection_points": utils.calc_projection_points, "ClusterTrack": object})
    out = {"sites": np.hstack([sites, np.zeros((len(sites), 1))])}
    try:
        for i, row in enumerate(sites):
            rng = np.random.default_rng(4100 + i)
            for c, v in zip(COLS, row):
                setattr(const, c, float(v))
            raw = raw_rows(rng, row[0], row[1])
            norm = _normalize(utils, raw)
            assert 0 < len(norm) < len(raw), (i, len(norm), len(raw))   # every site keeps a row and drops a row
            is32 = np.all((raw.astype(np.float32).astype(np.float64) == raw) | np.isnan(raw), axis=1)
            raw32 = raw[is32]
            norm32 = _normalize(utils, raw32)
            assert 0 < len(norm32) < len(raw32), (i, len(norm32))
            # a track cloud: three frames (oldest first) of up to 64 rows in the 8-column layout, intensities over 0 .. 300
            cloud = np.zeros((3, 64, 8))
            cn = np.array([64, 37, 0] if i % 2 else [51, 64, 12], np.int32)
            frames = []
            for k in range(3):
                fr = np.zeros((cn[k], 8))
                fr[:, 0:2] = rng.normal(0, 0.4, (cn[k], 2))
                fr[:, 2] = rng.uniform(0.05, 1.9, cn[k])
                fr[:, 3:6] = rng.normal(0, 0.3, (cn[k], 3))
                fr[:, 6] = rng.normal(0, 0.5, cn[k])
                fr[:, 7] = rng.integers(0, 300, cn[k])
                if cn[k] > 3:
                    fr[1, 0] = fr[0, 0]   # a tie in the sort key
                cloud[k, : cn[k]] = fr
                frames.append(fr)
            feat = np.asarray(utils.format_single_frame(frames, float(row[2]), float(row[3])))
            pp = rng.uniform(-3, 6, size=(16, 3))
            pp[0, 0], pp[1, 2] = row[4], row[6]
            pp[2] = [row[4], 2.0, row[6]]
            proj = np.array([utils.calc_projection_points(*p) for p in pp])
            fx = rng.uniform(-2, 6, size=(16, 9))
            fx[0, 1], fx[1, 1] = 40.0, -3.0   # the size clamps at the minimum / the maximum
            fk = rng.normal(0, 0.5, size=(16, 57)).astype(np.float32)
            res = []
            for t in range(16):
                tr = types.SimpleNamespace(state=types.SimpleNamespace(x=fx[t].reshape(9, 1)), keypoints=fk[t].astype(np.float64))
                (cx, cz), sz = fade["calc_fade_square"](tr)
                res.append([float(np.asarray(v).reshape(-1)[0]) for v in (cx, cz, sz)])
            out.update({f"raw_{i}": raw, f"norm_{i}": norm, f"raw32_{i}": raw32, f"norm32_{i}": norm32, f"cloud_{i}": cloud,
                        f"cloud_n_{i}": cn, f"feat_{i}": feat, f"proj_in_{i}": pp, f"proj_out_{i}": proj, f"fade_x_{i}": fx,
                        f"fade_kp_{i}": fk, f"fade_out_{i}": np.array(res)})
            print(f"  site {i}: h={row[0]} tilt={row[1]}: {len(raw)} rows -> {len(norm)} kept ({len(raw32)} fp32-exact -> {len(norm32)})")
    finally:
        for c, v in saved.items():
            setattr(const, c, v)
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sites.npz"))
