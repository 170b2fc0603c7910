"""What per-scene sites cost in k_normalize, k_features and k_table at the benchmark workload (bench.py: 4096 scenes x 512
points, TR_MAX_TRACKS 8, K = T population).

    python scripts/bench_sites.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--frames 12] [--reps 5] [--no-sites-only]

Every frame is mmw_normalize (raw rows) -> mmw_step -> mmw_features -> mmw_track_table on device buffers.  After a warm window
of --warmup frames the three kernels are timed with mmw_profile_get over --frames frames (events on the kernels' own packets);
that is one repeat.  Repeats ALTERNATE between "no sites" (the kernels of a context that never set any) and "distinct" (every
scene its own site: 4096 different mountings, intensity scales and windows, close enough to the default that the same rows are
kept), so that drift of the box shows in both.  Prints one JSON line: per mode and kernel the mean time per launch in
microseconds of every repeat, their median and spread (max - min).  --no-sites-only: only the first mode -- the form that also
runs on a checkout that has no sites, for the comparison with the parent commit: copy this script into scripts/ of a built
checkout of the parent and run it there with the flag, alternating with this tree in the same GPU visit.

No posture model is attached (the attached chain is for one-scene contexts); the features are taken with mmw_features, the launch
PosturePipeline uses, and after the warm window every track is given random keypoints once, so that k_table's fade-square
arithmetic runs on non-zero values."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sites-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import expand_device, pool_counts, scene_pool
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch

    S, N, T, W, F = a.scenes, a.pts, a.tracks, a.warmup, a.frames
    pool = scene_pool(np.arange(S), W + F, N, T, workers=16, population="full")
    cnt, dts = pool_counts(pool)
    dev = torch.device("cuda", 0)
    pts = expand_device(pool, dev, torch.float64)                      # [W + F][S][N][8] room-frame rows
    cfg = _lib.default_config(tr_max_tracks=T)
    # the raw sensor rows of a default-mounted radar: the inverse of normalize_data's transform
    c, s = cfg.tilt_cos, cfg.tilt_sin
    y, z = pts[..., 1], pts[..., 2] - cfg.s_height
    raw = torch.stack([pts[..., 0], c * y + s * z, -s * y + c * z, pts[..., 6], pts[..., 7]], dim=-1).contiguous()
    del pts, y, z
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    sb = SceneBatch(cfg, S, N)
    sb.follow_torch_stream()
    norm = torch.zeros((S, N, 8), dtype=torch.float64, device=dev)
    n_out = torch.zeros(S, dtype=torch.int32, device=dev)
    cap = S * sb.track_cap
    feat = torch.zeros((cap, sb.ring, 8, 8, 5), dtype=torch.float32, device=dev)
    owner = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    table = torch.zeros((S * T, _lib.SUMMARY_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
    kernels = {"k_normalize": _lib.K_NORMALIZE, "k_features": _lib.K_FEATURES, "k_table": _lib.K_TABLE}

    def frame(f):
        sb.normalize_dev(raw[f].data_ptr(), d_cnt[f].data_ptr(), norm.data_ptr(), n_out.data_ptr())
        sb.step_dev(norm.data_ptr(), n_out.data_ptr(), d_dt[f].data_ptr())
        rows = sb.features_dev(feat.data_ptr(), owner.data_ptr(), cap)
        sb.track_table_dev(table.data_ptr(), T)
        return rows

    def repeat():
        sb.reset()
        for f in range(W):
            frame(f)
        sb.check()
        rows = sb.features_dev(feat.data_ptr(), owner.data_ptr(), cap)
        if rows:
            kp = torch.randn((rows, 57), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            sb.set_keypoints_dev(kp.data_ptr(), owner.data_ptr(), rows)
        sb.profile(True, kernels=list(kernels.values()))
        sb.profile_reset()
        rows = 0
        for f in range(W, W + F):
            rows = frame(f)
        torch.cuda.synchronize()
        out = {}
        for name, kid in kernels.items():
            ms, launches = sb.profile_get(kid)
            assert launches == F, (name, launches)
            out[name] = 1e3 * ms / launches
        sb.profile(False)
        return out, int(rows), int(n_out.sum().item())

    modes = ["none"] if a.no_sites_only else ["none", "distinct"]
    sites = None
    if not a.no_sites_only:
        u = np.linspace(-1.0, 1.0, S)
        sites = _lib.make_sites(cfg, S, s_height=cfg.s_height + 0.02 * u, s_tilt=-5.0 + 0.2 * u, intensity_mu=cfg.intensity_mu + 5 * u,
                                intensity_std=cfg.intensity_std * (1 + 0.1 * u), m_x=cfg.m_x + 0.3 * u, m_z=cfg.m_z + 0.2 * u,
                                v_screen_fade_weight=cfg.v_screen_fade_weight * (1 + 0.5 * u))
    res = {m: {k: [] for k in kernels} for m in modes}
    work = {}
    for _ in range(a.reps):
        for m in modes:
            if m == "distinct":
                sb.set_sites(sites)
            elif not a.no_sites_only:
                sb.clear_sites()
            t, rows, kept = repeat()
            work[m] = {"feature_rows_last_frame": rows, "rows_kept_last_frame": kept}
            for k, v in t.items():
                res[m][k].append(round(v, 3))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    summary = {m: {k: {"us_per_launch": v, "median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)}
                   for k, v in res[m].items()} for m in modes}
    print(json.dumps({"workload": f"{S} scenes x {N} points, TR_MAX_TRACKS {T}, K = T, {W} warm frames, {F} timed frames, {a.reps} repeats per mode, alternated",
                      "library": sb.L.mmw_version().decode(), "commit": commit, "work": work, "modes": summary}))
    sb.close()


if __name__ == "__main__":
    main()
