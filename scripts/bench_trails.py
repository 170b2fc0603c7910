"""What the track trails cost at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8, every scene holding 8
targets) with depth 64 and every ring full: the sample call, the full export and the export cut to the newest 8 points per track,
against mmw_report_* on the same state in the same process and against a plain device copy of the exported bytes -- and whether
the tracker's step moved: bench.py's tracker line on this build against the parent commit's.

    python scripts/bench_trails.py [--scenes 4096] [--pts 512] [--tracks 8] [--depth 64] [--fill 64] [--states 3] [--reps 20]
                                   [--parent DIR] [--runs 3] [--steps 80] [--bench-warmup 20] [--out profiles/trail_bench.json]

The tracker runs --fill frames with one mmw_trails_sample behind each; then, --states times, one more frame and its sample and,
--reps times in rotating order,
  trails       mmw_trails_async, every point: count, scan, write, the copy of the counts
  trails_last  mmw_trails_async with max_per_track = 8
  report       mmw_report_async into device buffers: count, scan, write, the copy of the counts
  copy         a device-to-device copy of as many bytes as `trails` wrote (directory and points)
each between two device events on the context's stream (idle before the first); then --reps times `sample`, mmw_trails_sample with
the frame's n_pts as flags and a time per scene (the repeats add samples to full rings: the counts of the exports do not move).
The first report of a state is not timed: it takes the frame's events.
--parent DIR: a checkout of the parent commit with its library built.  bench.py's tracker leg (no CPU, end-to-end, cold or shard
legs) then runs --runs times from either tree, alternating, a fresh process each; reported are every run's ms_per_step, the two
medians, their difference and the parent's own spread (max - min).  No threshold is asserted here; the numbers are quoted in
README.md and DESIGN.md 8j."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def run(a):
    import numpy as np
    from bench import generate

    # the generator forks its workers: before anything of this process has touched the GPU runtime
    S, N, T, W = a.scenes, a.pts, a.tracks, a.fill
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    print(f"bench_trails: generated {W + a.states} frames", file=sys.stderr, flush=True)
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trails.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    sb.enable_trails(a.depth)
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    d_clock = torch.from_numpy(np.cumsum(dts, axis=0)).to(dev)
    cap = S * sb.track_cap
    cap_p = cap * a.depth
    tdt, pdt = _lib.TRAIL_TRACK_DTYPE.itemsize, _lib.TRAIL_POINT_DTYPE.itemsize
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    d_dir = torch.zeros(cap * tdt, dtype=torch.uint8, device=dev)
    d_pts = torch.zeros(cap_p * pdt, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(cap * tdt + cap_p * pdt, dtype=torch.uint8, device=dev)

    def step(f):
        p = torch.from_numpy(pts[f]).to(dev)   # fp32 rows
        with torch.cuda.stream(st):
            sb.step_dev_f32(p.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
            sb.sample_trails_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())
        st.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    copied = [0]                      # bytes the full export of the state wrote: what `copy` moves
    d_src = torch.zeros_like(d_copy)
    calls = {
        "trails": (lambda: sb.trails_dev(d_dir.data_ptr(), cap, d_pts.data_ptr(), cap_p, 0, 0), lambda: sb.trails_wait(0)),
        "trails_last": (lambda: sb.trails_dev(d_dir.data_ptr(), cap, d_pts.data_ptr(), cap_p, a.last, 1), lambda: sb.trails_wait(1)),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
        "copy": (lambda: d_copy[: copied[0]].copy_(d_src[: copied[0]]), lambda: (copied[0], 0)),
    }
    for f in range(W):
        step(f)
    print("bench_trails: rings filled", file=sys.stderr, flush=True)
    t = {k: [] for k in list(calls) + ["sample"]}
    counts = {k: [] for k in calls}
    order = list(calls)
    for k in range(a.states):
        f = W + k
        step(f)
        timed(calls["report"][0])      # untimed: this frame's events are taken
        calls["report"][1]()
        timed(calls["trails"][0])
        n_t, n_p = calls["trails"][1]()
        copied[0] = n_t * tdt + n_p * pdt
        for r in range(a.reps):
            for name in order[r % len(order):] + order[: r % len(order)]:
                t[name].append(timed(calls[name][0]))
                counts[name].append(calls[name][1]())
        for r in range(a.reps):
            t["sample"].append(timed(lambda: sb.sample_trails_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())))
        print(f"bench_trails: state {k} timed", file=sys.stderr, flush=True)
    live = int(sb.num_tracks().sum())
    sb.check()
    sb.close()

    out = {"live_tracks_last_state": live, "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0)}
    for name in t:
        v = t[name]
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "all": v}}
        if name in counts and name != "copy":
            out[name]["entries"] = sorted(set(c[0] for c in counts[name]))
            out[name]["points_or_events"] = sorted(set(c[1] for c in counts[name]))
    out["copy"]["bytes"] = sorted(set(c[0] for c in counts["copy"]))
    out["copy"]["GBps_median"] = float(np.median([c[0] for c in counts["copy"]])) / out["copy"]["us"]["median"] / 1e3
    out["trails"]["bytes"] = out["copy"]["bytes"]
    out["trails"]["GBps_median"] = float(np.median([c[0] for c in counts["copy"]])) / out["trails"]["us"]["median"] / 1e3
    for name in ("trails", "trails_last", "sample"):
        out[name]["ratio_to_report"] = out[name]["us"]["median"] / out["report"]["us"]["median"]
    out["trail_state_bytes"] = S * sb.track_cap * (24 * a.depth + 40) + 12 * S
    return out


def main():
    from bench_zones import tracker_ab   # (the same A/B of bench.py's tracker line)
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--fill", type=int, default=64, help="frames, each followed by a sample call, before anything is timed")
    ap.add_argument("--last", type=int, default=8, help="max_per_track of the cut export")
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the tracker A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trail_bench.json"))
    a = ap.parse_args()
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets, trail depth {a.depth}, "
                       f"{a.fill} frames sampled before the first timed call",
           "fill_frames": a.fill, "states": a.states, "reps_per_state": a.reps, "max_per_track_of_trails_last": a.last,
           "timing": "device events on the context's stream, idle before the first; microseconds"}
    res.update(run(a))
    res["tracker"] = tracker_ab(a) if a.parent else "not measured (--parent not given)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) or "us" not in v else {kk: vv for kk, vv in v.items() if kk != "us"} | {"us_best": v["us"]["best"], "us_median": v["us"]["median"]})
                      for k, v in res.items()}, sort_keys=True))


if __name__ == "__main__":
    main()
