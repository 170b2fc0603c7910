"""What it costs to count passages, at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8, every scene
holding 8 targets) with 16 wires per scene and a log of 256 events: mmw_tripwires_sample and mmw_tripwires_* against
mmw_trails_sample (depth 64) and mmw_report_* on the same state in the same process -- and whether the tracker's step moved:
bench.py's tracker line on this build against the parent commit's.

    python scripts/bench_tripwires.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--states 3] [--reps 20]
                                      [--swing 1.0] [--parent DIR] [--runs 3] [--steps 80] [--bench-warmup 20]
                                      [--out profiles/tripwire_bench.json]

The tracker runs --warmup frames; then, --states times, one more frame and, --reps times in rotating order,
  sample          mmw_tripwires_sample on a state that did not move since the previous sample: nobody crosses
  export_empty    mmw_tripwires_async with an empty log: count, scan, rows, the copy of the counts
  trails_sample   mmw_trails_sample (depth 64) on the same state
  report          mmw_report_async into device buffers
each between two device events on the context's stream (idle before the first).  Then the crossing case, --reps times: a step on
an empty frame whose dt swings the tracks --swing seconds along their velocities and back again (predict is x += (lifetime + dt) v,
so dt = +swing, -2 swing, +2 swing, ... walks every moving track to and fro over the same wires), and behind each such step
  sample_crossing mmw_tripwires_sample: `events` of it are crossings
  export_crossed  mmw_tripwires_async right behind it: the rows and those events
The wires are 16 parallel lines 0.25 m apart with no band, so a track that moves a quarter of a metre across them crosses one; how
many events a crossing sample logged, and how many tracks were live, is in the output -- a track that stands still crosses nothing.
--parent DIR: a checkout of the parent commit with its library built; bench.py's tracker leg then runs --runs times from either
tree, alternating (scripts/bench_zones.py's tracker_ab).  No threshold is asserted here; the numbers are quoted in README.md and
DESIGN.md 8k."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def wires(n_scenes):
    """16 wires per scene from (c, 12) to (c, -4), c = -2 + 0.25 k, no band."""
    import numpy as np
    from mmwave_msc_amd import _lib
    nw, wt = _lib.make_tripwires([[(-2.0 + 0.25 * k, 12.0, -2.0 + 0.25 * k, -4.0, 0.0, k) for k in range(16)]])
    return np.repeat(nw, n_scenes), np.repeat(wt, n_scenes, axis=0)


def run(a):
    import numpy as np
    from bench import generate

    # the generator forks its workers: before anything of this process has touched the GPU runtime
    S, N, T, W = a.scenes, a.pts, a.tracks, a.warmup
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    print(f"bench_tripwires: generated {W + a.states} frames", file=sys.stderr, flush=True)
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tripwires.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    sb.enable_trails(64)
    sb.enable_tripwires(256)
    sb.set_tripwires(wires(S))
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    d_empty = torch.full((S,), _lib.EMPTY_FRAME, dtype=torch.int32, device=dev)
    d_nopts = torch.zeros((S, N, 8), dtype=torch.float32, device=dev)
    cap = S * sb.track_cap
    cap_wr, cap_we = S * _lib.TRIPWIRES_MAX, S * 256
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    d_wr = torch.zeros(cap_wr * 32, dtype=torch.uint8, device=dev)
    d_we = torch.zeros(cap_we * 32, dtype=torch.uint8, device=dev)

    def step(f):
        p = torch.from_numpy(pts[f]).to(dev)   # fp32 rows
        with torch.cuda.stream(st):
            sb.step_dev_f32(p.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        st.synchronize()

    def swing(dt):
        d = torch.full((S,), float(dt), dtype=torch.float64, device=dev)
        with torch.cuda.stream(st):
            sb.step_dev_f32(d_nopts.data_ptr(), d_empty.data_ptr(), d.data_ptr())
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

    def export():
        sb.tripwires_async(d_wr.data_ptr(), cap_wr, d_we.data_ptr(), cap_we, 0, 0)

    calls = {
        "sample": (lambda: sb.sample_tripwires_dev(None, None), None),
        "export_empty": (export, lambda: sb.tripwires_wait(0)),
        "trails_sample": (lambda: sb.sample_trails_dev(None, None), None),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
    }
    for f in range(W):
        step(f)
    print("bench_tripwires: warmed up", file=sys.stderr, flush=True)
    names = list(calls) + ["sample_crossing", "export_crossed"]
    t = {k: [] for k in names}
    counts = {k: [] for k in names}
    live = []
    order = list(calls)
    for k in range(a.states):
        step(W + k)
        for name in order:          # untimed: the shapes of the timed window; the frame's events and crossings are taken
            timed(calls[name][0])
            if calls[name][1]:
                calls[name][1]()
        for r in range(a.reps):
            for name in order[r % 4:] + order[: r % 4]:
                t[name].append(timed(calls[name][0]))
                if calls[name][1]:
                    counts[name].append(calls[name][1]())
        live.append(int(sb.num_tracks().sum()))
        lifetime = 0.0              # (of a track the frame updated; the others swing by their own lifetime more, and back)
        for r in range(a.reps):     # to and fro: every moving track crosses the wires between its two positions
            target = a.swing if r % 2 == 0 else -a.swing
            swing(target - lifetime)
            lifetime = target
            t["sample_crossing"].append(timed(calls["sample"][0]))
            t["export_crossed"].append(timed(export))
            counts["export_crossed"].append(sb.tripwires_wait(0))
        print(f"bench_tripwires: state {k} timed", file=sys.stderr, flush=True)
    sb.check()
    sb.close()

    out = {"live_tracks_per_state": live, "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0), "swing_s": a.swing}
    for name in names:
        v = t[name]
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "spread": float(max(v) - min(v)), "all": v}}
        if counts[name]:
            out[name]["rows"] = sorted(set(c[0] for c in counts[name]))
            ev = [c[1] for c in counts[name]]
            out[name]["events"] = {"min": min(ev), "median": float(np.median(ev)), "max": max(ev)}
    for name in ("sample", "sample_crossing"):
        out[name]["ratio_to_trails_sample"] = out[name]["us"]["median"] / out["trails_sample"]["us"]["median"]
    for name in ("export_empty", "export_crossed"):
        out[name]["ratio_to_report"] = out[name]["us"]["median"] / out["report"]["us"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--swing", type=float, default=1.0, help="seconds the empty-frame steps of the crossing case swing the tracks by")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the tracker A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tripwire_bench.json"))
    a = ap.parse_args()
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets, 16 wires per scene, log depth 256, trail depth 64",
           "warmup_frames": a.warmup, "states": a.states, "reps_per_state": a.reps,
           "timing": "device events on the context's stream, idle before the first; microseconds; one run on one GPU"}
    res.update(run(a))
    if a.parent:
        from bench_zones import tracker_ab
        res["tracker"] = tracker_ab(a)
    else:
        res["tracker"] = "not measured (--parent not given)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) or "us" not in v else {kk: vv for kk, vv in v.items() if kk != "us"} | {"us_best": v["us"]["best"], "us_median": v["us"]["median"]})
                      for k, v in res.items()}, sort_keys=True))


if __name__ == "__main__":
    main()
