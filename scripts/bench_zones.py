"""What it costs to learn which zones are occupied, at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8,
every scene holding 8 targets) with 16 zones per scene: mmw_zones_* against mmw_report_* on the same state in the same process -- and
whether the tracker's step moved: bench.py's tracker line on this build against the parent commit's.

    python scripts/bench_zones.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--states 3] [--reps 20]
                                  [--parent DIR] [--runs 3] [--steps 80] [--bench-warmup 20] [--out profiles/zone_bench.json]

The tracker runs --warmup frames; then, --states times, one more frame and, --reps times in rotating order,
  zones    mmw_zones_async into device buffers: count, scan, write, the copy of the counts
  report   mmw_report_async into device buffers: count, scan, write, the copy of the counts
each between two device events on the context's stream (idle before the first).  The first call of either on a new state is not
timed: it takes the frame's events, so the timed repeats are the steady state of a room in which nobody crosses a line (rows are
always written; `events_first` is what the untimed call carried).  `zones_moved` times the other extreme: mmw_set_zones in front of
every repeat voids every membership, so each timed call emits a REBASED per scene and an ENTER per membership.
--parent DIR: a checkout of the parent commit with its library built.  bench.py's tracker leg (no CPU, end-to-end, cold or shard
legs) then runs --runs times from either tree, alternating, a fresh process each; reported are every run's ms_per_step, the two
medians, their difference and the parent's own spread (max - min).  No threshold is asserted here; the numbers are quoted in
README.md and DESIGN.md 8i."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def strips(n_scenes):
    """16 strips across x = -4 .. 4 (0.5 m each), any y, margin 0.05, per scene."""
    import numpy as np
    from mmwave_msc_amd import _lib
    one = [(-4.0 + 0.5 * k, -3.5 + 0.5 * k, -np.inf, np.inf, 0.05, k) for k in range(16)]
    nz, zt = _lib.make_zones([one])
    return np.repeat(nz, n_scenes), np.repeat(zt, n_scenes, axis=0)


def run(a):
    import numpy as np
    from bench import generate

    # the generator forks its workers: before anything of this process has touched the GPU runtime (a fork behind its
    # initialisation -- under a profiler, whose threads it does not carry over -- can leave the workers waiting for ever)
    S, N, T, W = a.scenes, a.pts, a.tracks, a.warmup
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    print(f"bench_zones: generated {W + a.states} frames", file=sys.stderr, flush=True)
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_zones.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    table = strips(S)
    sb.set_zones(table)
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    cap = S * sb.track_cap
    cap_zr, cap_ze = S * _lib.ZONES_MAX, S * (1 + 4 * sb.track_cap)   # (a track is in at most two neighbouring strips: leave two, enter two)
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    d_zr = torch.zeros(cap_zr * 32, dtype=torch.uint8, device=dev)
    d_ze = torch.zeros(cap_ze * 24, dtype=torch.uint8, device=dev)

    def step(f):
        p = torch.from_numpy(pts[f]).to(dev)   # fp32 rows
        with torch.cuda.stream(st):
            sb.step_dev_f32(p.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
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

    calls = {
        "zones": (lambda: sb.zones_async(d_zr.data_ptr(), cap_zr, d_ze.data_ptr(), cap_ze, 0, 0), lambda: sb.zones_wait(0)),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
    }
    for f in range(W):
        step(f)
    print("bench_zones: warmed up", file=sys.stderr, flush=True)
    t = {k: [] for k in list(calls) + ["zones_moved"]}
    counts = {k: [] for k in t}
    first = {k: [] for k in calls}
    order = list(calls)
    for k in range(a.states):
        step(W + k)
        for name in order:          # untimed: the shapes of the timed window, and this frame's events are taken
            timed(calls[name][0])
            first[name].append(calls[name][1]())
        for r in range(a.reps):
            for name in order[r % 2:] + order[: r % 2]:
                t[name].append(timed(calls[name][0]))
                counts[name].append(calls[name][1]())
        for r in range(a.reps):     # every membership void in front of each call: a REBASED per scene, an ENTER per membership
            sb.set_zones(table)
            t["zones_moved"].append(timed(calls["zones"][0]))
            counts["zones_moved"].append(calls["zones"][1]())
        print(f"bench_zones: state {k} timed", file=sys.stderr, flush=True)
    live = int(sb.num_tracks().sum())
    sb.check()
    sb.close()

    out = {"live_tracks_last_state": live, "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0)}
    for name in t:
        v = t[name]
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "all": v},
                     "rows": sorted(set(c[0] for c in counts[name])), "events": sorted(set(c[1] for c in counts[name]))}
        if name in first:
            out[name]["events_first"] = [c[1] for c in first[name]]
    for name in ("zones", "zones_moved"):
        out[name]["ratio_to_report"] = out[name]["us"]["median"] / out["report"]["us"]["median"]
    out["zones"]["bytes_written_per_row"], out["report"]["bytes_written_per_row"] = 32, _lib.TRACK_REPORT_DTYPE.itemsize
    return out


def tracker_line(root, a):
    """ms_per_step of bench.py's tracker leg, run from the tree at `root` in a fresh process."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.bench_warmup), "--no-cpu", "--no-e2e", "--no-e2e-parity",
           "--no-cold", "--no-shards", "--no-full", "--no-ingest", "--no-single"]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"bench.py in {root} failed ({res.returncode}): {res.stderr[-800:]}")
    return float(json.loads(res.stdout.strip().splitlines()[-1])["ms_per_step"])


def tracker_ab(a):
    import numpy as np
    this, parent = [], []
    for _ in range(a.runs):
        this.append(tracker_line(ROOT, a))
        parent.append(tracker_line(a.parent, a))
    return {"this_ms_per_step": this, "parent_ms_per_step": parent, "this_median": float(np.median(this)), "parent_median": float(np.median(parent)),
            "difference_ms": float(np.median(this) - np.median(parent)), "parent_spread_ms": float(max(parent) - min(parent)),
            "this_spread_ms": float(max(this) - min(this)), "steps": a.steps, "warmup": a.bench_warmup,
            "how": "bench.py --gpus 1, the tracker leg only, fresh processes alternating this / parent on one GPU"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the tracker A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zone_bench.json"))
    a = ap.parse_args()
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets, 16 zones per scene",
           "warmup_frames": a.warmup, "states": a.states, "reps_per_state": a.reps,
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
