"""What the stance watch costs, at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8, every scene holding
8 targets) with a rule in every scene and a log of 256 events: mmw_stance_sample and mmw_stance_* against mmw_tripwires_sample
(16 wires per scene) and mmw_report_* on the same state in the same process -- and whether the tracker's step moved: bench.py's
tracker line on this build against the parent commit's.

    python scripts/bench_stance.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--states 3] [--reps 20]
                                   [--parent DIR] [--runs 3] [--steps 80] [--bench-warmup 20] [--out profiles/stance_bench.json]

The tracker runs --warmup frames; then, --states times, one more frame, keypoints planted for every live track (mmw_set_keypoints:
head 1.5 m, UPRIGHT) and, --reps times in rotating order,
  sample            mmw_stance_sample on a state whose keypoints did not change since the previous sample: nobody changes class
  export_empty      mmw_stance_async with an empty log: count, scan, rows, the copy of the counts
  tripwires_sample  mmw_tripwires_sample (16 wires per scene, nobody crosses) on the same state
  report            mmw_report_async into device buffers
each between two device events on the context's stream (idle before the first).  Then the changing case, --reps times: the heads of
every fourth live track are planted at 0.25 m and at 1.5 m in turn (the others keep theirs), and behind each planting
  sample_changing   mmw_stance_sample: about a quarter of the tracks change class, half of those samples as FALLs
  export_changed    mmw_stance_async right behind it: the rows and those events
The rule is the default one with long_lie = +inf, so that the quiet samples stay quiet however long the run.  --parent DIR: a
checkout of the parent commit with its library built; bench.py's tracker leg then runs --runs times from either tree, alternating
(scripts/bench_zones.py's tracker_ab).  No threshold is asserted here; the numbers are quoted in DESIGN.md 8l."""
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
    from bench_tripwires import wires

    # the generator forks its workers: before anything of this process has touched the GPU runtime
    S, N, T, W = a.scenes, a.pts, a.tracks, a.warmup
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    print(f"bench_stance: generated {W + a.states} frames", file=sys.stderr, flush=True)
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stance.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    sb.enable_tripwires(256)
    sb.set_tripwires(wires(S))
    sb.enable_stance(256)
    nr, rt = _lib.make_stance_rules([[dict(long_lie=float("inf"))]])
    sb.set_stance_rules((np.repeat(nr, S), np.repeat(rt, S, axis=0)))
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    cap = S * sb.track_cap
    cap_se = S * 256
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(S * _lib.STANCE_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_se = torch.zeros(cap_se * _lib.STANCE_EVENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def step(f):
        p = torch.from_numpy(pts[f]).to(dev)   # fp32 rows
        with torch.cuda.stream(st):
            sb.step_dev_f32(p.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        st.synchronize()

    def plant(kp, owner):
        with torch.cuda.stream(st):
            sb.set_keypoints_dev(kp.data_ptr(), owner.data_ptr(), len(owner))
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
        sb.stance_async(d_sr.data_ptr(), S, d_se.data_ptr(), cap_se, 0, 0)

    calls = {
        "sample": (lambda: sb.sample_stance_dev(None, None), None),
        "export_empty": (export, lambda: sb.stance_wait(0)),
        "tripwires_sample": (lambda: sb.sample_tripwires_dev(None, None), None),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
    }
    for f in range(W):
        step(f)
    print("bench_stance: warmed up", file=sys.stderr, flush=True)
    names = list(calls) + ["sample_changing", "export_changed"]
    t = {k: [] for k in names}
    counts = {k: [] for k in names}
    live, moved = [], []
    order = list(calls)
    for k in range(a.states):
        step(W + k)
        ntr = sb.num_tracks()
        own = np.array([(s, j) for s in range(S) for j in range(int(ntr[s]))], np.int32).reshape(-1, 2)
        up = np.zeros((len(own), _lib.NKP), np.float32)
        up[:, 22] = 1.5
        quarter = np.ascontiguousarray(own[::4])
        down = np.zeros((len(quarter), _lib.NKP), np.float32)
        down[:, 22] = 0.25
        d_own, d_up = torch.from_numpy(own).to(dev), torch.from_numpy(up).to(dev)
        d_q, d_down, d_qup = torch.from_numpy(quarter).to(dev), torch.from_numpy(down).to(dev), torch.from_numpy(up[: len(quarter)].copy()).to(dev)
        plant(d_up, d_own)
        for name in order:          # untimed: the shapes of the timed window; the frame's events and first classifications are taken
            timed(calls[name][0])
            if calls[name][1]:
                calls[name][1]()
        for r in range(a.reps):
            for name in order[r % 4:] + order[: r % 4]:
                t[name].append(timed(calls[name][0]))
                if calls[name][1]:
                    counts[name].append(calls[name][1]())
        live.append(int(ntr.sum()))
        moved.append(len(quarter))
        for r in range(a.reps):     # down and up again: every fourth track changes class behind each planting
            plant(d_down if r % 2 == 0 else d_qup, d_q)
            t["sample_changing"].append(timed(calls["sample"][0]))
            t["export_changed"].append(timed(export))
            counts["export_changed"].append(sb.stance_wait(0))
        print(f"bench_stance: state {k} timed", file=sys.stderr, flush=True)
    sb.check()
    sb.close()

    out = {"live_tracks_per_state": live, "tracks_changing_per_state": moved, "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0)}
    for name in names:
        v = t[name]
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "spread": float(max(v) - min(v)), "all": v}}
        if counts[name]:
            out[name]["rows"] = sorted(set(c[0] for c in counts[name]))
            ev = [c[1] for c in counts[name]]
            out[name]["events"] = {"min": min(ev), "median": float(np.median(ev)), "max": max(ev)}
    for name in ("sample", "sample_changing"):
        out[name]["ratio_to_tripwires_sample"] = out[name]["us"]["median"] / out["tripwires_sample"]["us"]["median"]
    for name in ("export_empty", "export_changed"):
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
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the tracker A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stance_bench.json"))
    a = ap.parse_args()
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets, one stance rule per scene "
                       "(defaults, long_lie = +inf), log depth 256, 16 wires per scene",
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
