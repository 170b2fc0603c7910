"""What it costs to learn how the live tracks stand, at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8,
every scene holding 8 targets): mmw_skeletons_* against mmw_report_* on the same state, and against the route a caller had before.

    python scripts/bench_skeletons.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--states 3] [--reps 20] [--out profiles/skeleton_bench.json]

The tracker runs --warmup frames; then, --states times, one more frame, random keypoints planted on every live track (half of them
with a SpineMid - Neck distance above 0.5, so MMW_SKEL_DRAWN drops half) and, --reps times in rotating order,
  skeletons_all / skeletons_drawn   mmw_skeletons_async into a device buffer: count, scan, write, the copy of the counts
  report                            mmw_report_async into device buffers: count, scan, write, the copy of the counts
each between two device events on the context's stream (idle before the first).  Once per state, on the host clock:
  host_route    report_host() and the numpy transform of its rows (the track position there is fp32: the report's rows carry no fp64
                state, which is one reason this route does not reproduce the reference's arithmetic)
Reported per variant: best and median in microseconds and the entries written; `ratio_to_report` is median over median.  No
threshold is asserted here; the numbers are quoted in README.md and profiles/README.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_keypoints(rng, n):
    """float32[n, 57]: uniform keypoints; SpineMid - Neck (columns 1 and 2 of the reshape(3, 19) view) 0 .. 0.45 or 0.55 .. 1.2 apart."""
    import numpy as np
    kp = rng.uniform(-1.0, 2.0, size=(n, 57)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.where(rng.integers(0, 2, size=n) > 0, rng.uniform(0.55, 1.2, size=n), rng.uniform(0.0, 0.45, size=n))
    for c in range(3):
        kp[:, 19 * c + 1] = (kp[:, 19 * c + 2].astype(np.float64) + r * d[:, c]).astype(np.float32)
    return kp


def host_transform(rows):
    """The numpy a caller of report_host() runs for the same picture: (skipped[n], joint float32[n, 19, 3])."""
    import numpy as np
    m = rows["keypoints"].reshape(-1, 3, 19)
    g = (m[:, :, 1] - m[:, :, 2]).astype(np.float64)
    skipped = (g * g).sum(axis=1) > 0.25
    joint = np.empty((len(rows), 19, 3), np.float32)
    joint[:, :, 0] = (-(m[:, 0].astype(np.float64)) + rows["x"][:, 0:1].astype(np.float64)).astype(np.float32)
    joint[:, :, 1] = (m[:, 2].astype(np.float64) + rows["x"][:, 1:2].astype(np.float64)).astype(np.float32)
    joint[:, :, 2] = m[:, 1]
    return skipped, joint


def run(a):
    import numpy as np
    import torch
    from bench import generate
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch

    S, N, T, W = a.scenes, a.pts, a.tracks, a.warmup
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    cap = S * sb.track_cap
    d_skel = torch.zeros(cap * 256, dtype=torch.uint8, device=dev)
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(8700)

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
        "skeletons_all": (lambda: sb.skeletons_dev(d_skel.data_ptr(), cap, _lib.SKEL_ALL, 0), lambda: sb.skeletons_wait(0)),
        "skeletons_drawn": (lambda: sb.skeletons_dev(d_skel.data_ptr(), cap, _lib.SKEL_DRAWN, 0), lambda: sb.skeletons_wait(0)),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
    }
    for f in range(W):
        step(f)
    t = {k: [] for k in calls}
    counts = {k: [] for k in calls}
    host = []
    order = list(calls)
    for k in range(a.states):
        step(W + k)
        ntr = sb.num_tracks()
        owner = np.stack([np.repeat(np.arange(S, dtype=np.int32), ntr), np.concatenate([np.arange(n, dtype=np.int32) for n in ntr])], axis=1)
        sb.set_keypoints_host(random_keypoints(rng, len(owner)), owner)
        for name in order:          # every shape the timed window uses, once (and the report's events of this frame are taken)
            timed(calls[name][0])
            calls[name][1]()
        for r in range(a.reps):
            for name in order[r % 3:] + order[: r % 3]:
                t[name].append(timed(calls[name][0]))
                counts[name].append(calls[name][1]())
        st.synchronize()
        t0 = time.perf_counter()
        rows, _ = sb.report_host()
        t1 = time.perf_counter()
        skipped, joint = host_transform(rows)
        t2 = time.perf_counter()
        host.append({"rows": len(rows), "report_host_us": (t1 - t0) * 1e6, "numpy_us": (t2 - t1) * 1e6, "total_us": (t2 - t0) * 1e6,
                     "skipped": int(skipped.sum())})
    sb.check()
    sb.close()

    out = {}
    for name in calls:
        v = t[name]
        second = "events" if name == "report" else "live_tracks"   # (report_wait returns rows and events)
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "all": v},
                     "entries": sorted(set(c[0] for c in counts[name])), second: sorted(set(c[1] for c in counts[name]))}
    for name in ("skeletons_all", "skeletons_drawn"):
        out[name]["ratio_to_report"] = out[name]["us"]["median"] / out["report"]["us"]["median"]
        out[name]["bytes_written_per_entry"] = 256
    out["report"]["bytes_written_per_entry"] = _lib.TRACK_REPORT_DTYPE.itemsize
    out["host_route"] = {"per_state": host, "best_total_us": min(h["total_us"] for h in host)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_bench.json"))
    a = ap.parse_args()
    import torch
    from mmwave_msc_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeletons.py measures on the GPU: no device, no number")
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets", "warmup_frames": a.warmup,
           "states": a.states, "reps_per_state": a.reps,
           "timing": "device events on the context's stream, idle before the first; microseconds (host_route: host clock)",
           "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0)}
    res.update(run(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v if k == "host_route" or not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "us"} | {"us_best": v["us"]["best"], "us_median": v["us"]["median"]})
                      for k, v in res.items()}, sort_keys=True))


if __name__ == "__main__":
    main()
