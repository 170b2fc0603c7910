"""What the dwell heat maps cost at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8, every scene holding 8
targets) with a 32 x 32 grid in every scene: the sample call, the KEEP export of a sparse map (the state after --fill steps) and of a
full map (every cell touched), a CLEAR export of each, against mmw_trails_sample and mmw_report_* on the same state in the same
process and against a plain device copy of the bytes the export must move -- and whether the tracker's step moved: bench.py's
tracker line on this build against the parent commit's.

    python scripts/bench_heat.py [--scenes 4096] [--pts 512] [--tracks 8] [--fill 100] [--states 3] [--reps 20]
                                 [--parent DIR] [--runs 3] [--steps 80] [--bench-warmup 20] [--out profiles/heat_bench.json]

The tracker runs --fill frames with one mmw_heat_sample (and one mmw_trails_sample, depth 16) behind each; then, --states times, one
more frame with its samples and, --reps times in rotating order,
  heat_keep   mmw_heat_async, MMW_HEAT_KEEP: count, scan, write, the copy of the counts
  report      mmw_report_async into device buffers: count, scan, write, the copy of the counts
  copy        a device-to-device copy of as many bytes as the export must move: 4 B per cell of every scene for the count pass, 16 B
              per kept cell, and the rows and cells written
each between two device events on the context's stream (idle before the first); then --reps times `sample` (mmw_heat_sample) and
`trails_sample` (mmw_trails_sample), each with the frame's n_pts as flags and a time per scene.  The first report of a state is not
timed: it takes the frame's events.  `heat_clear` is ONE MMW_HEAT_CLEAR export of the last state (a second one would find an empty
map).
The full map: every scene's tracks are replaced, through one snapshot blob, by track_cap tracks standing in track_cap different cells,
and sampled; ceil(1024 / track_cap) such rounds touch every cell once.  Then `heat_keep_full` and `copy_full` --reps times in turn,
and ONE `heat_clear_full`.
--parent DIR: a checkout of the parent commit with its library built.  bench.py's tracker leg then runs --runs times from either tree,
alternating, a fresh process each (scripts/bench_zones.py has the code); reported are every run's ms_per_step, the two medians, their
difference and the parent's own spread.  No threshold is asserted here; README.md and DESIGN.md 8n quote what a run gave."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NX = NY = 32
GRID = dict(x0=-4.0, y0=0.0, cell=0.25, max_gap=1.0, nx=NX, ny=NY, id=0)


def planted_blob(sb, first_cell):
    """A snapshot blob of every scene of `sb`: track_cap tracks, track k in the centre of cell first_cell + k of GRID (wrapping)."""
    from tests._snap_plant import context_blob   # (the one place that builds version-1 sections by hand)
    cells = [(first_cell + k) % (NX * NY) for k in range(sb.track_cap)]
    return context_blob(sb, list(range(sb.track_cap)), [(GRID["x0"] + (c % NX + 0.5) * GRID["cell"], GRID["y0"] + (c // NX + 0.5) * GRID["cell"]) for c in cells])


def run(a):
    import numpy as np
    from bench import generate

    # the generator forks its workers: before anything of this process has touched the GPU runtime
    S, N, T, W = a.scenes, a.pts, a.tracks, a.fill
    pts, cnt, dts = generate(np.arange(S), W + a.states, N, T, workers=16, population="full")
    print(f"bench_heat: generated {W + a.states} frames", file=sys.stderr, flush=True)
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_heat.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.enable_report()
    sb.enable_trails(16)
    n_cells = NX * NY
    sb.enable_heat(n_cells)
    sb.set_heat_grids(_lib.make_heat_grids([[GRID]] * S))
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    d_clock = torch.from_numpy(np.cumsum(dts, axis=0)).to(dev)
    cap = S * sb.track_cap
    rdt, cdt = _lib.HEAT_ROW_DTYPE.itemsize, _lib.HEAT_CELL_DTYPE.itemsize
    d_rows = torch.zeros(cap * _lib.TRACK_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ev = torch.zeros(2 * cap * 16, dtype=torch.uint8, device=dev)
    d_hrows = torch.zeros(S * rdt, dtype=torch.uint8, device=dev)
    d_hcells = torch.zeros(S * n_cells * cdt, dtype=torch.uint8, device=dev)
    full_bytes = 4 * S * n_cells + (16 + cdt) * S * n_cells + rdt * S
    d_copy = torch.zeros(full_bytes, dtype=torch.uint8, device=dev)
    d_src = torch.zeros_like(d_copy)

    def step(f):
        p = torch.from_numpy(pts[f]).to(dev)   # fp32 rows
        with torch.cuda.stream(st):
            sb.step_dev_f32(p.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
            sb.sample_trails_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())
            sb.sample_heat_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())
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

    def moved(n_rows, n_kept):
        return 4 * S * n_cells + 16 * n_kept + rdt * n_rows + cdt * n_kept

    def heat(clear, ticket):
        return lambda: sb.heat_dev(d_hrows.data_ptr(), S, d_hcells.data_ptr(), S * n_cells, clear=clear, ticket=ticket)

    copied = [0]
    calls = {
        "heat_keep": (heat(False, 0), lambda: sb.heat_wait(0)),
        "report": (lambda: sb.report_async(d_rows.data_ptr(), cap, d_ev.data_ptr(), 2 * cap, 0, 0), lambda: sb.report_wait(0)),
        "copy": (lambda: d_copy[: copied[0]].copy_(d_src[: copied[0]]), lambda: (copied[0], 0)),
    }
    for f in range(W):
        step(f)
    print("bench_heat: filled", file=sys.stderr, flush=True)
    names = list(calls) + ["sample", "trails_sample", "heat_clear", "heat_keep_full", "copy_full", "heat_clear_full"]
    t = {k: [] for k in names}
    counts = {k: [] for k in names}
    order = list(calls)
    f = W
    for k in range(a.states):
        f = W + k
        step(f)
        timed(calls["report"][0])      # untimed: this frame's events are taken
        calls["report"][1]()
        timed(calls["heat_keep"][0])
        copied[0] = moved(*calls["heat_keep"][1]())
        for r in range(a.reps):
            for name in order[r % len(order):] + order[: r % len(order)]:
                t[name].append(timed(calls[name][0]))
                counts[name].append(calls[name][1]())
        for r in range(a.reps):
            t["sample"].append(timed(lambda: sb.sample_heat_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())))
            t["trails_sample"].append(timed(lambda: sb.sample_trails_dev(d_cnt[f].data_ptr(), d_clock[f].data_ptr())))
        print(f"bench_heat: state {k} timed", file=sys.stderr, flush=True)
    live = int(sb.num_tracks().sum())
    t["heat_clear"].append(timed(heat(True, 1)))
    counts["heat_clear"].append(sb.heat_wait(1))
    assert sb.heat_host()[1].size == 0
    sb.check()

    # the full map (a refused restore leaves the figures above standing: the full-map entries then say why they are missing)
    full_error = None
    m = sb.track_cap
    try:
        for k in range((n_cells + m - 1) // m):
            sb.restore(planted_blob(sb, k * m))
            sb.sample_heat_dev(None, None)
        sb.synchronize()
        print("bench_heat: every cell touched", file=sys.stderr, flush=True)
        timed(heat(False, 0))
        n_rows, n_kept = sb.heat_wait(0)
        assert (n_rows, n_kept) == (S, S * n_cells), (n_rows, n_kept)
        copied[0] = moved(n_rows, n_kept)
        for r in range(a.reps):
            for name in (("heat_keep_full", "copy_full") if r % 2 == 0 else ("copy_full", "heat_keep_full")):
                if name == "copy_full":
                    t[name].append(timed(calls["copy"][0]))
                    counts[name].append((copied[0], 0))
                else:
                    t[name].append(timed(heat(False, 0)))
                    counts[name].append(sb.heat_wait(0))
        t["heat_clear_full"].append(timed(heat(True, 1)))
        counts["heat_clear_full"].append(sb.heat_wait(1))
        assert sb.heat_host()[1].size == 0
    except _lib.MmwError as e:
        full_error = str(e)
    sb.close()

    out = {"live_tracks_last_state": live, "track_cap": m, "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0)}
    for name in t:
        v = t[name]
        if not v:
            out[name] = f"not measured: {full_error}"
            continue
        out[name] = {"us": {"best": min(v), "median": float(np.median(v)), "all": v}}
        if name.startswith("heat_"):
            out[name]["rows"] = sorted(set(c[0] for c in counts[name]))
            out[name]["cells"] = sorted(set(c[1] for c in counts[name]))
            out[name]["bytes_moved"] = sorted(set(moved(*c) for c in counts[name]))
            out[name]["GBps_median"] = float(np.median([moved(*c) for c in counts[name]])) / out[name]["us"]["median"] / 1e3
        if name.startswith("copy"):
            out[name]["bytes"] = sorted(set(c[0] for c in counts[name]))
            out[name]["GBps_median"] = float(np.median([c[0] for c in counts[name]])) / out[name]["us"]["median"] / 1e3
    out["heat_keep"]["ratio_to_copy"] = out["heat_keep"]["us"]["median"] / out["copy"]["us"]["median"]
    out["heat_keep"]["ratio_to_report"] = out["heat_keep"]["us"]["median"] / out["report"]["us"]["median"]
    if full_error is None:
        out["heat_keep_full"]["ratio_to_copy"] = out["heat_keep_full"]["us"]["median"] / out["copy_full"]["us"]["median"]
    out["sample"]["ratio_to_trails_sample"] = out["sample"]["us"]["median"] / out["trails_sample"]["us"]["median"]
    out["heat_state_bytes"] = S * (16 * n_cells + 16 * m + 36) + 56 * S
    return out


def main():
    from bench_zones import tracker_ab   # (the same A/B of bench.py's tracker line)
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--fill", type=int, default=100, help="frames, each followed by a sample call, before anything is timed")
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the tracker A/B")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heat_bench.json"))
    a = ap.parse_args()
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}, every scene with {a.tracks} targets, a {NX} x {NY} grid of 0.25 m cells "
                       f"per scene, {a.fill} frames sampled before the first timed call",
           "fill_frames": a.fill, "states": a.states, "reps_per_state": a.reps,
           "timing": "device events on the context's stream, idle before the first; microseconds; heat_clear and heat_clear_full are ONE call each"}
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
