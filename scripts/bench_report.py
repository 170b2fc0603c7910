"""What it costs to learn who is in the scenes, at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8):
the live-track report against the only way a context offered before it.

    python scripts/bench_report.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--reps 5] [--out profiles/report_bench.json]

Per population (K = T: every scene holds 8 targets; mixed: scene s holds 1 + s mod 8) the tracker runs --warmup frames, then
--reps times: one more frame (so that every repeat has events to report), and -- ALTERNATING which goes first --
  report   mmw_report_async into device buffers sized S x track_cap: count, scan, write
  table    mmw_track_table at slots = track_cap (dead slots included), plus mmw_get_tracks at cap = track_cap for the uids (the
           track table carries no identity): its export kernel and its read-back into host memory, which that entry cannot be
           asked to leave out
each between two device events on the context's stream (the stream is idle before the first).  Reported per variant: the best
and the median of the repeats in microseconds, and the bytes it writes -- rows x 324 + events x 16 against
S x track_cap x (336 + 1504).  `table_only_us` is mmw_track_table alone: what a caller that needs no uid paid.  No time
threshold is asserted anywhere; the numbers are quoted in DESIGN.md §8c."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_population(population, a):
    import numpy as np
    import torch
    from bench import generate
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch

    S, N, T, W, R = a.scenes, a.pts, a.tracks, a.warmup, a.reps
    pts, cnt, dts = generate(np.arange(S), W + R, N, T, workers=16, population=population)
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    cap = S * sb.track_cap
    rdt, edt, sdt, tdt = _lib.TRACK_REPORT_DTYPE, _lib.TRACK_EVENT_DTYPE, _lib.SUMMARY_DTYPE, _lib.TRACK_DTYPE
    rows = torch.zeros(cap * rdt.itemsize, dtype=torch.uint8, device=dev)
    events = torch.zeros(2 * cap * edt.itemsize, dtype=torch.uint8, device=dev)
    table = torch.zeros(cap * sdt.itemsize, dtype=torch.uint8, device=dev)
    tracks_host = np.zeros((S, sb.track_cap), dtype=tdt)
    sb.enable_report()

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

    counts = []

    def report():
        sb.report_async(rows.data_ptr(), cap, events.data_ptr(), 2 * cap, 0, 0)

    def table_and_uids():
        sb.track_table_dev(table.data_ptr(), sb.track_cap)
        sb._chk(sb.L.mmw_get_tracks(sb.h, tracks_host.ctypes.data, sb.track_cap))

    def table_only():
        sb.track_table_dev(table.data_ptr(), sb.track_cap)

    for f in range(W):
        step(f)
    for fn in (report, table_and_uids, table_only):   # every shape the timed window uses, once
        timed(fn)
    sb.report_wait(0)
    t = {"report": [], "table": [], "table_only": []}
    for r in range(R):
        step(W + r)
        order = ("report", "table") if r % 2 == 0 else ("table", "report")
        for which in order:
            t[which].append(timed(report if which == "report" else table_and_uids))
            if which == "report":
                counts.append(sb.report_wait(0))
        t["table_only"].append(timed(table_only))
    sb.check()
    n_rows = [c[0] for c in counts]
    n_events = [c[1] for c in counts]
    bytes_report = [c[0] * rdt.itemsize + c[1] * edt.itemsize for c in counts]
    bytes_table = cap * (sdt.itemsize + tdt.itemsize)
    out = {
        "population": population, "track_cap": sb.track_cap, "live_rows": n_rows, "events": n_events,
        "tracks_per_scene": float(np.mean(n_rows)) / S,
        "report_us": {"best": min(t["report"]), "median": float(np.median(t["report"])), "all": t["report"]},
        "table_plus_get_tracks_us": {"best": min(t["table"]), "median": float(np.median(t["table"])), "all": t["table"]},
        "table_only_us": {"best": min(t["table_only"]), "median": float(np.median(t["table_only"])), "all": t["table_only"]},
        "bytes_report": bytes_report, "bytes_table_plus_get_tracks": bytes_table, "bytes_table_only": cap * sdt.itemsize,
        "ratio_time_best": min(t["table"]) / min(t["report"]),
        "ratio_time_table_only_best": min(t["table_only"]) / min(t["report"]),
        "ratio_bytes": bytes_table / max(1.0, float(np.mean(bytes_report))),
        "ratio_bytes_table_only": cap * sdt.itemsize / max(1.0, float(np.mean(bytes_report))),
    }
    sb.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_bench.json"))
    a = ap.parse_args()
    import torch
    from mmwave_msc_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_report.py measures on the GPU: no device, no number")
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}", "warmup_frames": a.warmup, "reps": a.reps,
           "timing": "device events on the context's stream, idle before the first; microseconds",
           "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0),
           "populations": [run_population(p, a) for p in ("full", "mixed")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
