"""What it costs to learn where the live tracks' points are, at the benchmark workload (bench.py: 4096 scenes x 512 points,
TR_MAX_TRACKS 8): mmw_clouds_* against a plain device-to-device copy of the same bytes and against the two routes a context offered before.

    python scripts/bench_clouds.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--reps 5] [--out profiles/cloud_bench.json]

Per population (full: every scene holds 8 targets; mixed: scene s holds 1 + s mod 8) the tracker runs --warmup frames, then --reps
times one more frame and, in rotating order,
  points / points+ring / rows / rows+ring   mmw_clouds_async into device buffers: count, scan, write (+ring = MMW_CLOUD_UNASSIGNED)
  copy                                      hipMemcpyAsync device to device of as many bytes as rows+ring writes: the copy rate of this
                                            device in this run
each between two device events on the context's stream (idle before the first).  Once per population, on the host clock (both wait
for the stream themselves):
  snapshot     mmw_snapshot of all scenes into a device buffer that is large enough: the bulk route to the same rows
  getter loop  mmw_get_track_ring_frame over every (track, frame) of the first 64 scenes, scaled to all scenes
Reported per variant: best and median in microseconds, the bytes it reads and writes (rows x 64 in and out for ROWS, rows x 24 in and
x 16 out for POINTS, + 32 per directory entry; all per repeat, since the frames differ), and the best (read + written) / time of
the repeats as a fraction of the copy's best 2 x bytes / time.  No
threshold is asserted anywhere; the numbers are quoted in DESIGN.md §8d."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"points": (False, False), "points+ring": (False, True), "rows": (True, False), "rows+ring": (True, True)}


def _hip_runtime(torch):
    """The HIP runtime this process already runs on (torch's own copy where torch bundles one), by file name; the global symbol
    scope only where no such file is found."""
    for d in (os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib"):
        p = os.path.join(d, "libamdhip64.so")
        if os.path.isfile(p):
            return C.CDLL(p)
    return C.CDLL(None)


def run_population(population, a):
    import numpy as np
    import torch
    from bench import generate
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import DevBuf, SceneBatch

    S, N, T, W, R = a.scenes, a.pts, a.tracks, a.warmup, a.reps
    pts, cnt, dts = generate(np.arange(S), W + R, N, T, workers=16, population=population)
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    hip = _hip_runtime(torch)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    cap_t = S * (sb.track_cap + 1)
    cap_p = S * (sb.track_cap * sb.ring * sb.ring_rows + sb.ring * N)
    d_dir = torch.zeros(cap_t * 32, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(cap_p * 64, dtype=torch.uint8, device=dev)
    d_src = torch.zeros(cap_p * 64, dtype=torch.uint8, device=dev)

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

    def clouds(name):
        rows, ring = VARIANTS[name]
        mode = (_lib.CLOUD_ROWS if rows else _lib.CLOUD_POINTS) | (_lib.CLOUD_UNASSIGNED if ring else 0)
        return lambda: sb.clouds_dev(d_dir.data_ptr(), cap_t, d_out.data_ptr(), cap_p, mode, 0)

    copy_bytes = [0]

    def copy():
        rc = hip.hipMemcpyAsync(d_out.data_ptr(), d_src.data_ptr(), copy_bytes[0], 3, st.cuda_stream)   # 3 = hipMemcpyDeviceToDevice
        assert rc == 0, rc

    for f in range(W):
        step(f)
    counts = {}
    for name in VARIANTS:   # every shape the timed window uses, once
        timed(clouds(name))
        counts[name] = sb.clouds_wait(0)
    copy_bytes[0] = counts["rows+ring"][1] * 64
    timed(copy)
    t = {k: [] for k in list(VARIANTS) + ["copy"]}
    per_rep = {k: [] for k in VARIANTS}     # (entries, points) of every repeat: the frames differ, so do the bytes
    copy_sizes = []
    order = list(t)
    for r in range(R):
        step(W + r)
        timed(clouds("rows+ring"))          # (untimed for the record: this frame's size for the copy)
        copy_bytes[0] = sb.clouds_wait(0)[1] * 64
        for name in order[r % len(order):] + order[: r % len(order)]:
            if name == "copy":
                t[name].append(timed(copy))
                copy_sizes.append(copy_bytes[0])
            else:
                t[name].append(timed(clouds(name)))
                per_rep[name].append(sb.clouds_wait(0))
    sb.check()

    def summary(v):
        return {"best": min(v), "median": float(np.median(v)), "all": v}

    # every rate is formed per repeat, from that repeat's bytes and time; "best" is the best RATE
    copy_rates = [2.0 * b / us for b, us in zip(copy_sizes, t["copy"])]   # bytes read + written per microsecond
    copy_rate = max(copy_rates)
    out = {"population": population, "track_cap": sb.track_cap, "ring": sb.ring, "ring_rows": sb.ring_rows,
           "copy": {"us": summary(t["copy"]), "bytes": copy_sizes, "rate_GBps": {"best": copy_rate / 1e3, "all": [v / 1e3 for v in copy_rates]}}}
    for name, (rows, ring) in VARIANTS.items():
        # read: the rows, the scene headers, and ring_len / uid / ring_n / ring_slot of a record, counted ONCE -- each of the four waves
        # of a scene's workgroup loads them, three of the four from cache: memory traffic, not instruction traffic, is what the
        # copy's rate is compared with; written: the rows or points and the directory
        rd = [n_p * (64 if rows else 24) + S * 64 + (n_t - (S if ring else 0)) * 40 for n_t, n_p in per_rep[name]]
        wr = [n_p * (64 if rows else 16) + n_t * 32 for n_t, n_p in per_rep[name]]
        rates = [(a_ + b_) / us for a_, b_, us in zip(rd, wr, t[name])]
        out[name] = {"us": summary(t[name]), "entries": [c[0] for c in per_rep[name]], "points": [c[1] for c in per_rep[name]],
                     "bytes_read": rd, "bytes_written": wr, "rate_GBps": {"best": max(rates) / 1e3, "all": [v / 1e3 for v in rates]},
                     "fraction_of_copy_rate": max(rates) / copy_rate}
    # the routes that existed before, on the host clock: both wait for the stream themselves
    snap = DevBuf(sb, sb.snapshot_size())
    sb.snapshot_dev(None, snap)
    st.synchronize()
    t0 = time.perf_counter()
    _, snap_bytes = sb.snapshot_dev(None, snap)
    out["snapshot_all_scenes"] = {"host_us": (time.perf_counter() - t0) * 1e6, "bytes": snap_bytes}
    snap.free()
    ntr, trk = sb.num_tracks(), sb.tracks()
    n_small = min(64, S)
    calls = 0
    t0 = time.perf_counter()
    for s in range(n_small):
        for j in range(int(ntr[s])):
            for k in range(int(trk[s, j]["ring_len"])):
                sb.track_ring_frame(s, j, k)
                calls += 1
    dt_us = (time.perf_counter() - t0) * 1e6
    out["getter_loop"] = {"scenes_timed": n_small, "calls": calls, "host_us": dt_us, "host_us_scaled_to_all_scenes": dt_us * S / n_small,
                          "calls_scaled": calls * S // n_small}
    sb.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.json"))
    a = ap.parse_args()
    import torch
    from mmwave_msc_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_clouds.py measures on the GPU: no device, no number")
    res = {"workload": f"{a.scenes} scenes x {a.pts} pts x TR_MAX_TRACKS={a.tracks}", "warmup_frames": a.warmup, "reps": a.reps,
           "timing": "device events on the context's stream, idle before the first; microseconds (snapshot and getter loop: host clock)",
           "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0),
           "populations": [run_population(p, a) for p in ("full", "mixed")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
