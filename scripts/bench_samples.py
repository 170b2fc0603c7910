"""What it costs to turn the state after a step into training samples, at the benchmark workload (bench.py: 4096 scenes x 512 points,
TR_MAX_TRACKS 8): mmw_samples_* in both modes against a plain device-to-device copy of the same output bytes and against the path it
replaces -- mmw_clouds(MMW_CLOUD_ROWS) on the same state, read back, and the numpy restatement of the rule on the host.

    python scripts/bench_samples.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--reps 5] [--out profiles/sample_bench.json]

The tracker runs --warmup frames, then --reps times one more frame and, in rotating order,
  block / input     mmw_samples_async into device buffers, every scene asked: count, scan, write (MMW_SAMPLE_BLOCK / MMW_SAMPLE_INPUT)
  copy_block / copy_input   hipMemcpyAsync device to device of as many bytes as that mode wrote: the copy rate of this device in this run
  clouds_rows       mmw_clouds_async(MMW_CLOUD_ROWS): the device part of the replaced path
each between two device events on the context's stream (idle before the first).  Once, on the host clock:
  replaced path     clouds_host(rows=True) + tracks() read back, then per scene the rule and relative_coordinates +
                    format_batched_frames restated in numpy (the blocks are compared with the export's, bit for bit)
Reported per variant: best and median in microseconds and the samples of every repeat.  No threshold is asserted anywhere; the
numbers are quoted in DESIGN.md §8g."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK_BYTES, INPUT_BYTES, ENTRY_BYTES = 192 * 5 * 8, 64 * 5 * 4, 48


def _hip_runtime(torch):
    """The HIP runtime this process already runs on (torch's own copy where torch bundles one), by file name; the global symbol
    scope only where no such file is found."""
    for d in (os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib"):
        p = os.path.join(d, "libamdhip64.so")
        if os.path.isfile(p):
            return C.CDLL(p)
    return C.CDLL(None)


def host_blocks(np, d, rows, trk, ntr, ring_rows):
    """The replaced path's host part: from the clouds' directory and rows and the track records, every scene's block."""
    first_entry = np.concatenate([[0], np.cumsum(ntr)])[:-1]
    scenes, blocks = [], []
    for s in np.flatnonzero(ntr > 0):
        rec, e = trk[s, 0], d[first_entry[s]]
        rn = [int(v) for v in rec["ring_n"][: int(rec["ring_len"])]]
        if rec["lifetime"] != 0 or sum(rn) == 0:
            continue
        out = np.zeros((192, 5))
        at = int(e["first"]) + int(e["count"])
        for j, n in enumerate(reversed(rn)):          # newest first; the clouds hold at most ring_rows rows of a frame, oldest frame first
            stored = min(n, ring_rows)
            at -= stored
            fr = rows[at: at + min(stored, 64)][:, [0, 1, 2, 6, 7]].copy()
            fr[:, 0] -= rec["centroid"][0]
            fr[:, 1] -= rec["centroid"][1]
            out[j * 64: j * 64 + len(fr)] = fr
        scenes.append(s)
        blocks.append(out)
    return np.array(scenes), np.array(blocks).reshape(-1, 192, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import generate
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_samples.py measures on the GPU: no device, no number")

    S, N, T, W, R = a.scenes, a.pts, a.tracks, a.warmup, a.reps
    pts, cnt, dts = generate(np.arange(S), W + R, N, T, workers=16, population="full")
    dev = torch.device("cuda", 0)
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    d_cnt, d_dt = torch.from_numpy(cnt).to(dev), torch.from_numpy(dts).to(dev)
    hip = _hip_runtime(torch)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    d_dir = torch.zeros(S * ENTRY_BYTES, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(S * BLOCK_BYTES, dtype=torch.uint8, device=dev)
    d_src = torch.zeros(S * BLOCK_BYTES, dtype=torch.uint8, device=dev)
    cap_t, cap_p = S * sb.track_cap, S * sb.track_cap * sb.ring * sb.ring_rows
    c_dir = torch.zeros(cap_t * 32, dtype=torch.uint8, device=dev)
    c_out = torch.zeros(cap_p * 64, dtype=torch.uint8, device=dev)

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

    n_now = [0]
    runs = {
        "block": lambda: sb.samples_dev(d_dir.data_ptr(), S, d_out.data_ptr(), _lib.SAMPLE_BLOCK, None, 0),
        "input": lambda: sb.samples_dev(d_dir.data_ptr(), S, d_out.data_ptr(), _lib.SAMPLE_INPUT, None, 0),
        "copy_block": lambda: hip.hipMemcpyAsync(d_out.data_ptr(), d_src.data_ptr(), n_now[0] * BLOCK_BYTES, 3, st.cuda_stream),
        "copy_input": lambda: hip.hipMemcpyAsync(d_out.data_ptr(), d_src.data_ptr(), n_now[0] * INPUT_BYTES, 3, st.cuda_stream),
        "clouds_rows": lambda: sb.clouds_dev(c_dir.data_ptr(), cap_t, c_out.data_ptr(), cap_p, _lib.CLOUD_ROWS, 0),
    }
    waits = {"block": sb.samples_wait, "input": sb.samples_wait, "clouds_rows": sb.clouds_wait}

    for f in range(W):
        step(f)
    for name, fn in runs.items():   # every shape the timed window uses, once
        timed(fn)
        if name in waits:
            got = waits[name](0)
            if name == "block":
                n_now[0] = got
    t = {k: [] for k in runs}
    samples, order = [], list(runs)
    for r in range(R):
        step(W + r)
        timed(runs["block"])                 # (untimed for the record: this frame's sample count, for the copies)
        n_now[0] = sb.samples_wait(0)
        samples.append(n_now[0])
        for name in order[r % len(order):] + order[: r % len(order)]:
            t[name].append(timed(runs[name]))
            if name in waits:
                waits[name](0)
    sb.check()

    # the replaced path once, on the host clock, and its blocks against the export's
    sb.clouds_host(rows=True)   # (untimed: the host routes' buffers grow to their sizes)
    sb.samples_host()
    st.synchronize()
    t0 = time.perf_counter()
    d, rows = sb.clouds_host(rows=True)
    trk, ntr = sb.tracks(), sb.num_tracks()
    t1 = time.perf_counter()
    scenes, blocks = host_blocks(np, d, rows, trk, ntr, sb.ring_rows)
    t2 = time.perf_counter()
    sd, sblocks = sb.samples_host()
    t3 = time.perf_counter()
    same = bool(np.array_equal(sd["scene"], scenes) and sblocks.tobytes() == blocks.tobytes())
    sb.close()

    def summary(v):
        return {"best": min(v), "median": float(np.median(v)), "all": v}

    res = {"workload": f"{S} scenes x {N} pts x TR_MAX_TRACKS={T}", "warmup_frames": W, "reps": R,
           "timing": "device events on the context's stream, idle before the first; microseconds (replaced path: host clock)",
           "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0), "ring": sb.ring, "ring_rows": sb.ring_rows,
           "samples": samples,
           "bytes_written": {"block": [n * (BLOCK_BYTES + ENTRY_BYTES) for n in samples], "input": [n * (INPUT_BYTES + ENTRY_BYTES) for n in samples]},
           "us": {k: summary(v) for k, v in t.items()},
           "block_over_copy": min(t["block"]) / min(t["copy_block"]), "input_over_copy": min(t["input"]) / min(t["copy_input"]),
           "replaced_path": {"readback_host_us": (t1 - t0) * 1e6, "numpy_host_us": (t2 - t1) * 1e6, "total_host_us": (t2 - t0) * 1e6,
                             "samples_host_us": (t3 - t2) * 1e6, "samples": int(len(scenes)), "blocks_equal_the_exports": same,
                             "clouds_rows": int(len(rows)), "clouds_bytes_read_back": int(rows.nbytes + d.nbytes + trk.nbytes)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
