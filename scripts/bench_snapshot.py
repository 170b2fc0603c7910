"""Snapshot / restore throughput at the benchmark workload (bench.py: 4096 scenes x 512 points, TR_MAX_TRACKS 8, K = T
population), after a warm window of steps.

    python scripts/bench_snapshot.py [--scenes 4096] [--pts 512] [--tracks 8] [--warmup 12] [--reps 5]

Prints one JSON line: bytes per whole-context snapshot, the time of mmw_snapshot and mmw_restore between two device events
on the context's stream (best of --reps; each call is synchronous and is ONE C-ABI call into a reused buffer: the drain, the size
pass, one small read-back and the pack / the drain, two small reads of header and directory, the check kernel and its
read-back, the scrub and the unpack), and the rate against the 6.3 TB/s device-to-device copy of MI355X_MICROARCH.md
(a snapshot reads and writes its bytes once each: rate = 2 x bytes / time)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import expand_device, pool_counts, scene_pool
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch

    S, N, T, W = a.scenes, a.pts, a.tracks, a.warmup
    pool = scene_pool(np.arange(S), W, N, T, workers=16, population="full")
    cnt, dts = pool_counts(pool)
    dev = torch.device("cuda", 0)
    pts = expand_device(pool, dev, torch.float64)
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_dt = torch.from_numpy(dts).to(dev)
    cfg = _lib.default_config(tr_max_tracks=T)
    A = SceneBatch(cfg, S, N)
    A.follow_torch_stream()
    for f in range(W):
        A.step_dev(pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
    A.check()
    B = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    B.follow_torch_stream()
    torch.cuda.synchronize()
    buf, nbytes = A.snapshot_dev()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_snap, t_rest = [], []
    for _ in range(a.reps):
        ev[0].record()
        buf, nbytes = A.snapshot_dev(out=buf)
        ev[1].record()
        torch.cuda.synchronize()
        t_snap.append(ev[0].elapsed_time(ev[1]))
        ev[0].record()
        B.restore((buf, nbytes))
        ev[1].record()
        torch.cuda.synchronize()
        t_rest.append(ev[0].elapsed_time(ev[1]))
    assert B.snapshot() == A.snapshot(), "restored context differs"
    ts, tr = min(t_snap), min(t_rest)
    rate = lambda ms: 2 * nbytes / (ms * 1e-3) / 1e12
    print(json.dumps({"workload": f"{S} scenes x {N} points, TR_MAX_TRACKS {T}, K = T, after {W} steps",
                      "bytes": int(nbytes), "bytes_per_scene": round(nbytes / S, 1), "tracks": int(A.num_tracks().sum()),
                      "snapshot_ms": round(ts, 4), "restore_ms": round(tr, 4),
                      "snapshot_TBps": round(rate(ts), 3), "restore_TBps": round(rate(tr), 3),
                      "snapshot_of_copy": round(rate(ts) / COPY_TBPS, 3), "restore_of_copy": round(rate(tr) / COPY_TBPS, 3),
                      "snapshot_ms_all": [round(v, 4) for v in t_snap], "restore_ms_all": [round(v, 4) for v in t_rest]}))
    A.close()
    B.close()


if __name__ == "__main__":
    main()
