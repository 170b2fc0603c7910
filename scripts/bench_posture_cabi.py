#!/usr/bin/env python3
"""The batched estimate_posture of the C-ABI against what it stands beside, on one GPU (K = T population: 4096 scenes x 512 points x
8 tracks, the e2e leg's 31.7 k samples; S / FRAMES / REPEATS from the environment for smaller boxes):

  dense2   k_mars_dense2 (mmw_mars_dense2) against torch.addmm on the same operands, as MarsCNN.forward calls it
           (addmm(bias, hidden, weight.t(), out=kp)): HIP-event pairs around ITERS launches, alternating, REPEATS each;
           `hidden` bytes / time as a fraction of the 6.3 TB/s copy rate.
  frame    step + mmw_estimate_posture per frame against step + PosturePipeline(overlap=False) on the same frames, alternating,
           REPEATS each, a host clock around a loop that ends in a device synchronise; the overlapped schedule beside it for context.
           Gate: the C entry is not slower than the serial pipeline by more than the spread (max - min) of the pipeline's repeats.
  attach   mmw_posture_attach once (split of 9.4 M weights + allocations): reported, not gated.

Writes one JSON document to argv[1] (default profiles/posture_cabi_bench.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import torch  # noqa: E402
from mmwave_msc_amd import _lib  # noqa: E402
from mmwave_msc_amd.batch import SceneBatch  # noqa: E402
from mmwave_msc_amd.mars import MarsCNN  # noqa: E402
from mmwave_msc_amd.marsweights import random_keras_weights  # noqa: E402
from mmwave_msc_amd.posture import PosturePipeline  # noqa: E402

S, N, T = int(os.environ.get("S", 4096)), 512, 8
F = int(os.environ.get("FRAMES", 10))
REPEATS, ITERS = max(5, int(os.environ.get("REPEATS", 7))), 20
COPY_RATE = 6.3e12   # B/s, the measured HBM copy rate (profiles/README.md)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "posture_cabi_bench.json")
dev = torch.device("cuda:0")
L = _lib.load()
w = random_keras_weights(0, 3)
cnn = MarsCNN.from_keras_weights(w).to(dev)
res = {"config": f"{S} scenes x {N} points x TR_MAX_TRACKS={T}, population full, {F} frames, {REPEATS} repeats"}


def stats(v):
    return {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4), "spread": round(max(v) - min(v), 4), "all": [round(x, 4) for x in v]}


# ---- dense2 against torch.addmm --------------------------------------------------------------------------------------------
n = 31744 if S >= 4096 else max(256, S * 7 // 256 * 256)
g = torch.Generator().manual_seed(1)
hidden = torch.relu(torch.randn((n, 1536), generator=g) * 1.5 + 0.3).to(dev)
kp_a, kp_b = torch.empty((n, 57), device=dev), torch.empty((n, 57), device=dev)
bias, wt = cnn.dense2.bias, cnn.dense2.weight


def run_hip():
    rc = L.mmw_mars_dense2(torch.cuda.current_stream().cuda_stream or None, hidden.data_ptr(), 1536, wt.data_ptr(), bias.data_ptr(), kp_a.data_ptr(), n, 1536)
    assert rc == 0, L.mmw_last_error(None)


def run_addmm():
    torch.addmm(bias, hidden, wt.t(), out=kp_b)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e3   # us per launch


with torch.no_grad():
    for _ in range(3):
        run_hip(); run_addmm()
    torch.cuda.synchronize()
    t_hip, t_mm = [], []
    for _ in range(REPEATS):
        t_hip.append(timed(run_hip)); t_mm.append(timed(run_addmm))
want = bias.double() + hidden.double() @ wt.double().t()
scale = want.abs().clamp(min=1.0)
res["dense2"] = {"rows": n, "hidden_bytes": n * 1536 * 4, "k_mars_dense2_us": stats(t_hip), "torch_addmm_us": stats(t_mm),
                 "k_mars_dense2_fraction_of_copy_rate": round(n * 1536 * 4 / (float(np.median(t_hip)) * 1e-6) / COPY_RATE, 3),
                 "torch_addmm_fraction_of_copy_rate": round(n * 1536 * 4 / (float(np.median(t_mm)) * 1e-6) / COPY_RATE, 3),
                 "k_mars_dense2_err_vs_fp64": float(((kp_a.double() - want).abs() / scale).max()),
                 "torch_addmm_err_vs_fp64": float(((kp_b.double() - want).abs() / scale).max())}
del hidden, kp_a, kp_b, want, scale

# ---- per frame: the C entry against the serial PosturePipeline ---------------------------------------------------------------
pts, cnt, dts = bench.generate(np.arange(S), F, N, T, workers=8, population="full")
cap = S * 2 * T
ctx_c = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
ctx_p = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
ctx_o = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
t0 = time.perf_counter()
ctx_c.attach_posture_batch(w, cap)
ctx_c.synchronize()
res["attach_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
pipe_p = PosturePipeline(ctx_p, cnn, cap, overlap=False)
pipe_o = PosturePipeline(ctx_o, cnn, cap, overlap=True)
d_pts = torch.from_numpy(pts).to(dev)   # fp32 rows: mmw_step_f32
d_cnt, d_dt = torch.from_numpy(cnt).to(dev), torch.from_numpy(dts).to(dev)
torch.cuda.synchronize()
rows_c = [0]


def loop_c():
    ctx_c.reset()
    rows_c[0] = 0
    for f in range(F):
        ctx_c.step_dev_f32(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        rows_c[0] += ctx_c.estimate_posture()
    ctx_c.synchronize()


def loop_pipe(ctx, pipe):
    def run():
        ctx.reset()
        for f in range(F):
            ctx.step_dev_f32(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
            pipe.after_step()
        pipe.drain()
    return run


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / F * 1e3   # ms per frame


loops = {"c_entry": loop_c, "pipeline_serial": loop_pipe(ctx_p, pipe_p), "pipeline_overlapped": loop_pipe(ctx_o, pipe_o)}
for fn in loops.values():
    fn(); fn()
times = {k: [] for k in loops}
for _ in range(REPEATS):
    for k, fn in loops.items():
        times[k].append(clock(fn))
res["frame_ms"] = {k: stats(v) for k, v in times.items()}
res["frame_rows_total"] = rows_c[0]
res["overlap_note"] = pipe_o.overlap_note
ser, ce = res["frame_ms"]["pipeline_serial"], res["frame_ms"]["c_entry"]
res["gate_c_entry_not_slower_than_serial_plus_its_spread"] = bool(ce["median"] <= ser["median"] + ser["spread"])
# same keypoints (the two differ by Dense-2's summation order only)
ctx_c.check(); ctx_p.check()
na, nb = ctx_c.num_tracks(), ctx_p.num_tracks()
ta, tb = ctx_c.tracks(cap=max(int(na.max()), 1)), ctx_p.tracks(cap=max(int(nb.max()), 1))
res["tracks_equal"] = bool(np.array_equal(na, nb) and np.array_equal(ta["x"], tb["x"]))
res["keypoints_max_abs_diff"] = float(np.abs(ta["keypoints"].astype(np.float64) - tb["keypoints"]).max())
pipe_p.close(); pipe_o.close()
for c in (ctx_c, ctx_p, ctx_o):
    c.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
