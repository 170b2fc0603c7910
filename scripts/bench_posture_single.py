#!/usr/bin/env python3
"""mmw_estimate_posture with the single-frame model (define_CNN, a context with FB_FRAMES_BATCH = 0) beside the 3-frame model
(define_CNN_3D, FB_FRAMES_BATCH = 2) on one GPU, K = T population: 4096 scenes x 512 points x 8 tracks (S / FRAMES / REPEATS from
the environment for smaller boxes).  Both contexts track the same frames; then the call is repeated on each, alternating, between
device events on the stream both contexts run on: features, split conv pair, Dense-1, Dense-2, the four launches of the range
repair (no sample is outside fp16's range, so they find nothing to do) and the keypoint scatter.  No bar: the figures are for the
next reader.

Writes one JSON document to argv[1] (default profiles/posture_single_bench.json) and prints it."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import torch  # noqa: E402
from mmwave_msc_amd import _lib  # noqa: E402
from mmwave_msc_amd.batch import SceneBatch  # noqa: E402
from mmwave_msc_amd.marsweights import random_keras_weights  # noqa: E402

S, N, T = int(os.environ.get("S", 4096)), 512, 8
F = int(os.environ.get("FRAMES", 8))
REPEATS, WARM = max(5, int(os.environ.get("REPEATS", 40))), 5
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "posture_single_bench.json")
dev = torch.device("cuda:0")
pts, cnt, dts = bench.generate(np.arange(S), F, N, T, workers=8, population="full")
d_pts = torch.from_numpy(pts).to(dev)   # fp32 rows: mmw_step_f32
d_cnt, d_dt = torch.from_numpy(cnt).to(dev), torch.from_numpy(dts).to(dev)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
ctxs = {}
for frames in (1, 3):
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T, fb_frames_batch=frames - 1), S, N)
    sb.follow_torch_stream(st)
    sb.attach_posture_batch(random_keras_weights(0, frames), S * sb.track_cap)
    for f in range(F):
        sb.step_dev_f32(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        sb.estimate_posture()
    sb.synchronize()
    sb.check()
    ctxs[frames] = sb
times, rows = {1: [], 3: []}, {}
for rep in range(WARM + REPEATS):
    for frames, sb in ctxs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        rows[frames] = sb.estimate_posture()
        b.record(st)
        b.synchronize()
        if rep >= WARM:
            times[frames].append(a.elapsed_time(b))
res = {"config": f"{S} scenes x {N} points x TR_MAX_TRACKS={T}, population full, after {F} frames, {REPEATS} repeats, the two contexts alternating",
       "what": "mmw_estimate_posture between device events: k_features, k_mars_conv16, k_mars_dense1, k_mars_dense2, the four launches of the range repair "
               "(nothing to repair), k_set_kp; the host's wait for the row count lies inside the interval"}
for frames, sb in ctxs.items():
    t = times[frames]
    res["define_CNN" if frames == 1 else "define_CNN_3D"] = {
        "fb_frames_batch": frames - 1, "samples": int(rows[frames]), "ms": {"min": round(min(t), 4), "median": round(float(np.median(t)), 4), "max": round(max(t), 4)},
        "range_word": sb.posture_range()}
    sb.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
