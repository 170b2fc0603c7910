#!/usr/bin/env python3
"""mmw_estimate_posture with several posture models behind it (mmw_posture_attach_models) on one GPU: 4096 scenes x 512
points x 8 tracks, the 3-frame model, after 8 frames (S / FRAMES / REPEATS from the environment for smaller boxes).  One context
per variant, all tracking the same frames; then the call is repeated on each, the variants alternating, between device events on
the stream they share:

  legacy             one model through mmw_posture_attach_frames
  models_1           the same model through mmw_posture_attach_models (the same launches)
  models_2 / 4 / 8   that many models, the scenes dealt round-robin
  halves_2           two models, scenes 0 .. S/2-1 on the first

No bar on the multi-model variants: min / median / max, the rows per band and the launches per call are for the next reader.  The
one condition is on the one-model path, which claims to run what it always ran: with PARENT_TREE=<a checkout of the parent commit,
built> the `legacy` variant alone is timed in fresh processes, this build and the parent's alternating, and the difference of
the medians must lie inside the spread of the parent's own runs.

  bench_posture_models.py [out.json]                      the variants (+ the comparison when PARENT_TREE is set)
  bench_posture_models.py --legacy-only data.npz          (a child of the comparison: prints its times as JSON; runs on the parent too)
  bench_posture_models.py --kernel-stats stats.csv [out.json]   fold the device times of k_feat_scan / k_feat_scan_models from a
                                                          kernel-trace statistics file of this script's run into out.json
"""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("MMW_TREE", HERE)   # the checkout whose package is measured
DEFAULT_OUT = os.path.join(HERE, "profiles", "posture_models_bench.json")
S, N, T = int(os.environ.get("S", 4096)), 512, 8
F = int(os.environ.get("FRAMES", 8))
REPEATS, WARM = max(5, int(os.environ.get("REPEATS", 30))), 5
ROUNDS = int(os.environ.get("ROUNDS", 3))


def fold_kernel_stats(stats_csv, out_path):
    rows = {}
    with open(stats_csv) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            for k in ("k_feat_scan_models", "k_feat_scan", "k_feat_count"):
                if k in name and (k != "k_feat_scan" or "k_feat_scan_models" not in name):
                    rows[k] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                               "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    with open(out_path) as fh:
        res = json.load(fh)
    res["scan_device_time"] = dict(rows, what=f"device time per launch at S = {res.get('scenes', S)}, from a kernel trace of this script's run")
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["scan_device_time"]))


if len(sys.argv) > 1 and sys.argv[1] == "--kernel-stats":
    fold_kernel_stats(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT)
    sys.exit(0)

sys.path.insert(0, TREE)
import torch  # noqa: E402
from mmwave_msc_amd import _lib  # noqa: E402
from mmwave_msc_amd.batch import SceneBatch  # noqa: E402
from mmwave_msc_amd.marsweights import random_keras_weights  # noqa: E402

dev = torch.device("cuda:0")


def frames_on_device(path):
    z = np.load(path)
    return torch.from_numpy(z["pts"]).to(dev), torch.from_numpy(z["cnt"]).to(dev), torch.from_numpy(z["dts"]).to(dev)


def tracked_context(st, data, attach):
    d_pts, d_cnt, d_dt = data
    sb = SceneBatch(_lib.default_config(tr_max_tracks=T), S, N)
    sb.follow_torch_stream(st)
    attach(sb)
    for f in range(F):
        sb.step_dev_f32(d_pts[f].data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr())
        sb.estimate_posture()
    sb.synchronize()
    sb.check()
    return sb


def timed(st, ctxs, repeats):
    times, rows = {k: [] for k in ctxs}, {}
    for rep in range(WARM + repeats):
        for name, sb in ctxs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            rows[name] = sb.estimate_posture()
            b.record(st)
            b.synchronize()
            if rep >= WARM:
                times[name].append(a.elapsed_time(b))
    return times, rows


def stats(t):
    return {"min": round(min(t), 4), "median": round(float(np.median(t)), 4), "max": round(max(t), 4)}


if len(sys.argv) > 1 and sys.argv[1] == "--legacy-only":
    st = torch.cuda.Stream(device=dev)
    sb = tracked_context(st, frames_on_device(sys.argv[2]), lambda sb: sb.attach_posture_batch(random_keras_weights(0, 3), S * sb.track_cap))
    times, rows = timed(st, {"legacy": sb}, REPEATS)
    sb.close()
    print("LEGACY " + json.dumps({"version": _lib.load().mmw_version().decode(), "rows": rows["legacy"], "ms": stats(times["legacy"])}))
    sys.exit(0)

import bench  # noqa: E402
import tempfile  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
pts, cnt, dts = bench.generate(np.arange(S), F, N, T, workers=8, population="full")
tmp = tempfile.mkdtemp()
data_path = os.path.join(tmp, "frames.npz")
np.savez(data_path, pts=pts, cnt=cnt, dts=dts)
data = frames_on_device(data_path)
torch.cuda.synchronize()
st = torch.cuda.Stream(device=dev)
weights = [random_keras_weights(seed, 3) for seed in range(8)]
maps = {"models_1": (1, np.zeros(S, np.int32)), "models_2": (2, np.arange(S, dtype=np.int32) % 2), "models_4": (4, np.arange(S, dtype=np.int32) % 4),
        "models_8": (8, np.arange(S, dtype=np.int32) % 8), "halves_2": (2, (np.arange(S) >= S // 2).astype(np.int32))}
ctxs = {"legacy": tracked_context(st, data, lambda sb: sb.attach_posture_batch(weights[0], S * sb.track_cap))}
for name, (n, smap) in maps.items():
    ctxs[name] = tracked_context(st, data, lambda sb, n=n, smap=smap: sb.attach_posture_models(weights[:n], smap, S * sb.track_cap))
times, rows = timed(st, ctxs, REPEATS)
L = _lib.load()
RANGE_REPAIR = 5   # k_range_gather, the fp32 conv pair, the two kernels of the small head, k_range_scatter


def launches(per_band):
    """count + scan + features, then per band: conv16, Dense-1's tile plan, Dense-2, the range repair, k_set_kp"""
    n = 3
    for r in per_band:
        if r > 0:
            plan = (C.c_int32 * 4)()
            assert L.mmw_mars_dense1_plan((int(r) + 255) // 256 * 256, 1536, plan) == 0
            n += 1 + sum(1 for v in plan[:3] if v > 0) + 1 + RANGE_REPAIR + 1
    return n


res = {"config": f"{S} scenes x {N} points x TR_MAX_TRACKS={T}, population full, the 3-frame model, after {F} frames, {REPEATS} repeats, the variants alternating in one process",
       "scenes": S,
       "what": "mmw_estimate_posture between device events: k_feat_count, the scan (k_feat_scan, or k_feat_scan_models where the rows are grouped), "
               "k_features, then per band k_mars_conv16, k_mars_dense1, k_mars_dense2, the range repair (nothing to repair), k_set_kp; the host's "
               "wait for the row counts lies inside the interval", "variants": {}}
for name, sb in ctxs.items():
    per = sb.posture_group_rows().tolist()
    res["variants"][name] = {"models": len(per), "rows": int(rows[name]), "rows_per_band": per, "launches_per_call": launches(per),
                             "ms": stats(times[name]), "range_word": sb.posture_range()}
    sb.close()
base = res["variants"]["legacy"]["ms"]["median"]
res["per_additional_band_ms"] = {k: round((v["ms"]["median"] - base) / (v["models"] - 1), 4) for k, v in res["variants"].items() if v["models"] > 1}

parent = os.environ.get("PARENT_TREE")
if parent:
    def child(tree):
        env = dict(os.environ, MMW_TREE=tree)
        env.pop("PARENT_TREE")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--legacy-only", data_path], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("LEGACY ")]
        assert out.returncode == 0 and line, out.stderr[-2000:]
        return json.loads(line[-1][len("LEGACY "):])

    runs = {"this": [], "parent": []}
    for _ in range(ROUNDS):   # fresh processes, the two builds alternating on the same box
        runs["this"].append(child(HERE))
        runs["parent"].append(child(parent))
    med = {k: [r["ms"]["median"] for r in v] for k, v in runs.items()}
    spread = max(med["parent"]) - min(med["parent"])
    diff = float(np.median(med["this"]) - np.median(med["parent"]))
    res["one_model_against_parent"] = {
        "what": f"the legacy variant alone in fresh processes, {ROUNDS} runs of {REPEATS} repeats per build, the builds alternating; ms per call",
        "this_build": {"version": runs["this"][0]["version"], "run_medians": med["this"], "median": round(float(np.median(med["this"])), 4)},
        "parent_build": {"version": runs["parent"][0]["version"], "run_medians": med["parent"], "median": round(float(np.median(med["parent"])), 4)},
        "parent_spread_ms": round(spread, 4), "difference_ms": round(diff, 4), "inside_parent_spread": bool(abs(diff) <= spread)}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
if parent:
    assert res["one_model_against_parent"]["inside_parent_spread"], res["one_model_against_parent"]
