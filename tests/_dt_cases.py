"""The interval-schedule cases (tests/_fuzz.py: DT_SCHEDULES) of tests/test_reference_dt.py and tests/test_gpu_dt.py: the seed
list, and what the C oracle does on every (seed, schedule) pair -- on the CPU alone, no reference, no GPU.

A schedule tests something only where its odd intervals meet live tracks, so the seeds are CHOSEN, by conditions on the inputs
that `check` asserts on the oracle (they are no measurement of the code under test).  For every (seed, schedule):

  * no scene ends on a reference exception (LinAlgError rc=-2, ZeroDivisionError rc=-3);
  * on an out-of-band frame (dt outside 0.05 .. 0.2 s) a track takes points: a predict with an out-of-band lifetime + dt, then
    an update from it;
  * on an out-of-band frame a track goes unassigned and survives: `lifetime` accumulates an out-of-band dt;
  * negative: some track's lifetime is below zero after a frame;
  * long60, hour: a track expires on an out-of-band frame and a later DBSCAN call of the scene makes a track again.

What the drawn configurations cannot reach, and what stands in its place:

  * long60, hour: Q carries dtm^4 / 4 = 3.2e6 and more, log|det C| alone is beyond every drawn tr_gate (2.5 .. 7), so NO track takes a
    point on a 60 s frame, in any of seeds 0 .. 3999.  A 60 s predict that is then gated, on both sides of the gate, is the planted
    edge tests/_edge_inputs.py: long_predict.
  * long5: every drawn lifetime limit is <= 1.5 s, so an unassigned track cannot survive 5 s: it must expire, and a track must be
    made again, as under long60.  Under CONST_ACC (dim_x 9), whose Q also has the acceleration block, no track of seeds 0 .. 3999
    takes a point on a 5 s frame either; the CONST_VEL seeds do.

All the conditions together hold for some 18 of seeds 0 .. 3999 (a track must lose its points on exactly an odd frame and, for
long1, be static with a limit >= 1 s): four CONST_VEL seeds of those, and four CONST_ACC seeds that meet everything but the 5 s
update."""
import functools

import numpy as np

from tests._fuzz import DT_SCHEDULES, draw_case, dt_out_of_band, dt_schedule, scene_inputs

SEEDS = (18, 218, 555, 3834, 50, 260, 603, 776)            # dim_x 6, 6, 6, 6, 9, 9, 9, 9; none is a seek_inner seed (seed % 8 == 5)
CPU_SIZE = dict(max_pts=300, max_scenes=2, frames=12)      # the live reference's DBSCAN metric is a Python callable
GPU_SIZE = dict(max_pts=300, max_scenes=4, frames=12)      # a few tracks in a few scenes: k_predict, k_track and k_scene all run
TALLY_KEYS = ("frames", "oob_frames", "oob_updated", "oob_survived", "expired", "oob_expired", "respawned", "negative")


@functools.lru_cache(maxsize=None)
def oracle_tally(seed: int, name: str, max_scenes: int = CPU_SIZE["max_scenes"]) -> dict:
    """The oracle on draw_case(seed, max_scenes=...) under schedule `name`: counts over all scenes and frames.
    frames: track() calls; oob_frames: ... with dt out of band; oob_updated: tracks that took points on such a frame;
    oob_survived: tracks left unassigned on such a frame and kept; expired / oob_expired: tracks dropped (on such a frame);
    respawned: tracks DBSCAN made on a frame after an expiry of the same scene; negative: track records with lifetime < 0;
    raised: scenes that ended on a reference exception."""
    from oracle import c_oracle as co
    case = draw_case(seed, **dict(CPU_SIZE, max_scenes=max_scenes))
    assert not case["seek_inner"]
    pts, cnt, _ = scene_inputs(case)
    dts = dt_schedule(case, name)
    oob = dt_out_of_band(dts)
    cfg = co.default_config(**case["cfg"])
    t = dict.fromkeys(TALLY_KEYS + ("raised",), 0)
    for s in range(case["S"]):
        orc = co.OracleScene(cfg, case["N"])
        seen_expiry = False
        for f in range(case["F"]):
            c = int(cnt[f, s])
            if c == 0:
                continue
            before = orc.n_tracks
            try:
                assoc, labels = orc.track(pts[f, s, : max(c, 0)].astype(np.float64), float(dts[f, s]))
            except RuntimeError:
                t["raised"] += 1
                break
            # every cluster apply_DBscan finds becomes a track (Tracking.py:576-589); only an unassigned track can expire
            new = int(labels.max() + 1) if labels is not None and len(labels) else 0
            taken = len(np.unique(assoc[assoc >= 0]))
            expired = before + new - orc.n_tracks
            assert 0 <= expired <= before - taken, (seed, name, s, f)
            t["frames"] += 1
            t["expired"] += expired
            t["respawned"] += new if seen_expiry else 0
            seen_expiry |= expired > 0
            t["negative"] += int(np.sum(orc.tracks()["lifetime"] < 0))
            if oob[f, s]:
                t["oob_frames"] += 1
                t["oob_updated"] += taken
                t["oob_survived"] += before - taken - expired
                t["oob_expired"] += expired
    return t


def check(seed: int, name: str, max_scenes: int = CPU_SIZE["max_scenes"]) -> dict:
    """The conditions of this module's docstring, on the oracle."""
    t = oracle_tally(seed, name, max_scenes)
    ctx = (seed, name, max_scenes, t)
    dim_x = draw_case(seed, **CPU_SIZE)["cfg"]["dim_x"]
    assert t["raised"] == 0 and t["oob_frames"] >= 2, ctx
    if name in ("long60", "hour") or (name == "long5" and dim_x == 9):
        assert t["oob_updated"] == 0, ctx                    # (the day this fails, the condition below is reachable: ask for it)
    else:
        assert t["oob_updated"] >= 1, ctx
    if name in ("long5", "long60", "hour"):
        assert t["oob_survived"] == 0 and t["oob_expired"] >= 1 and t["respawned"] >= 1, ctx
    else:
        assert t["oob_survived"] >= 1, ctx
    if name == "negative":
        assert t["negative"] >= 1, ctx
    return t


def schedule_tally(name: str, max_scenes: int = CPU_SIZE["max_scenes"]) -> dict:
    """The tallies of one schedule over SEEDS (DESIGN.md quotes them)."""
    out = dict.fromkeys(TALLY_KEYS, 0)
    for seed in SEEDS:
        t = oracle_tally(seed, name, max_scenes)
        for k in TALLY_KEYS:
            out[k] += t[k]
    return out


assert len(DT_SCHEDULES) == 11 and not any(sd % 8 == 5 for sd in SEEDS)
