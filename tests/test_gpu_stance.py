"""The stance watch (mmw_stance_*, include/mmw.h) on the GPU: per scene zero or one rule, per live uid a class from the head height of
the posture keypoints, and changes, falls and long lies as events in a per-scene log.

Expected values come from tests/_stance_ref.py, a numpy restatement of the header section applied to the state read back with
`tracks()` / `num_tracks()` after each step; it carries its own rules, slots, counters and log.  Every field of every row and event
is compared by its bytes -- there is no tolerance anywhere: the device compares fp64 values the host derived and takes one fp64
difference for each of the two ages, and the squared gap is three products and two sums of widened fp32 differences in one order
(the library is built with -ffp-contract=off).

Keypoints are planted with `set_keypoints_host` behind each frame, from `_stance_ref.planted(scene, uid, frame)` or by hand; the CNN
runs in one test only.  What a sample reads is what the track records hold when its kernel runs, so the edge cases plant, sample and
plant again without a step in between: the uids stay, the heads are chosen."""
import numpy as np
import pytest

from tests._feature_run import BASE, REPORT, S2, TRACKS, StanceRun, TripRun, cut, head_kp as _kp, n_kind, nothing_else_moves, same_pair, settled, step_empty
from tests._layouts import make_checked
from tests._report_scenes import CFG_KW, F, N, S, scenario, wires16
from tests._snap_plant import FAR, directory, plant_state, record_at
from tests._stance_ref import HEAD, L, LOW, LYING, M, U, UPRIGHT, StanceRef, planted

pytestmark = pytest.mark.gpu

RULE = (1.25, 0.5, 0.125, 0.25, 0.5, 0.5)   # h_stand, h_lie, margin, fall_window, long_lie, max_gap: every derived threshold is exact
UP_HI, UP_LO, LIE_HI, LIE_LO, H_STAND, H_LIE = 1.375, 1.125, 0.625, 0.375, 1.25, 0.5
F32 = np.float32


def _up(x):
    """The next fp32 above x."""
    return np.nextafter(F32(x), F32(np.inf))


# 1 ------------------------------------------------------------------------------------------------------------------------
NO_RULE = (5, 17)


@pytest.mark.parametrize("layout", ["per_scene", "one_workgroup"])
def test_scenario_planted_sampled_every_frame_and_exported_every_third(layout):
    """24 scenes x 96 points x 12 frames; scenes 5 and 17 have no rule.  What came out of this run (both layouts alike): the tallies
    are printed, the figures of one MI355X run stand in DESIGN.md 8l."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.stance import Watch
    sb = make_checked(S, N, layout, **CFG_KW)
    run = StanceRun(sb, 64)
    run.set_rules([[RULE + (100 + s,)] if s not in NO_RULE else [] for s in range(S)])
    watch, last_rows = Watch(), None
    for f in range(F):
        run.step(f)
        run.plant(lambda s, j, uid: planted(s, uid, f))
        run.sample(t=0.125 * f)
        if f % 3 == 2:
            rows, events = run.compare((layout, f))
            watch.apply(events)
            assert len(rows) == S - len(NO_RULE) and not rows["lost"].any()
            assert not np.isin(rows["scene"] - BASE, NO_RULE).any() and not np.isin(events["scene"] - BASE, NO_RULE).any()
            last_rows = rows
    ntr, trk = sb.num_tracks(), sb.tracks()
    sb.check()
    sb.close()
    ref, tally = run.ref, run.ref.tally
    print("stance tallies", layout, sorted(tally.items()), "falls", int(ref.falls.sum()), "long_lies", int(ref.long_lies.sum()), "events", int(ref.logged.sum()))
    # the fold of the GPU's events = the restatement's slots: who is down at the end, and the totals
    down = {(BASE + s, int(trk[s, j]["uid"])) for s in range(S) if s not in NO_RULE for j in range(int(ntr[s])) if ref.cls(s, int(trk[s, j]["uid"])) == LYING}
    assert {k for k in watch.down() if k in {(BASE + s, int(trk[s, j]["uid"])) for s in range(S) for j in range(int(ntr[s]))}} == down
    assert (watch.falls, watch.long_lies) == (int(ref.falls.sum()), int(ref.long_lies.sum())) == (int(last_rows["falls"].sum()), int(last_rows["long_lies"].sum()))
    # the scenario holds every case the issue names, by the restatement's own count
    for key in ("first_upright", "first_low", "first_lying", "change_between_known", "fall_from_upright", "fall_through_low", "lay_down_slowly",
                "kept_upright_by_margin", "kept_below_upright_by_margin", "kept_lying_by_margin", "kept_above_lying_by_margin", "long_lie",
                "long_lie_not_repeated", "implausible_gap", "implausible_head", "slot_reused_after_lying", "asked_without_rule"):
        assert tally[key] >= 1, (key, sorted(tally.items()))


# 2 ------------------------------------------------------------------------------------------------------------------------
def _settled(n_scenes=S2, frames=4, depth=64, **cfg):
    """A context whose scenes hold tracks that stay (lifetimes of 100 s), stance enabled behind them."""
    return settled(lambda sb, data: StanceRun(sb, depth, data), n_scenes, frames, long_lived=True, **cfg)


def _rules(n, **over):
    from mmwave_msc_amd import _lib
    out = []
    for s in range(n):
        r = dict(zip(_lib.STANCE_FIELDS, RULE), id=40 + s)
        r.update({k: (v[s] if isinstance(v, (list, tuple)) else v) for k, v in over.items()})
        out.append([r])
    return out


def test_heads_at_every_boundary_and_one_ulp_above_from_every_old_class():
    """Scene k of 0 .. 3 is driven to old class k (0: a NaN head leaves it UNKNOWN), scene 4 to LOW; then every live track gets the
    same head.  `above` is strict: a head exactly on the boundary that counts for the old class is not above it, the next fp32 is."""
    run = _settled()
    drive = [np.nan, U, M, L, M]
    t = 0.0
    classes = {}
    for head in (UP_LO, UP_HI, LIE_LO, LIE_HI, H_STAND, H_LIE):
        for h in (F32(head), _up(head)):
            run.set_rules(_rules(S2))                       # every slot void again: old = UNKNOWN where nothing is driven
            run.plant_heads(drive)
            run.sample(t=t)
            run.plant_heads([h] * S2)
            run.sample(t=t + 1.0)                           # (far beyond fall_window: no FALL here)
            t += 2.0
            run.compare(("boundary", head, float(h)))
            ntr, trk = run.sb.num_tracks(), run.sb.tracks()
            classes[(head, bool(h > F32(head)))] = [run.ref.cls(s, int(trk[s, 0]["uid"])) for s in range(S2)]
    # by hand, [old UNKNOWN, UPRIGHT, LOW, LYING, LOW]: exactly on the boundary, then one ulp above
    want = {
        (UP_LO, False): [LOW, LOW, LOW, LOW, LOW], (UP_LO, True): [LOW, UPRIGHT, LOW, LOW, LOW],
        (UP_HI, False): [UPRIGHT, UPRIGHT, LOW, LOW, LOW], (UP_HI, True): [UPRIGHT, UPRIGHT, UPRIGHT, UPRIGHT, UPRIGHT],
        (LIE_LO, False): [LYING, LYING, LYING, LYING, LYING], (LIE_LO, True): [LYING, LOW, LOW, LYING, LOW],
        (LIE_HI, False): [LOW, LOW, LOW, LYING, LOW], (LIE_HI, True): [LOW, LOW, LOW, LOW, LOW],
        (H_STAND, False): [LOW, UPRIGHT, LOW, LOW, LOW], (H_STAND, True): [UPRIGHT, UPRIGHT, LOW, LOW, LOW],
        (H_LIE, False): [LYING, LOW, LOW, LYING, LOW], (H_LIE, True): [LOW, LOW, LOW, LYING, LOW],
    }
    assert classes == want, classes
    run.sb.check()
    run.sb.close()


def test_signed_zero_non_finite_heads_and_the_gap_at_its_bound():
    from mmwave_msc_amd import _lib
    run = _settled()
    run.set_rules(_rules(S2, long_lie=float("inf")))
    run.plant_heads([U, U, M, L, U])
    run.sample(t=0.0)
    # -0.0 is a height like any other (LYING); +inf and NaN are not plausible: the class stays; scene 4: s = 0.25 exactly is plausible
    run.plant_heads([-0.0, np.inf, np.nan, -np.inf, L], g=[0.0, 0.0, 0.0, 0.0, 0.5])
    run.sample(t=8.0)
    rows, events = run.compare("non-finite")
    ntr, trk = run.sb.num_tracks(), run.sb.tracks()
    assert [run.ref.cls(s, int(trk[s, 0]["uid"])) for s in range(S2)] == [LYING, UPRIGHT, LOW, LYING, LYING]
    assert set((events["scene"][events["t"] == 8.0] - BASE).tolist()) == {0, 4}
    assert run.ref.tally["implausible_head"] == int(ntr[1] + ntr[2] + ntr[3])
    # ... and the next fp32 above 0.5 is not: nothing of scene 4 changes, whatever the head says
    run.plant_heads([None, None, None, None, U], g=[0.0, 0.0, 0.0, 0.0, _up(0.5)])
    run.sample(t=16.0)
    rows, events = run.compare("gap")
    assert len(events) == 0 and run.ref.tally["implausible_gap"] == int(ntr[4])
    # a NaN s is plausible, as `nan > 0.5` is false
    run.plant_heads([None, None, None, None, U], g=[0.0, 0.0, 0.0, 0.0, np.nan])
    run.sample(t=24.0)
    rows, events = run.compare("nan gap")
    assert len(events) == int(ntr[4]) and (events["to"] == UPRIGHT).all() and (events["kind"] == _lib.SEV_CHANGE).all()
    run.sb.check()
    run.sb.close()


def test_fall_window_at_its_bound_and_long_lie_zero_and_never():
    from mmwave_msc_amd import _lib
    run = _settled()
    # scenes 0, 1: the window; 2: long_lie = 0; 3: long_lie = +inf; 4: long_lie = 0.5
    run.set_rules(_rules(S2, long_lie=[30.0, 30.0, 0.0, float("inf"), 0.5]))
    run.plant_heads([U] * S2)
    run.sample(t=1.0)
    run.compare("upright")
    run.plant_heads([L] * S2)
    run.sample(t=[1.25, 1.25 + 2.0 ** -50, 1.25, 1.25, 1.25])          # tt - t_upright == fall_window: FALL; the next step beyond: CHANGE
    rows, events = run.compare("window")
    ntr = run.sb.num_tracks()
    kinds = {s: events["kind"][events["scene"] == BASE + s].tolist() for s in range(S2)}
    assert kinds[0] == [_lib.SEV_FALL] * int(ntr[0]) and kinds[1] == [_lib.SEV_CHANGE] * int(ntr[1])
    assert kinds[2] == [_lib.SEV_FALL, _lib.SEV_LONG_LIE] * int(ntr[2])   # long_lie == 0: both in one sample, in that order, track by track
    assert kinds[3] == [_lib.SEV_FALL] * int(ntr[3]) and kinds[4] == [_lib.SEV_FALL] * int(ntr[4])
    assert rows["falls"].tolist() == [int(ntr[0]), 0, int(ntr[2]), int(ntr[3]), int(ntr[4])] and rows["long_lies"].tolist() == [0, 0, int(ntr[2]), 0, 0]
    # a second sample without a step changes only the ordinal -- and gives the LONG_LIE that is due (scene 4), once
    run.sample(t=1.75)
    rows, events = run.compare("due")
    assert events["kind"].tolist() == [_lib.SEV_LONG_LIE] * int(ntr[4]) and (events["scene"] == BASE + 4).all()
    run.sample(t=1e300)
    rows, events = run.compare("never")
    assert events["kind"].tolist() == [_lib.SEV_LONG_LIE] * int(ntr[0] + ntr[1]) and rows["long_lies"].tolist() == [int(n) for n in (ntr[0], ntr[1], ntr[2], 0, ntr[4])]
    assert rows["d_long_lies"].tolist() == [int(ntr[0]), int(ntr[1]), 0, 0, 0]
    run.sb.check()
    run.sb.close()


def test_log_depth_2_capacity_subsets_and_ordinals():
    from mmwave_msc_amd import _lib
    run = _settled(depth=2)
    sb, ref = run.sb, run.ref
    # REBASED, FALL-less CHANGE and LONG_LIE of every track in ONE call: more than the log holds -- the newest two stay, the counters are exact
    run.set_rules(_rules(S2, long_lie=0.0))
    run.plant_heads([L] * S2)
    run.sample(t=None)                                       # t = the call ordinal 0
    ntr = sb.num_tracks()
    want_rows, want_events = ref.peek(BASE)
    assert want_rows["lost"].tolist() == [1 + 2 * int(n) - 2 for n in ntr] and len(want_events) == 2 * S2
    assert want_rows["long_lies"].tolist() == [int(n) for n in ntr] and (want_events["t"] == 0.0).all()
    # MMW_E_CAPACITY with both counts; nothing is written, nothing is taken
    b_r, b_e = sb.alloc(S2 * 48), sb.alloc(2 * S2 * 32)
    sent = np.full(2 * S2 * 32, 0x5A, np.uint8)
    b_e.upload(sent)
    for caps in ((S2, 2 * S2 - 1), (S2 - 1, 2 * S2)):
        sb.stance_async(b_r.ptr, caps[0], b_e.ptr, caps[1], BASE, 1)
        with pytest.raises(_lib.MmwError) as ei:
            sb.stance_wait(1)
        assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (S2, 2 * S2)
        assert b_e.download((2 * S2 * 32,), np.uint8).tobytes() == sent.tobytes()
    sb.stance_async(b_r.ptr, S2, b_e.ptr, 2 * S2, BASE, 2)
    assert sb.stance_wait(2) == (S2, 2 * S2)
    same_pair((b_r.download((S2,), _lib.STANCE_ROW_DTYPE), b_e.download((2 * S2,), _lib.STANCE_EVENT_DTYPE)), ref.export(BASE), "retry")
    for b in (b_r, b_e):
        b.free()
    # a subset of the scenes, t = None: the asked scenes' ordinals move (1), the others' do not
    run.plant_heads([U] * S2)
    run.sample(t=None, scenes=[1, 3])
    rows, events = run.compare("subset")
    assert set((events["scene"] - BASE).tolist()) == {1, 3} and (events["t"] == 1.0).all()
    run.sample(t=None)
    rows, events = run.compare("all")
    assert sorted(set(zip((events["scene"] - BASE).tolist(), events["t"].tolist()))) == [(0, 1.0), (2, 1.0), (4, 1.0)]
    assert ref.ordinal.tolist() == [2, 3, 2, 3, 2]
    # depth outside 0 .. STANCE_LOG_MAX is refused and changes nothing; 0 frees, and then every call but the getter is refused
    for bad in (-1, _lib.STANCE_LOG_MAX + 1):
        with pytest.raises(_lib.MmwError) as ei:
            sb.enable_stance(bad)
        assert ei.value.code == _lib.E_ARG
    run.sample(t=None)
    run.compare("still there")
    sb.enable_stance(0)
    with pytest.raises(_lib.MmwError):
        sb.sample_stance()
    assert not sb.stance_rules()[0].any()
    sb.enable_stance(_lib.STANCE_LOG_MAX)
    sb.check()
    sb.close()


def test_refused_rules_change_nothing():
    from mmwave_msc_amd import _lib
    run = _settled()
    run.set_rules(_rules(S2))
    before = run.sb.stance_rules()
    inf, nan = float("inf"), float("nan")
    bad = [dict(h_stand=inf), dict(h_lie=nan), dict(margin=inf), dict(margin=-0.125), dict(fall_window=-1.0), dict(fall_window=inf), dict(long_lie=-1.0),
           dict(long_lie=nan), dict(long_lie=-inf), dict(max_gap=0.0), dict(max_gap=-0.5), dict(max_gap=inf), dict(h_stand=0.75), dict(margin=0.375)]
    for over in bad:                                         # (h_stand 0.75: lie_hi == up_lo; margin 0.375: lie_hi 0.875 == up_lo)
        with pytest.raises(_lib.MmwError) as ei:
            run.sb.set_stance_rules(_rules(S2)[:2] + _rules(1, **over), scenes=[3, 1, 0])
        assert ei.value.code == _lib.E_ARG, over
    nr, rt = _lib.make_stance_rules(_rules(1))
    rt[0, 0]["reserved_"] = 1
    with pytest.raises(_lib.MmwError):
        run.sb.set_stance_rules((nr, rt))
    with pytest.raises(_lib.MmwError):
        run.sb.set_stance_rules((np.array([2], np.int32), rt))
    after = run.sb.stance_rules()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and after[0].tolist() == [1] * S2
    run.plant_heads([U] * S2)
    run.sample(t=0.0)
    rows, events = run.compare("one REBASED only")           # (of the accepted set call; the refused ones bumped nothing)
    assert n_kind(events, _lib.SEV_REBASED) == S2
    run.sb.check()
    run.sb.close()


def test_reset_restore_and_set_rules_rebase_their_scenes_only():
    from mmwave_msc_amd import _lib
    run = _settled()
    sb, ref = run.sb, run.ref
    run.set_rules(_rules(S2, long_lie=float("inf")))
    run.plant_heads([U, M, L, U, M])
    run.sample(t=0.0)
    rows, events = run.compare("first")
    assert n_kind(events, _lib.SEV_REBASED) == S2
    blob = sb.snapshot()
    # a set call on scene 2 alone: its counters restart and it is REBASED; the neighbours keep their classes (no event for them)
    run.set_rules(_rules(1, id=99, long_lie=float("inf")), scenes=[2])
    assert ref.peek()[0]["unknown"][2] == 0 and ref.peek()[0]["lying"][2] == 0          # rebased and not yet sampled: all four are 0
    run.compare("set, before the sample")
    run.sample(t=1.0)
    rows, events = run.compare("set")
    assert (events["scene"] == BASE + 2).all() and events["kind"][0] == _lib.SEV_REBASED and rows["id"].tolist() == [40, 41, 99, 43, 44]
    # reset_scenes: scenes 0 and 3 are empty and REBASED (slot = 0 live tracks), nobody else
    sb.reset_scenes(np.isin(np.arange(S2), (0, 3)))
    ref.rebase([0, 3])
    run.sample(t=2.0)
    rows, events = run.compare("reset_scenes")
    assert sorted((events["scene"] - BASE).tolist()) == [0, 3] and (events["kind"] == _lib.SEV_REBASED).all() and (events["slot"] == 0).all()
    assert rows["upright"][0] == 0 and rows["upright"][3] == 0
    # restore: every scene of the blob, their tracks are back with the keypoints they had
    sb.restore(blob)
    ref.rebase()
    run.sample(t=3.0)
    rows, events = run.compare("restore")
    assert n_kind(events, _lib.SEV_REBASED) == S2 and n_kind(events, _lib.SEV_CHANGE) == int(sb.num_tracks().sum())
    assert rows["falls"].tolist() == [0] * S2                # the first classification behind a REBASED is never a FALL
    sb.reset()
    ref.rebase()
    run.sample(t=4.0)
    rows, events = run.compare("reset")
    assert events["kind"].tolist() == [_lib.SEV_REBASED] * S2 and rows["unknown"].tolist() == [0] * S2
    sb.check()
    sb.close()


def test_one_scene_with_64_tracks_every_lane_a_track_and_a_slot():
    """track_cap = 64 and a scene of 64 live tracks, planted through a snapshot blob: the section of a real scene with its first record
    repeated 64 times under uids 63 .. 0 and no ring rows (tests/_snap_plant.py has the offsets)."""
    from mmwave_msc_amd import _lib
    from tests._snap_plant import plant_tracks
    from mmwave_msc_amd.batch import SceneBatch
    sb = SceneBatch(_lib.default_config(tr_max_tracks=64, db_min_samples=12, track_cap=64, tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0), 2, N)
    assert sb.track_cap == 64
    pts, cnt, dts = cut(2)
    for f in range(4):
        sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])
    assert (sb.num_tracks() >= 1).all()
    plant_tracks(sb, 0, list(range(63, -1, -1)))
    assert sb.num_tracks()[0] == 64 and sb.tracks()[0]["uid"].tolist() == list(range(63, -1, -1))
    sb.enable_stance(256)
    ref = StanceRef(2, 64, 256)
    nr, rt = _lib.make_stance_rules(_rules(2, long_lie=0.125))
    sb.set_stance_rules((nr, rt))
    ref.set_rules([0, 1], nr, rt)
    heads = (U, M, L, 1.1875, 0.5625, np.nan)
    for k in range(4):
        trk = sb.tracks()
        own = np.array([(0, j) for j in range(64)], np.int32)
        sb.set_keypoints_host(np.stack([_kp(heads[(j * 5 + k * (1 + j % 3)) % len(heads)], 0.75 if (j + k) % 11 == 0 else 0.0) for j in range(64)]), own)
        sb.sample_stance(t=0.125 * k)
        ref.sample(sb.tracks(), sb.num_tracks(), t=np.full(2, 0.125 * k))
        rows, events = sb.stance_host(scene_base=BASE)
        same_pair((rows, events), ref.export(BASE), ("64", k))
        assert int(rows["upright"][0] + rows["low"][0] + rows["lying"][0] + rows["unknown"][0]) == 64
    assert ref.falls[0] >= 1 and ref.long_lies[0] >= 1 and ref.tally["implausible_gap"] >= 1 and ref.tally["implausible_head"] >= 1, sorted(ref.tally.items())
    sb.check()
    sb.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_sampled_behind_the_cnn_without_a_host_wait():
    """estimate_posture() then sample_stance(): the sampler's kernel is queued on the context's stream behind the chain's keypoint
    scatter (launch_set_kp in api_posture.hip), so what it classes is what `tracks()` shows afterwards.  The heights of a random
    model are anything; the rule is wide enough to see all three classes over 24 scenes."""
    from tests import _posture_cabi as pc
    from tests._posture_gpu import KW, _weights
    from mmwave_msc_amd import _lib
    n = 24
    sb = make_checked(n, pc.N_PTS, "per_scene", **KW[3])
    pts, cnt, dts = pc.scenario(n)
    sb.attach_posture_batch(_weights(0, 3), n * sb.track_cap)
    sb.enable_stance(64)
    ref = StanceRef(n, sb.track_cap, 64)
    est = 0
    for f in range(8):
        sb.step_host(pts[f], cnt[f], dts[f])
        if f == 3:                                           # the rule sits at the heads the model gives: the median and the lower quartile
            sb.estimate_posture()
            ntr, trk = sb.num_tracks(), sb.tracks()
            heads = np.array([float(trk[s, j]["keypoints"][HEAD]) for s in range(n) for j in range(int(ntr[s]))])
            heads = heads[np.isfinite(heads)]
            assert len(heads) >= 8
            hs, hl = float(np.float32(np.median(heads))), float(np.float32(np.quantile(heads, 0.25)))
            margin = (hs - hl) / 8.0
            assert margin > 0.0
            nr, rt = _lib.make_stance_rules([[dict(h_stand=hs, h_lie=hl, margin=margin, fall_window=0.5, long_lie=0.25, max_gap=1e6, id=s)] for s in range(n)])
            sb.set_stance_rules((nr, rt))
            ref.set_rules(range(n), nr, rt)
        if f >= 3:
            est += sb.estimate_posture()                     # (waits for the row count only: the chain is still queued)
            sb.sample_stance(t=0.125 * f)
            ref.sample(sb.tracks(), sb.num_tracks(), t=np.full(n, 0.125 * f))
            same_pair(sb.stance_host(scene_base=BASE), ref.export(BASE), ("cnn", f))
    assert est >= n and ref.logged.sum() > n
    got = {k for k in ref.tally if k.startswith("first_")}
    assert len(got) >= 2, sorted(ref.tally.items())
    sb.check()
    sb.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    from mmwave_msc_amd import _lib
    a = make_checked(S, N, "per_scene", **CFG_KW)
    b = make_checked(S, N, "per_scene", **CFG_KW)
    for sb in (a, b):
        sb.enable_report()
    # before enable_stance every stance call is refused, and the getter reports no rule
    buf = a.alloc(64)
    for call in (lambda: a.set_stance_rules([[RULE]]), lambda: a.sample_stance(), lambda: a.sample_stance_dev(None, None),
                 lambda: a.stance_async(buf.ptr, 1, buf.ptr, 1), lambda: a.stance_wait(0), lambda: a.stance_host()):
        with pytest.raises(_lib.MmwError) as ei:
            call()
        assert ei.value.code == _lib.E_ARG
    buf.free()
    nr, rt = a.stance_rules()
    assert nr.tolist() == [0] * S and rt.tobytes() == bytes(S * 64)
    run = StanceRun(a, 64)
    run.set_rules([[RULE]] * S)

    def plant(sb, f):
        ntr, trk = sb.num_tracks(), sb.tracks()
        own = [(s, j) for s in range(S) for j in range(int(ntr[s]))]
        if own:
            sb.set_keypoints_host(np.stack([planted(s, int(trk[s, j]["uid"]), f) for s, j in own]), np.array(own, np.int32))

    def drive(f):
        run.sample(t=0.125 * f)
        if f % 4 == 3:
            run.compare(("moves", f))

    nothing_else_moves(a, b, scenario(), F, drive, both=plant, at_end=TRACKS + REPORT)
    for sb in (a, b):
        sb.check()
        sb.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_trails_tripwires_and_stance_keep_separate_slot_tables_and_generations():
    from mmwave_msc_amd import _lib
    S6 = 6
    sb = make_checked(S6, N, "per_scene", **CFG_KW)
    data = cut(S6)
    run = StanceRun(sb, 64, data)
    sb.enable_trails(8)
    trip = TripRun(sb, 64, data)
    trip.set_wires(wires16(S6))
    run.set_rules([[RULE]] * S6)

    for f in range(F):
        run.step(f)
        run.plant(lambda s, j, uid: planted(s, uid, f))
        if f % 2 == 0:                                       # the three are sampled at different times: their slot tables drift apart
            sb.sample_trails(t=0.125 * f)
        if f % 3 != 1:
            trip.sample(t=0.125 * f)
        run.sample(t=0.125 * f)
        run.compare(("stance", f))
        trip.compare(("trip", f))
        if f == 5:                                           # a rule set call: a REBASED for stance alone
            run.set_rules([[RULE + (9,)]] * 2, scenes=[1, 4])
            run.sample(t=0.125 * f + 0.0625)
            trip.sample(t=0.125 * f + 0.0625)
            _, ev = run.compare("stance set")
            assert sorted((ev["scene"][ev["kind"] == _lib.SEV_REBASED] - BASE).tolist()) == [1, 4]
            assert n_kind(trip.compare("trip after stance set")[1], _lib.TW_REBASED) == 0
        if f == 8:                                           # reset_scenes: one REBASED each
            sb.reset_scenes(np.isin(np.arange(S6), (2,)))
            run.ref.rebase([2]); trip.ref.rebase([2])
            run.sample(t=0.125 * f + 0.0625)
            trip.sample(t=0.125 * f + 0.0625)
            _, ev = run.compare("stance reset")
            assert (ev["scene"][ev["kind"] == _lib.SEV_REBASED] - BASE).tolist() == [2]
            tw = trip.compare("trip reset")[1]
            assert (tw["scene"][tw["kind"] == _lib.TW_REBASED] - BASE).tolist() == [2]
    d, p = sb.trails_host()
    ntr = sb.num_tracks()
    assert len(d) == int(ntr.sum())
    sb.check()
    sb.close()


def test_tripwire_log_of_depth_3_and_stance_log_of_depth_5_in_one_context():
    """Both event logs in one context of three scenes, at depths that are odd, differ and are no power of two, so a swapped depth or
    ring shows: tripwires at 3, stance at 5; scene 1 has neither wires nor a rule.  Track 0 of scenes 0 and 2 is planted half a metre
    in front of five parallel wires one metre apart with a velocity of one metre per second, so an empty frame whose predict multiplier
    is five crosses five wires in ONE sample call (more than the log holds) and multipliers of two cross two; every live track's head is planted LYING and UPRIGHT
    in turn under a rule with long_lie 0, so a call logs CHANGE and LONG_LIE of three tracks (six events, more than the log holds)
    or three CHANGEs.  The two consumers export at different frames, with more than two turns of their ring in between, and one stance
    export is first asked with one event too few.  Rows, events and `lost` are the reference model's, byte for byte."""
    from mmwave_msc_amd import _lib
    S3 = 3
    kw = {k: v for k, v in CFG_KW.items() if k != "tr_max_tracks"}     # (the default track cap)
    sb = make_checked(S3, N, "per_scene", **dict(kw, tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0, kf_q_std=0.0))
    data = cut(S3)
    for f in range(9):                                       # (the C oracle: three tracks in each of the three scenes from frame 8 on)
        sb.step_host(data[0][f].astype(np.float64), data[1][f], data[2][f])
    assert sb.num_tracks().tolist() == [3, 3, 3]
    blob = bytearray(sb.snapshot())
    ents = directory(blob)
    for sc in (0, 2):
        plant_state(blob, record_at(ents, sc), [FAR - 0.5, 0.0, 1.0, 1.0, 0.0, 0.0])
    sb.restore(bytes(blob))
    run = StanceRun(sb, 5, data)                             # stance, log depth 5
    trip = TripRun(sb, 3, data)
    trip.set_wires([[(FAR + k, -4.0, FAR + k, 4.0, 0.0, 60 + k) for k in range(5)]] * 2, scenes=[0, 2])
    run.set_rules(_rules(2, long_lie=0.0), scenes=[0, 2])

    def frame(k, at, head):
        """Move the planted tracks to FAR - 0.5 + at, plant every head, sample both consumers at t = k."""
        if k:                                                # (an empty frame moves a track by velocity x the running sum of dt: that sum becomes the move)
            mult = float(at - frame.at)
            step_empty(sb, mult - frame.mult)
            frame.mult = mult
        frame.at = at
        assert [float(sb.tracks()["x"][sc, 0, 0]) for sc in (0, 2)] == [FAR - 0.5 + at] * 2
        run.plant_heads([head] * S3)
        run.sample(t=float(k))
        trip.sample(t=float(k))

    frame.mult = 0.0
    frame(0, 0, L)                                           # stance: REBASED, 3 CHANGE, 3 LONG_LIE in one call -- 7 > 5; tripwires: REBASED
    assert run.ref.logged.tolist() == [7, 0, 7] and trip.ref.logged.tolist() == [1, 0, 1]
    rows, events = run.compare("stance at 0")
    assert rows["lost"].tolist() == [2, 2] and len(events) == 10 and n_kind(events, _lib.SEV_REBASED) == 0
    frame(1, 5, U)                                           # tripwires: five wires in one call -- 5 > 3
    assert trip.ref.logged.tolist() == [6, 0, 6]
    rows, events = trip.compare("tripwires at 1")
    assert rows["lost"].tolist() == [3] * 10 and rows["backward"].tolist() == [1] * 10
    assert [(int(e["scene"]) - BASE, int(e["wire"])) for e in events] == [(0, 2), (0, 3), (0, 4), (2, 2), (2, 3), (2, 4)]
    frame(2, 3, L)
    frame(3, 5, U)                                           # stance since its export: 3 + 6 + 3 events, the ring of 5 turned twice
    assert run.ref.logged.tolist() == [19, 0, 19]
    # one event too few: MMW_E_CAPACITY with both counts, nothing is written, nothing is taken
    b_r, b_e = sb.alloc(2 * 48), sb.alloc(10 * 32)
    sent = np.full(10 * 32, 0x5A, np.uint8)
    b_e.upload(sent)
    sb.stance_async(b_r.ptr, 2, b_e.ptr, 9, BASE, 1)
    with pytest.raises(_lib.MmwError) as ei:
        sb.stance_wait(1)
    assert ei.value.code == _lib.E_CAPACITY and ei.value.needed == (2, 10)
    assert b_e.download((10 * 32,), np.uint8).tobytes() == sent.tobytes()
    for b in (b_r, b_e):
        b.free()
    rows, events = run.compare("stance at 3")
    assert rows["lost"].tolist() == [7, 7] and len(events) == 10
    frame(4, 3, L)
    frame(5, 5, U)                                           # tripwires since their export: 4 x 2 events, the ring of 3 turned twice
    assert trip.ref.logged.tolist() == [14, 0, 14]
    rows, events = trip.compare("tripwires at 5")
    assert rows["lost"].tolist() == [5] * 10 and len(events) == 6
    assert rows["forward"].tolist() == [0, 0, 0, 2, 2] * 2 and rows["backward"].tolist() == [1, 1, 1, 3, 3] * 2
    frame(6, 3, L)
    rows, events = run.compare("stance at 6")
    assert rows["lost"].tolist() == [10, 10] and len(events) == 10
    rows, events = trip.compare("tripwires at 6")
    assert not rows["lost"].any() and [int(e["wire"]) for e in events] == [3, 4, 3, 4]
    sb.check()
    sb.close()
