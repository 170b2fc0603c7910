"""The generation bump that the live-track report, the zones and the trails share (k_uid_rebase, one launch behind mmw_reset /
mmw_reset_scenes / mmw_restore for whichever of the three is on) on the GPU.

259 scenes x 32 points, TR_MAX_TRACKS 4; the touched scenes are {0, 255, 256, 258}: the first and the last thread of the bump
kernel's first 256-thread workgroup, and a second workgroup of three threads.  Every on/off combination of {report, zones, trails}
runs the same sequence in a context of its own -- reset_scenes, restore of a snapshot into the same scenes, reset -- and after each
every consumer that is on must say exactly what its restatement says: the report test's host-side event list, tests/_zone_ref.py,
tests/_trail_ref.py.  With all three on, mmw_set_zones for one scene must void the zones' memberships of that scene and nothing of
the other two consumers."""
import functools
import itertools

import numpy as np
import pytest

from tests._feature_run import export_and_compare, same_trails
from tests._report_scenes import CFG_KW, as_tuples, host_events, strips, uid_lists
from tests._trail_ref import TrailRef
from tests._zone_ref import ZoneRef

pytestmark = pytest.mark.gpu

SN, NP, FR = 259, 32, 8
TOUCHED = (0, 255, 256, 258)
DEPTH = 4


@functools.lru_cache(maxsize=None)
def _data():
    """(pts[FR, SN, NP, 8] float32, cnt[FR, SN] int32, dt[FR, SN] float64): one walking target per scene, in view throughout; read-only."""
    from mmwave_msc_amd.synth import make_scene
    pts = np.zeros((FR, SN, NP, 8), np.float32)
    cnt = np.zeros((FR, SN), np.int32)
    dts = np.zeros((FR, SN))
    for s in range(SN):
        pts[:, s], cnt[:, s], dts[:, s] = make_scene(8100 + s, FR, NP, 1)
    for a in (pts, cnt, dts):
        a.setflags(write=False)
    return pts, cnt, dts


class _Ctx:
    """A context with the consumers asked for, and the restatement of each."""

    def __init__(self, report, zones, trails):
        from mmwave_msc_amd import _lib
        from mmwave_msc_amd.batch import SceneBatch
        self.sb = SceneBatch(_lib.default_config(**CFG_KW), SN, NP)
        assert self.sb.cfg.tr_max_tracks == 4
        self.report, self.zones, self.trails = report, zones, trails
        self.frame = 0
        self.prev = None
        self.zref = self.tref = None
        if report:
            self.sb.enable_report()
        if zones:
            nz, zt = strips(SN)
            self.sb.set_zones((nz, zt))
            self.zref = ZoneRef(SN)
            self.zref.set_zones(nz, zt)
        if trails:
            self.sb.enable_trails(DEPTH)
            self.tref = TrailRef(SN, self.sb.track_cap, DEPTH)

    def step(self):
        pts, cnt, dts = _data()
        self.sb.step_host(pts[self.frame].astype(np.float64), cnt[self.frame], dts[self.frame])
        self.frame += 1

    def rebase(self, scenes):
        for ref in (self.zref, self.tref):
            if ref is not None:
                ref.rebase(scenes)

    def sample_and_export(self, ctx, rebased=()):
        """Sample the trails, export everything that is on, compare each with its restatement; `rebased`: the scenes whose uids
        restarted since the previous export.  -> (report events, zone events, trail directory), None for what is off."""
        from mmwave_msc_amd import _lib
        sb = self.sb
        out = [None, None, None]
        if self.trails:
            t = np.full(SN, float(self.frame))
            sb.sample_trails(t=t)
            self.tref.sample(sb.tracks(), sb.num_tracks(), t=t)
            got = sb.trails_host()
            same_trails(got, self.tref.export(sb.tracks(), sb.num_tracks()), (ctx, "trails"))
            out[2] = got[0]
        if self.report:
            rows, events = sb.report_host()
            cur = uid_lists(sb)
            assert len(rows) == sum(len(c) for c in cur), ctx
            if self.prev is not None:
                assert as_tuples(events) == host_events(self.prev, cur, rebased=rebased), (ctx, "report")
            assert sorted(int(e["scene"]) for e in events if e["kind"] == _lib.EV_REBASED) == sorted(rebased), (ctx, "report REBASED")
            self.prev = cur
            out[0] = events
        if self.zones:
            _, events = export_and_compare(sb, self.zref, (ctx, "zones"), scene_base=0)
            assert sorted(int(e["scene"]) for e in events if e["kind"] == _lib.ZEV_REBASED) == sorted(rebased), (ctx, "zones REBASED")
            out[1] = events
        return out


def _totals(d):
    return {(int(e["scene"]), int(e["uid"])): int(e["total"]) for e in d}


@pytest.mark.parametrize("report,zones,trails", list(itertools.product((False, True), repeat=3)),
                         ids=lambda v: "on" if v else "off")
def test_one_bump_serves_the_consumers_that_are_on(report, zones, trails):
    c = _Ctx(report, zones, trails)
    sb = c.sb
    for _ in range(3):
        c.step()
    assert int(sb.num_tracks().min()) >= 1, "every scene holds a track"
    # the first exports, so that baselines exist: the report's says BORN for everything live (it was enabled on an empty context),
    # the zones' REBASED for every scene (mmw_set_zones voided all it listed) and ENTER for the tracks that stand inside a zone
    if report:
        sb.report_host()
        c.prev = uid_lists(sb)
    if zones:
        _, events = export_and_compare(sb, c.zref, "first zones", scene_base=0)
        assert len(events) > SN, "memberships exist"
    first = c.sample_and_export("baselines")

    def flagged_scenes(how):
        if how == "reset_scenes":
            sb.reset_scenes(np.isin(np.arange(SN), TOUCHED))
            assert not sb.num_tracks()[list(TOUCHED)].any() and int(sb.num_tracks().sum()) >= SN - len(TOUCHED)
            return TOUCHED
        if how == "restore":
            sb.restore(sb.snapshot(list(TOUCHED)), scenes=list(TOUCHED))
            return TOUCHED
        sb.reset()
        assert not sb.num_tracks().any()
        return tuple(range(SN))

    before = first[2]
    for how in ("reset_scenes", "restore", "reset"):
        touched = flagged_scenes(how)
        c.rebase(touched)
        c.step()
        _, _, d = c.sample_and_export(how, rebased=touched)
        if trails:
            hit = np.isin(d["scene"], touched)
            assert hit.any() and (d["total"][hit] == 1).all() and not d["travelled"][hit].any(), how
            was, now = _totals(before[~np.isin(before["scene"], touched)]), _totals(d[~hit])
            kept = set(was) & set(now)
            assert all(now[k] == was[k] + 1 for k in kept) and (how == "reset" or len(kept) >= SN // 2), how
            before = d
    sb.check()

    if report and zones and trails:
        # mmw_set_zones for scene 7 alone: the zones' word of scene 7, and no other word of anybody
        c.step()
        _, _, before = c.sample_and_export("settled")
        nz, zt = strips(SN, margin=0.125)
        sb.set_zones((nz[7:8], zt[7:8]), scenes=[7])
        c.zref.set_zones(nz[7:8], zt[7:8], scenes=[7])
        c.step()
        sb.sample_trails(t=np.full(SN, float(c.frame)))
        c.tref.sample(sb.tracks(), sb.num_tracks(), t=np.full(SN, float(c.frame)))
        d, p = sb.trails_host()
        same_trails((d, p), c.tref.export(sb.tracks(), sb.num_tracks()), "set_zones: trails")
        was, now = _totals(before[before["scene"] == 7]), _totals(d[d["scene"] == 7])
        assert was and set(was) <= set(now) and all(now[k] == was[k] + 1 for k in was), (was, now)   # scene 7's trails go on
        from mmwave_msc_amd import _lib
        _, events = sb.report_host()
        cur = uid_lists(sb)
        assert as_tuples(events) == host_events(c.prev, cur) and not (events["kind"] == _lib.EV_REBASED).any()
        _, zev = export_and_compare(sb, c.zref, "set_zones: zones", scene_base=0)
        assert [int(e["scene"]) for e in zev if e["kind"] == _lib.ZEV_REBASED] == [7]
    sb.close()
