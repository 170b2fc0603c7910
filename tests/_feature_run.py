"""The scaffolding the uid-keyed exports' GPU suites share (zones, trails, tripwires, stance watch, heat maps): step a context on the
report scenario, sample the feature and its numpy restatement on the state read back, and compare the two exports by their bytes.
tests/test_feature_harness.py drives every adapter below against a stub context without a GPU.

Zones have no sample call and no adapter: `export_and_compare` is their whole harness, a thin function over `same_pair`."""
import numpy as np

from tests._heat_ref import HeatRef
from tests._report_scenes import CFG_KW, F, N, scenario
from tests._stance_ref import HEAD, NKP, StanceRef
from tests._trail_ref import TrailRef
from tests._tripwire_ref import TripRef

BASE = 7      # scene_base of the compared exports
S2 = 5        # a short last workgroup: one of four waves, one of one


def cut(n_scenes, n_frames=F):
    pts, cnt, dts = scenario()
    return pts[:n_frames, :n_scenes], cnt[:n_frames, :n_scenes], dts[:n_frames, :n_scenes]


def step(sb, f, data=None):
    pts, cnt, dts = data if data is not None else scenario()
    sb.step_host(pts[f].astype(np.float64), cnt[f], dts[f])


def step_empty(sb, dt):
    """A frame of no points in every scene: predict alone moves the tracks, by their velocity times (lifetime + dt)."""
    from mmwave_msc_amd import _lib
    n = sb.S
    sb.step_host(np.zeros((n, sb.max_pts, 8)), np.full(n, _lib.EMPTY_FRAME, np.int32), np.full(n, dt, np.float64), check=False)


def n_kind(events, kind):
    return int((events["kind"] == kind).sum())


def same_records(got, want, ctx, what="", skip=()):
    """The comparison rule: the same dtype, the same length, and every field but those in `skip` the same bytes."""
    assert got.dtype == want.dtype, (ctx, what, "dtype", got.dtype, want.dtype)
    assert len(got) == len(want), (ctx, what, "length", len(got), len(want), got.tolist(), want.tolist())
    for k in got.dtype.names:
        if k not in skip:
            assert got[k].tobytes() == want[k].tobytes(), (ctx, what, k, got[k].tolist(), want[k].tolist())


def same_pair(got, want, ctx, nouns=("rows", "events")):
    """... for both arrays of a two-buffer export."""
    for g, w, what in zip(got, want, nouns):
        same_records(g, w, ctx, what)


def same_trails(got, want, ctx):
    """(dir, points) pairs: everything by its bytes, `travelled` within total * 2^-52 * |want| of the restatement's and NaN where
    the restatement's is (tests/test_gpu_trails.py derives the bound); -> (bit-equal travelled values, all of them)."""
    (gd, gp), (wd, wp) = got, want
    same_records(gd, wd, ctx, "dir", skip=("travelled",))
    same_records(gp, wp, ctx, "points")
    g, w = gd["travelled"], wd["travelled"]
    assert np.array_equal(np.isnan(g), np.isnan(w)), (ctx, "travelled NaN", g.tolist(), w.tolist())
    ok = ~np.isnan(w)
    with np.errstate(invalid="ignore"):
        bound = wd["total"][ok] * 2.0 ** -52 * np.abs(w[ok])
        assert (np.abs(g[ok] - w[ok]) <= bound).all(), (ctx, "travelled", g.tolist(), w.tolist())
    return int((g.view(np.uint64) == w.view(np.uint64)).sum()), len(g)


def export_and_compare(sb, ref, ctx, scene_base=BASE):
    """One zone export of `sb` against the restatement (tests/_zone_ref.py) on the state read back; (rows, events)."""
    got = sb.zones_host(scene_base=scene_base)
    same_pair(got, ref.export(sb.tracks(), sb.num_tracks(), scene_base=scene_base), ctx)
    return got


class FeatureRun:
    """A context and its restatement, stepped, sampled and compared together.  A feature names what differs: the restatement class,
    the context's enable / sample / host-export methods, the nouns of its two arrays, and (sb setter, restatement setter, _lib
    maker) of its per-scene table; `want` where the restatement's export takes other arguments than (scene_base, **kw)."""
    Ref = enable = sampler = host = table = None
    nouns = ("rows", "events")

    def __init__(self, sb, size, data=None):
        self.sb, self.data = sb, data if data is not None else scenario()
        getattr(sb, self.enable)(size)
        self.ref = self.Ref(sb.S, sb.track_cap, size)

    def set_table(self, table, scenes=None):
        from mmwave_msc_amd import _lib
        sb_set, ref_set, make = self.table
        n, t = table if isinstance(table, tuple) else getattr(_lib, make)(table)
        getattr(self.sb, sb_set)((n, t), scenes=scenes)
        getattr(self.ref, ref_set)(list(range(len(n))) if scenes is None else list(scenes), n, t)

    def step(self, f):
        step(self.sb, f, self.data)

    def step_empty(self, dt):
        step_empty(self.sb, dt)

    def sample(self, t=None, scenes=None):
        getattr(self.sb, self.sampler)(t=t, scenes=scenes)
        flags = None
        if scenes is not None:
            flags = np.zeros(self.sb.S, np.int32)
            flags[list(scenes)] = 1
        t = None if t is None else np.broadcast_to(np.asarray(t, np.float64), (self.sb.S,))
        self.ref.sample(self.sb.tracks(), self.sb.num_tracks(), flags=flags, t=t)

    def want(self, scene_base, **kw):
        return self.ref.export(scene_base, **kw)

    def same(self, got, want, ctx):
        same_pair(got, want, ctx, self.nouns)

    def compare(self, ctx, scene_base=BASE, **kw):
        got = getattr(self.sb, self.host)(scene_base=scene_base, **kw)
        self.same(got, self.want(scene_base, **kw), ctx)
        return got


class TrailRun(FeatureRun):
    """compare(ctx, last=0): the restatement exports from the state read back, and `travelled` has its bound; the run counts how
    many of its values were bit-equal."""
    Ref, enable, sampler, host, nouns = TrailRef, "enable_trails", "sample_trails", "trails_host", ("dir", "points")
    equal = seen = 0

    def want(self, scene_base, **kw):
        return self.ref.export(self.sb.tracks(), self.sb.num_tracks(), scene_base=scene_base, **kw)

    def same(self, got, want, ctx):
        e, n = same_trails(got, want, ctx)
        self.equal, self.seen = self.equal + e, self.seen + n


class TripRun(FeatureRun):
    Ref, enable, sampler, host = TripRef, "enable_tripwires", "sample_tripwires", "tripwires_host"
    table = ("set_tripwires", "set_wires", "make_tripwires")
    set_wires = FeatureRun.set_table


class StanceRun(FeatureRun):
    Ref, enable, sampler, host = StanceRef, "enable_stance", "sample_stance", "stance_host"
    table = ("set_stance_rules", "set_rules", "make_stance_rules")
    set_rules = FeatureRun.set_table

    def plant(self, kp_of):
        """kp_of(scene, position, uid) -> the 57 keypoints of that live track, or None to leave them."""
        ntr, trk = self.sb.num_tracks(), self.sb.tracks()
        kps, own = [], []
        for s in range(self.sb.S):
            for j in range(int(ntr[s])):
                kp = kp_of(s, j, int(trk[s, j]["uid"]))
                if kp is not None:
                    kps.append(kp); own.append((s, j))
        if own:
            self.sb.set_keypoints_host(np.stack(kps), np.array(own, np.int32))

    def plant_heads(self, heads, g=None):
        """Every live track of scene s gets head heads[s] (None: left alone) and kp[1] = g[s]."""
        self.plant(lambda s, j, uid: None if heads[s] is None else head_kp(heads[s], 0.0 if g is None else g[s]))


def head_kp(head, g=0.0):
    """Keypoints that are zero but for the head height and kp[1]."""
    kp = np.zeros(NKP, np.float32)
    kp[HEAD], kp[1] = head, g
    return kp


class HeatRun(FeatureRun):
    """compare(ctx, scenes=None, clear=False)."""
    Ref, enable, sampler, host, nouns = HeatRef, "enable_heat", "sample_heat", "heat_host", ("rows", "cells")
    table = ("set_heat_grids", "set_grids", "make_heat_grids")
    set_grids = FeatureRun.set_table


def settled(make_run, n_scenes=S2, frames=4, long_lived=False, each_frame=None, **cfg):
    """make_run(sb, data) on a fresh context of the first `n_scenes` scenes, then `frames` frames with each_frame(run, f) behind each.
    `long_lived`: lifetimes of 100 s, so that every scene holds tracks that stay."""
    from tests._layouts import make_checked
    kw = dict(CFG_KW, **cfg)
    if long_lived:
        kw.update(tr_lifetime_dynamic=100.0, tr_lifetime_static=100.0)
    sb = make_checked(n_scenes, N, "per_scene", **kw)
    data = cut(n_scenes)
    run = make_run(sb, data)
    for f in range(frames):
        step(sb, f, data)
        if each_frame is not None:
            each_frame(run, f)
    if long_lived:
        assert (sb.num_tracks() >= 1).all()
    return run


def _bytes_of(x):
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return [_bytes_of(v) for v in x] if isinstance(x, (tuple, list)) else x


TRACKS = (lambda sb: sb.tracks(), lambda sb: sb.num_tracks())        # the witnesses every feature compares
REPORT = (lambda sb: sb.report_host(),)                              # (both contexts have the report enabled)


def nothing_else_moves(a, b, data, frames, drive, both=None, each_frame=(), at_end=TRACKS):
    """Two contexts on the same frames: behind each step `both(sb, f)` runs on either, then `drive(f)` drives the feature on `a`
    (and whatever the test does to both).  Every witness -- a function of a context that returns arrays, bytes or numbers, nested
    as it likes -- must say of `a` what it says of `b`, byte for byte: `each_frame` after every frame, `at_end` once."""
    def compare(witnesses, where):
        for k, w in enumerate(witnesses):
            assert _bytes_of(w(a)) == _bytes_of(w(b)), ("witness", k, where)
    for f in range(frames):
        for sb in (a, b):
            step(sb, f, data)
            if both is not None:
                both(sb, f)
        drive(f)
        compare(each_frame, f)
    compare(at_end, "end")
