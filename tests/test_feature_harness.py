"""The GPU suites' shared scaffolding (tests/_feature_run.py, tests/_snap_plant.py) without a GPU: the comparison rule refuses what
it must, every feature's adapter really runs its export through that rule -- driven against a stub context that hands back the
restatement's own export, intact or with one byte flipped --, and the blob edits land where the snapshot format says."""
import numpy as np
import pytest

from mmwave_msc_amd import _lib, snapshot
from mmwave_msc_amd.batch import TRACK_DTYPE
from tests import _snap_plant as sp
from tests._feature_run import BASE, FeatureRun, HeatRun, StanceRun, TrailRun, TripRun, export_and_compare, same_records
from tests._report_scenes import strips, wires16
from tests._zone_ref import ZoneRef
from tests.test_snapshot_format import SCENES, build_blob

REC = np.dtype([("n", "i4"), ("v", "f8")])


def _recs(*rows):
    return np.array(list(rows), REC)


# ---- same_records ------------------------------------------------------------------------------------------------------------
def test_same_records_accepts_equal_arrays_and_skipped_fields():
    a = _recs((1, 0.5), (2, np.nan))
    same_records(a, a.copy(), "ctx")
    same_records(a, _recs((1, 0.5), (2, 7.0)), "ctx", skip=("v",))


def _nan(payload):
    return np.array([0x7FF8000000000000 | payload], np.uint64).view(np.float64)[0]


@pytest.mark.parametrize("got,want,names", [
    (_recs((1, 0.5)), np.array([(1, 0.5)], np.dtype([("n", "i4"), ("v", "f4")])), ("dtype", "'v'")),     # (both dtypes are printed, fields by name)
    (_recs((1, 0.5)), _recs((1, 0.5), (2, 0.5)), ("length",)),
    (_recs((1, 0.5)), _recs((257, 0.5)), ("'n'",)),                                                      # one byte of one field
    (_recs((1, 0.0)), _recs((1, -0.0)), ("'v'",)),
    (_recs((1, _nan(1))), _recs((1, _nan(2))), ("'v'",)),
], ids=["dtype", "length", "one_byte", "signed_zero", "nan_payload"])
def test_same_records_refuses(got, want, names):
    with pytest.raises(AssertionError) as ei:
        same_records(got, want, "ctx", "what")
    for name in names + ("ctx", "what"):
        assert name in str(ei.value), str(ei.value)


# ---- every adapter is wired to it ----------------------------------------------------------------------------------------------
T_CAP = 4


class _Stub:
    """What an adapter needs of a context: 2 scenes of 3 live tracks each with distinct uids and positions, every enable / set / sample
    call accepted and recorded, and one `*_host` export that returns `export(**kw)`."""

    def __init__(self):
        self.S, self.track_cap, self.max_pts, self.calls = 2, T_CAP, 8, []
        self._tracks = np.zeros((2, T_CAP), TRACK_DTYPE)
        for s in range(2):
            for j in range(3):
                self._tracks[s, j]["uid"] = 10 * s + j + 1
                self._tracks[s, j]["x"][:3] = (0.3 * j - 0.2 + 0.05 * s, 1.0 + 0.5 * j, 1.0)     # inside a strip, a grid cell, a wire's span
                self._tracks[s, j]["keypoints"][22] = 1.5                                        # a head height (StanceRef's HEAD)

    def tracks(self):
        return self._tracks.copy()

    def num_tracks(self):
        return np.array([3, 3], np.int32)

    def move(self):
        self._tracks["x"][:, :, 0] += 0.125

    def __getattr__(self, name):
        if not name.startswith(("enable_", "set_", "sample_")):
            raise AttributeError(name)
        return lambda *a, **kw: self.calls.append((name, a, kw))


def _trails():
    sb = _Stub()
    run = TrailRun(sb, 4)
    run.sample(t=0.0)
    sb.move()
    run.sample(t=0.5)
    return run, lambda scene_base=0, **kw: run.ref.export(sb.tracks(), sb.num_tracks(), scene_base=scene_base, **kw)


def _tripwires():
    run = TripRun(_Stub(), 8)
    run.set_wires(wires16(2))
    run.sample(t=0.0)
    return run, lambda scene_base=0: run.ref.peek(scene_base)


def _stance():
    run = StanceRun(_Stub(), 8)
    run.set_rules([[(1.25, 0.5, 0.125, 0.25, 0.5, 0.5, 40 + s)] for s in range(2)])
    run.sample(t=0.0)
    return run, lambda scene_base=0: run.ref.peek(scene_base)


def _heat():
    run = HeatRun(_Stub(), 1024)
    run.set_grids([[dict(x0=-4.0, y0=0.0, cell=0.25, max_gap=1.0, nx=32, ny=32, id=s)] for s in range(2)])
    run.sample(t=0.0)
    return run, lambda scene_base=0, **kw: run.ref.export(scene_base, **kw)


class _ZoneRun:
    """Zones have no adapter: export_and_compare under the adapters' `compare` signature."""

    def __init__(self):
        self.sb, self.ref, self.host = _Stub(), ZoneRef(2), "zones_host"
        self.ref.set_zones(*strips(2))

    def compare(self, ctx, scene_base=BASE):
        return export_and_compare(self.sb, self.ref, ctx, scene_base)


def _zones():
    run = _ZoneRun()
    return run, lambda scene_base=0: run.ref.export(run.sb.tracks(), run.sb.num_tracks(), scene_base=scene_base, commit=False)


MAKERS = dict(trails=_trails, tripwires=_tripwires, stance=_stance, heat=_heat, zones=_zones)
FIELDS = [(name, which, field) for name, dtypes in dict(
    trails=(_lib.TRAIL_TRACK_DTYPE, _lib.TRAIL_POINT_DTYPE), tripwires=(_lib.TRIPWIRE_ROW_DTYPE, _lib.TRIPWIRE_EVENT_DTYPE),
    stance=(_lib.STANCE_ROW_DTYPE, _lib.STANCE_EVENT_DTYPE), heat=(_lib.HEAT_ROW_DTYPE, _lib.HEAT_CELL_DTYPE),
    zones=(_lib.ZONE_ROW_DTYPE, _lib.ZONE_EVENT_DTYPE)).items() for which in (0, 1) for field in dtypes[which].names]


def _flip(a, field):
    """One bit of the last byte but one of a[0][field]: another integer; in an fp64 another exponent, beyond any rounding bound."""
    dt, off = a.dtype.fields[field][:2]
    a.view(np.uint8).reshape(len(a), a.dtype.itemsize)[0, off + dt.itemsize - 2] ^= 1


def _drive(name, flip=None):
    run, export = MAKERS[name]()

    def host(**kw):
        got = tuple(x.copy() for x in export(**kw))
        assert len(got[0]) > 0 and len(got[1]) > 0, "both arrays of the export hold something"
        if flip is not None:
            _flip(got[flip[0]], flip[1])
        return got
    setattr(run.sb, run.host, host)
    return run.compare((name, flip))


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_an_adapter_accepts_the_restatements_own_export(name):
    rows, second = _drive(name)
    assert (rows["scene"] >= BASE).all()                     # (the adapter's scene_base reached both sides)


@pytest.mark.parametrize("name,which,field", FIELDS, ids=["-".join(map(str, f)) for f in FIELDS])
def test_an_adapter_refuses_one_flipped_byte(name, which, field):
    with pytest.raises(AssertionError) as ei:
        _drive(name, (which, field))
    assert repr(field) in str(ei.value) or (name, field) == ("trails", "travelled") and "travelled" in str(ei.value), str(ei.value)


def test_sample_turns_scenes_into_flags_and_broadcasts_t():
    class Recorder:
        def __init__(self, *args):
            self.args, self.seen = args, []

        def sample(self, tracks, ntr, flags=None, t=None):
            self.seen.append((flags, t))

    class Probe(FeatureRun):
        Ref, enable, sampler = Recorder, "enable_probe", "sample_probe"

    sb = _Stub()
    run = Probe(sb, 5, data=())
    assert run.ref.args == (2, T_CAP, 5) and sb.calls == [("enable_probe", (5,), {})]
    run.sample(t=0.25, scenes=[1])
    run.sample()
    (flags, t), (flags1, t1) = run.ref.seen
    assert flags.dtype == np.int32 and flags.tolist() == [0, 1] and t.shape == (2,) and t.dtype == np.float64 and t.tolist() == [0.25, 0.25]
    assert flags1 is None and t1 is None
    assert sb.calls[1:] == [("sample_probe", (), dict(t=0.25, scenes=[1])), ("sample_probe", (), dict(t=None, scenes=None))]


# ---- _snap_plant on a blob built without a GPU ---------------------------------------------------------------------------------
def test_directory_and_record_at_find_what_the_blob_builder_laid_out():
    blob = build_blob(SCENES)
    ents = sp.directory(blob)
    want, at = [], (600 + 48 * len(SCENES) + 15) // 16 * 16
    for n_tracks, g_rows, trk_rows in SCENES:                # build_blob: sections back to back behind the directory
        want.append(at)
        at += 64 + 1504 * n_tracks + 64 * (sum(g_rows) + sum(trk_rows))
    assert [int(o) for o in ents["offset"]] == want and at == len(blob)
    assert sp.record_at(ents, 0) == want[0] + 64 and sp.record_at(ents, 0, 1) == want[0] + 64 + 1504 and sp.record_at(ents, 2) == want[2] + 64


def test_plant_state_writes_x_a_zero_covariance_and_lifetime_0_and_nothing_else():
    orig = bytearray(build_blob(SCENES))
    ents = sp.directory(orig)
    at = sp.record_at(ents, 0, 1)
    for k in range(at, at + _lib.SNAP_TRACK_BYTES):          # (build_blob's records are zeros: make every byte of this one show)
        orig[k] = 0xA5
    blob = bytearray(orig)
    x6 = [0.5, -0.0, 1.0, 3.0, np.inf, -2.0 ** -1074]
    sp.plant_state(blob, at, x6)
    differs = {k for k in range(len(blob)) if blob[k] != orig[k]}
    assert differs and differs <= set(range(at, at + 720)) | set(range(at + sp.REC_LIFETIME, at + sp.REC_LIFETIME + 8))
    assert bytes(blob[at: at + 72]) == np.array(x6 + [0.0, 0.0, 0.0]).tobytes()
    assert bytes(blob[at + 72: at + 720]) == bytes(648) and bytes(blob[at + sp.REC_LIFETIME: at + sp.REC_LIFETIME + 8]) == bytes(8)
    assert (sp.REC_X, sp.REC_P, sp.REC_P + sp.P_BYTES) == (0, 72, 720)
    snapshot.inspect(bytes(blob))
    sp.plant_word(blob, at + sp.REC_X, np.nan)
    assert np.isnan(np.frombuffer(bytes(blob[at: at + 8]))[0]) and bytes(blob[at + 8: at + 72]) == np.array(x6[1:] + [0.0, 0.0, 0.0]).tobytes()


def test_record_offsets_agree_with_the_public_track_record_where_the_two_share_a_position():
    f = TRACK_DTYPE.fields
    assert (f["x"][1], f["P"][1], f["lifetime"][1], f["ring_len"][1]) == (sp.REC_X, sp.REC_P, sp.REC_LIFETIME, sp.REC_RING_LEN) == (0, 72, 1208, 1224)
    assert f["P"][0].itemsize == sp.P_BYTES
    # REC_UID = 1228 and REC_RING_N = 1232 are the snapshot's own order: the public record has ring_n[4] first and uid behind it, and
    # so its keypoints start at 1248 where the snapshot's 1496-byte record has them at REC_KP = 1264.  The records end alike:
    assert (sp.REC_UID, sp.REC_RING_N, sp.REC_KP) == (1228, 1232, 1264)
    assert sp.REC_KP + f["keypoints"][0].itemsize <= _lib.SNAP_TRACK_BYTES


def test_dts_are_the_differences_of_the_multipliers_and_zero_is_refused():
    assert sp.dts([[1, 3, 3.5]]).tolist() == [[1.0], [2.0], [0.5]]
    assert sp.dts([[1, 3], [-2, 2]]).tolist() == [[1.0, -2.0], [2.0, 4.0]]
    with pytest.raises(AssertionError):
        sp.dts([[1, 0, 2]])


class _OneScene:
    """A context of 3 scenes for the section builder: snapshot(scenes=[s]) is a one-scene blob, restore() keeps what it is given."""
    S = 3

    def snapshot(self, scenes):
        assert scenes in ([0], [2])
        return build_blob([(2, [], [])])

    def restore(self, blob, scenes):
        self.restored = (blob, scenes)


def test_plant_tracks_is_plant_xy_with_the_records_own_y_and_context_blob_repeats_the_section():
    sb = _OneScene()
    sp.plant_xy(sb, 2, [7, 3, 5], [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0)])     # (build_blob's first record: x[1] == 0.0)
    by_xy, scenes = sb.restored
    sp.plant_tracks(sb, 2, [7, 3, 5])
    assert sb.restored == (by_xy, [2]) and scenes == [2]
    info = snapshot.inspect(by_xy)
    ent = info["entries"][0]
    assert info["header"]["n_scenes"] == 1 and info["header"]["total_bytes"] == len(by_xy)
    assert (int(ent["n_tracks"]), int(ent["g_len"]), int(ent["bytes"])) == (3, 0, 64 + 3 * 1504)
    shdr = np.frombuffer(by_xy, np.int32, 16, int(ent["offset"]))
    assert shdr[0] == 3 and shdr[13] == 8                     # n_tracks, next_uid past every uid
    for k, (uid, x0) in enumerate(zip((7, 3, 5), (0.0, 0.25, 0.5))):
        at = sp.record_at(info["entries"], 0, k)
        assert np.frombuffer(by_xy, np.float64, 2, at + sp.REC_X).tolist() == [x0, 0.0]
        assert np.frombuffer(by_xy, np.int32, 1, at + sp.REC_UID)[0] == uid and np.frombuffer(by_xy, np.int32, 1, at + sp.REC_RING_LEN)[0] == 1
    whole = sp.context_blob(sb, [7, 3, 5], [(0.0, 0.0), (0.25, 0.0), (0.5, 0.0)])
    ents = snapshot.inspect(whole)["entries"]
    sec = by_xy[int(ent["offset"]):]
    assert len(ents) == 3 and all(whole[int(e["offset"]): int(e["offset"]) + int(e["bytes"])] == sec for e in ents)
