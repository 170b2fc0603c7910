"""Every kernel that writes a frame's rows -- k_normalize<double | float, R, SITE> and k_normalize_tlv<R, SITE>, k_uart_read<R, SITE,
LOG>, each flag false and true -- ends in normalize_rows<R> (csrc/mmw_normalize.hpp).  Here each of them, at 1, 2 and 4
rows per thread (max_pts 256 | 257, 512 | 513, 768, 1024), against the C oracle.

NO expected value in this file comes from a GPU call: every `want` is tests/_rows_ref.py's expected_rows -- oracle.c_oracle.normalize
under the scene's mounting -- of raw rows built on the host (the wire-format tests decode their bodies with
radar.decode_tlv_bodies_numpy, host numpy pinned to the reference's recorded read()).  Never normalize_host, never another kernel.
Every comparison is by bits (same_bits: NaN equals NaN), n_out is exact, and `pts` is prefilled with a sentinel that must survive
at and beyond n_out[s]: a compaction that stores past its count does not pass.  What makes the inputs sensitive to a wrong block
offset, and the edge rows' fate, is asserted without a GPU in tests/test_row_inputs.py.

Last, mmw_step_f32 with 2 and 4 points per thread (k_track / k_scene's fp32 loads, load_point_row<true>) against mmw_step on the
promoted rows and against OracleScene."""
import functools

import numpy as np
import pytest

from tests import _rows_ref as rr
from tests._layouts import LAYOUTS, make_checked
from tests.test_sites_golden import same_bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ expected values: the oracle, once
@functools.lru_cache(maxsize=None)
def _expected(max_pts, group, f32, sites):
    """(scenes, want): the scenes of one context and expected_rows of each under its own mounting.  Shared, never modified."""
    scenes = rr.scene_group(max_pts, group, f32=f32, sites=sites)
    want = [rr.expected_rows(sc.mount, sc.raw, sc.n) for sc in scenes]
    for w in want:
        w.setflags(write=False)
    return scenes, want


@functools.lru_cache(maxsize=None)
def _tlv_inputs(max_pts):
    """(tags, bodies[S, stride] uint8, raw[S, max_pts, 5], counts[S]): raw / counts are the HOST decode of the bodies."""
    tags, objs, counts = rr.tlv_group(max_pts)
    bodies = rr.tlv_bodies(objs, counts, max_pts)
    raw, cnt = rr.decoded_rows(bodies, max_pts)
    assert list(cnt) == counts
    for a in (bodies, raw):
        a.setflags(write=False)
    return tags, bodies, raw, counts


def _tlv_mounts(S, sites):
    return [rr.MOUNTINGS[s % len(rr.MOUNTINGS)] if sites else rr.EXACT for s in range(S)]


# --------------------------------------------------------------------------------------------------------------- contexts
def _context(max_pts, mounts, sites):
    """A context of len(mounts) scenes: without sites under mounts[0] (all equal), with sites each scene under its own.  Asserts
    that the mounting each scene really has is the one its expected rows were computed under."""
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    S = len(mounts)
    if not sites:
        assert all(m == mounts[0] for m in mounts)
        sb = SceneBatch(_lib.default_config(**mounts[0]), S, max_pts)
        assert not sb.has_sites
        have = [rr.mounting(sb.cfg)] * S
    else:
        sb = SceneBatch(_lib.default_config(), S, max_pts)
        hcs = [rr.mounting(sb.cfg) if m == rr.DEFAULT else rr.mounting(m) for m in mounts]
        sb.set_sites(_lib.make_sites(sb.cfg, S, s_height=[v[0] for v in hcs], tilt_cos=[v[1] for v in hcs], tilt_sin=[v[2] for v in hcs]))
        assert sb.has_sites
        have = [rr.mounting(site) for site in sb.sites()]
        assert len(set(have)) >= 2
    assert have == [rr.mounting(m) for m in mounts], (have, mounts)
    return sb


def _sentinel(sb, name):
    S, M = sb.S, sb.max_pts
    return sb.buf(name, S * M * 64).upload(np.full((S, M, 8), rr.SENTINEL))


def _check_rows(pts, n_out, want, tags, where):
    """n_out exact, the kept rows bit-equal to the oracle's, everything at and beyond n_out still the sentinel."""
    assert list(n_out) == [len(w) for w in want], (where, list(zip(tags, n_out.tolist(), [len(w) for w in want])))
    for s, w in enumerate(want):
        got = pts[s, : len(w)]
        if not same_bits(got, w):
            bad = np.argwhere(~((got == w) | (np.isnan(got) & np.isnan(w))))
            raise AssertionError(f"{where} scene {s} ({tags[s]}): {len(bad)} values differ, first at output row {bad[0][0]} column {bad[0][1]} "
                                 f"(raw row {w[bad[0][0], 7]:.0f}): got {got[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")
        tail = pts[s, len(w):]
        assert np.all(tail == rr.SENTINEL), (where, s, tags[s], "rows written past n_out", np.argwhere(tail != rr.SENTINEL)[:4].tolist())


# ------------------------------------------------------------------------------------- mmw_normalize / mmw_normalize_f32
@pytest.mark.parametrize("sites", [False, True], ids=["ctx", "sites"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("group", ["counts", "edges"])
@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_normalize_equals_the_oracle(max_pts, group, f32, sites):
    """k_normalize<double | float, R, false> and k_normalize<., R, true>: seam frames, the count list (with the counts normalize_scene
    clamps) and the edge rows.  The fp32 entry gets the same values where float32 holds them exactly; the edge rows that need
    5e-324 or 1e+-200 (the smallest double, r == 0 by underflow, r == inf by overflow) exist in no float32 and are left out
    of the fp32 runs, which get float32's own one-ulp neighbours and smallest positive value instead (_rows_ref.edge_rows)."""
    scenes, want = _expected(max_pts, group, f32, sites)
    S = len(scenes)
    sb = _context(max_pts, [sc.mount for sc in scenes], sites)
    raw = np.stack([sc.raw for sc in scenes])
    if f32:
        raw32 = raw.astype(np.float32)
        assert same_bits(raw32.astype(np.float64), raw)                    # the fp32 entry sees the oracle's values
        raw = raw32
    b_raw = sb.buf("raw", raw.nbytes).upload(raw)
    b_n = sb.buf("n", S * 4).upload(np.array([sc.n for sc in scenes], np.int32))
    b_out, b_no = _sentinel(sb, "pts"), sb.buf("n_out", S * 4).upload(np.full(S, -99, np.int32))
    sb.normalize_dev(b_raw.ptr, b_n.ptr, b_out.ptr, b_no.ptr, f32=f32)
    n_out, pts = b_no.download((S,), np.int32), b_out.download((S, max_pts, 8), np.float64)
    _check_rows(pts, n_out, want, [sc.tag for sc in scenes], (max_pts, group, f32, sites))
    sb.close()


# ----------------------------------------------------------------------------------------------------- mmw_normalize_tlv
@pytest.mark.parametrize("sites", [False, True], ids=["ctx", "sites"])
@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_normalize_tlv_equals_host_decode_then_the_oracle(max_pts, sites):
    """k_normalize_tlv<R, false> / k_normalize_tlv<R, true> on bodies encoded from int16 objects (seam frames in wire format, the count
    list, y == 0 objects, doppler indices on both sides of the wrap) at 2-byte-aligned offsets.  Expected: the host numpy decode
    of the same bytes, then the oracle."""
    from mmwave_msc_amd import radar
    tags, bodies, raw, counts = _tlv_inputs(max_pts)
    S = len(tags)
    mounts = _tlv_mounts(S, sites)
    want = [rr.expected_rows(mounts[s], raw[s], counts[s]) for s in range(S)]
    sb = _context(max_pts, mounts, sites)
    blob, offs = rr.tlv_blob(bodies)
    assert np.all(offs % 2 == 0) and np.any(offs % 4 == 2)
    b_pk = sb.buf("tlv_bytes", len(blob) + 16).upload(np.frombuffer(blob, dtype=np.uint8))
    b_of = sb.buf("tlv_off", S * 8).upload(offs)
    b_out, b_no = _sentinel(sb, "pts"), sb.buf("n_out", S * 4).upload(np.full(S, -99, np.int32))
    sb.normalize_tlv_dev(b_pk.ptr, len(blob), b_of.ptr, radar.uart_cfg(rr.CFGP), b_out.ptr, b_no.ptr)
    n_out, pts = b_no.download((S,), np.int32), b_out.download((S, max_pts, 8), np.float64)
    _check_rows(pts, n_out, want, tags, (max_pts, sites))
    sb.close()


# --------------------------------------------------------------------------------------------------------- mmw_uart_read
@pytest.mark.parametrize("mode", ["plain", "sites", "log", "sites+log"])
@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_uart_read_equals_host_decode_then_the_oracle(max_pts, mode):
    """k_uart_read<R, SITE, LOG>, all four combinations of the flags: three reads, each delivering one complete packet to every scene
    (read k gives scene s the body of scene s + k, so the second and third start from the buffer the one before cut): status
    MMW_UART_POINTS, the frame number, n and the rows against the host decode + the oracle under the scene's mounting.  With the
    log enabled the staged frame is the host decode as well.  A fourth read: max_pts + 1 objects stay MMW_UART_OVERFLOW."""
    from mmwave_msc_amd import _lib
    tags, bodies, raw, counts = _tlv_inputs(max_pts)
    S = len(tags)
    sites, log = "sites" in mode, "log" in mode
    mounts = _tlv_mounts(S, sites)
    sb = _context(max_pts, mounts, sites)
    sb.open_radars(rr.CFGP, t0=0.0)
    if log:
        sb.enable_radar_log()

    def download(r):
        return (r.status.download((S,), np.int32), r.frame_number.download((S,), np.uint32), r.n.download((S,), np.int32),
                r.pts.download((S, max_pts, 8), np.float64))

    for k in range(3):
        src = [(s + k) % S for s in range(S)]
        chunks = [rr.uart_packet(100 + k, bodies[j], counts[j]) for j in src]
        want = [rr.expected_rows(mounts[s], raw[j], counts[j]) for s, j in enumerate(src)]
        _sentinel(sb, "radar_pts")                                         # (the buffer read_radars hands to the kernel)
        status, frame, n_out, pts = download(sb.read_radars(chunks, now=1.0 + k))
        assert list(status) == [_lib.UART_POINTS] * S, (mode, k, status)
        assert list(frame) == [100 + k] * S, (mode, k, frame)
        _check_rows(pts, n_out, want, [tags[j] for j in src], (max_pts, mode, "read", k))
        if log:
            d, rows = sb.radar_log_host()
            assert list(d["scene"]) == list(range(S)) and list(d["count"]) == [counts[j] for j in src], (mode, k)
            assert list(d["frame_number"]) == [100 + k] * S
            for e, j in zip(d, src):
                mine = rows[e["first"]: e["first"] + e["count"]]
                for c, col in enumerate(("x", "y", "z", "doppler", "peak_val")):
                    assert same_bits(mine[col], raw[j, : counts[j], c]), (mode, k, int(e["scene"]), col)
    # max_pts + 1 objects: refused as before, nothing written
    o = rr.tlv_objects(np.random.default_rng(5), max_pts + 1)
    body = np.frombuffer(np.array([max_pts + 1, rr.QFMT], "<u2").tobytes() + np.ascontiguousarray(o, "<i2").tobytes(), dtype=np.uint8)
    _sentinel(sb, "radar_pts")
    status, frame, n_out, pts = download(sb.read_radars([rr.uart_packet(200, body, max_pts + 1)] + [b""] * (S - 1), now=9.0))
    assert status[0] == _lib.UART_OVERFLOW and n_out[0] == _lib.BAD_FRAME and list(status[1:]) == [_lib.UART_NONE] * (S - 1), status
    assert not n_out[1:].any() and np.all(pts == rr.SENTINEL)
    sb.close()


# ---------------------------------------------------------------------------- mmw_step_f32 at 2 and 4 points per thread
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("max_pts", [320, 1024])
def test_fp32_step_with_2_and_4_points_per_thread(max_pts, layout):
    """mmw_step_f32 where a thread of k_track / k_scene owns 2 (max_pts 320) and 4 (max_pts 1024) points -- the `i * 2` float4
    loads and the q * 256 + tid seams of load_point_row<true> -- against mmw_step on the promoted rows: association, labels,
    db_n and every byte of tracks() equal after every frame; the final state equal to OracleScene's.  Counts reach past row 256
    / 768 in every scene; one scene-frame is skipped (count 0) and one is MMW_EMPTY_FRAME."""
    import torch
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.synth import make_batch
    from oracle import c_oracle as co
    from tests._golden import assert_tracks_match
    S, N, F, T = 8, max_pts, 8, 4
    # (track_cap: the default, tr_max_tracks - 1 + 3 * max_pts / db_min_samples + 1, is 31 at 320 points and would be cut to the
    #  limit of 64 at 1024, which forbids every layout but per_scene; 32 holds these scenes' tracks -- check() below says so)
    kw = dict(tr_max_tracks=T, track_cap=32)
    pts = np.zeros((F, S, N, 8), np.float32); cnt = np.zeros((F, S), np.int32); dts = np.zeros((F, S))
    for s in range(S):
        p, c, d = make_batch([7300 + 10 * N + s], F, N, 1 + s % T, ragged=(s % 2 == 0))
        pts[:, s], cnt[:, s], dts[:, s] = p[:, 0], c[:, 0], d[:, 0]
    cnt[:, 0] = N                                                          # (a ragged scene may stay short: this one never does)
    reach = 256 if N == 320 else 768
    assert (N + 255) // 256 == (2 if N == 320 else 4)
    assert np.all(cnt.max(axis=0) > reach), cnt.max(axis=0)               # every scene has rows in the last 256-row group
    cnt[3, 5] = 0; cnt[4, 6] = _lib.EMPTY_FRAME
    assert np.all(np.delete(cnt[:, 5], 3).max() > reach) and np.delete(cnt[:, 6], 4).max() > reach
    a, b = make_checked(S, N, layout, **kw), make_checked(S, N, layout, **kw)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        a.follow_torch_stream(st); b.follow_torch_stream(st)
        d_cnt = torch.from_numpy(cnt).to(dev); d_dt = torch.from_numpy(dts).to(dev)
        out = [dict(a=torch.full((S, N), -7, dtype=torch.int32, device=dev), l=torch.full((S, a.UM), -7, dtype=torch.int32, device=dev),
                    n=torch.full((S,), -7, dtype=torch.int32, device=dev)) for _ in range(2)]
        for f in range(F):
            p32 = torch.from_numpy(pts[f]).to(dev)
            p64 = p32.double()
            a.step_dev(p64.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr(), out[0]["a"].data_ptr(), out[0]["l"].data_ptr(), out[0]["n"].data_ptr())
            b.step_dev_f32(p32.data_ptr(), d_cnt[f].data_ptr(), d_dt[f].data_ptr(), out[1]["a"].data_ptr(), out[1]["l"].data_ptr(), out[1]["n"].data_ptr())
            st.synchronize()
            for k in ("a", "l", "n"):
                assert torch.equal(out[0][k], out[1][k]), (f, k)
            na, nb = a.num_tracks(), b.num_tracks()
            assert np.array_equal(na, nb), f
            assert a.tracks(cap=max(int(na.max()), 1)).tobytes() == b.tracks(cap=max(int(na.max()), 1)).tobytes(), f
    a.check(); b.check()
    ocfg = co.default_config(**kw)
    ntr = b.num_tracks(); trk = b.tracks(cap=max(int(ntr.max()), 1))
    assert ntr.sum() > 0
    for s in range(S):
        sc = co.OracleScene(ocfg, N)
        for f in range(F):
            if cnt[f, s] != 0:   # (0: the frame never reaches track(); -1: track() on an empty cloud)
                sc.track(pts[f, s, : max(int(cnt[f, s]), 0)].astype(np.float64), float(dts[f, s]))
        assert ntr[s] == sc.n_tracks, s
        assert_tracks_match(trk[s, : ntr[s]], sc.tracks(), ctx=f"scene {s}", exact=True)
    a.close(); b.close()
