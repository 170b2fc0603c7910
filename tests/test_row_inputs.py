"""The inputs of tests/test_gpu_row_producers.py (tests/_rows_ref.py) have the properties that give those tests their teeth --
asserted here on the C oracle alone, without a GPU: the seam frames' per-block counts, the edge rows' fate, the fp32 variants'
exactness, the count lists, and that a wrong block offset in the ordered compaction cannot reproduce the expected bytes."""
import itertools

import numpy as np
import pytest

from tests import _rows_ref as rr
from tests.test_sites_golden import same_bits


def _counts_per_block(mount, raw):
    return [len(b) for b in rr.blocks_of(mount, raw, len(raw))]


def _check_seam(mount, raw, ks, where):
    M = len(raw)
    got = _counts_per_block(mount, raw)
    assert got == ks, (where, got, ks)
    assert all(0 < k < 64 for k in got) and len(set(got)) == len(got) == (M + 63) // 64, (where, got)
    assert all(k <= size for k, size in zip(got, rr.block_sizes(M))), (where, got)
    assert len(set(raw[:, 4].tolist())) == M and np.array_equal(raw[:, 4], np.arange(M)), where   # peakVal = row index
    out = rr.expected_rows(mount, raw, M)
    assert np.array_equal(out[:, 7], np.flatnonzero(np.isin(np.arange(M), out[:, 7]))), where     # ordered, each row once


@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_seam_frames_keep_a_different_count_in_every_block_under_every_mounting(max_pts):
    for seed in (1000 * max_pts, 1000 * max_pts + 1, 1000 * max_pts + 2, 1000 * max_pts + 9):
        raw, ks = rr.seam_frame(max_pts, seed)
        assert raw.shape == (max_pts, 5)
        for mount in rr.MOUNTINGS:
            _check_seam(mount, raw, ks, (max_pts, seed, mount))


@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_seam_property_holds_on_the_decoded_tlv_rows(max_pts):
    """The wire-format seam frames, after the host decode the TLV tests take their expected rows from; the dropped rows include
    y == 0 objects, which only the `y > 0` comparison drops."""
    for k in range(3):
        o, ks = rr.seam_objects(max_pts, 500 * max_pts + k)
        raw, cnt = rr.decoded_rows(rr.tlv_bodies([o], [max_pts], max_pts), max_pts)
        assert raw.shape == (1, max_pts, 5) and cnt[0] == max_pts
        for mount in rr.MOUNTINGS:
            _check_seam(mount, raw[0], ks, (max_pts, k, mount))
        y0 = (raw[0, :, 1] == 0) & (raw[0, :, 2] == 0)
        if max_pts > 257:
            assert y0.any()
        h = rr.mounting(rr.EXACT)[0]
        assert np.all((raw[0, y0, 2] + h > 0) & (raw[0, y0, 2] + h <= 2.5))       # z' passes: y' == 0 is what drops them


def test_count_lists():
    for M in rr.MAX_PTS:
        cl = rr.count_list(M)
        assert cl[-3:] == [-1, -7, M + 5] and rr.count_list(M, clamped=False) == cl[:-3]
        inside = cl[:-3]
        assert inside == sorted(set(inside)) and inside[0] == 0 and inside[-2:] == [M - 1, M] and max(inside) <= M
        for edge in (64, 256, 512, 768):
            if edge < M:
                assert {edge - 1, edge, edge + 1} <= set(inside), (M, edge)
    assert 513 in rr.count_list(513) and 769 not in rr.count_list(768) and 769 in rr.count_list(1024)


@pytest.mark.parametrize("group", ["counts", "edges"])
@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_scene_groups_fit_a_context_and_keep_and_drop_rows(max_pts, group):
    for sites in (False, True):
        scenes = rr.scene_group(max_pts, group, sites=sites)
        assert len(scenes) <= 24
        if sites:
            mounts = {tuple(sorted(sc.mount.items())) for sc in scenes}
            assert len(mounts) >= (3 if group == "counts" else 2), mounts
            assert any(sc.mount == rr.EXACT for sc in scenes) and any(sc.mount == rr.DEFAULT for sc in scenes)
        kept = dropped = 0
        for sc in scenes:
            assert sc.raw.shape == (max_pts, 5)
            want = rr.expected_rows(sc.mount, sc.raw, sc.n)
            n = min(max(sc.n, 0), max_pts)
            assert len(want) <= n
            kept += len(want)
            dropped += n - len(want)
            if n <= max_pts - 64:   # the rows at and past n are rows the filter keeps some of: a kernel that ignored n would show
                assert len(rr.expected_rows(sc.mount, sc.raw, max_pts)) > len(want), sc.tag
        assert kept > 0 and dropped > 0


@pytest.mark.parametrize("f32", [False, True])
def test_edge_rows_are_kept_or_dropped_as_listed(f32):
    edges = rr.edge_rows(f32)
    assert len(edges) == (12 if f32 else 14)
    for e in edges:
        got = rr.expected_rows(rr.EXACT, np.array([e.row + (7.0,)]), 1)
        assert len(got) == int(e.kept), (e.name, got)
        if not e.kept:
            continue
        assert got[0, 6] == e.row[3] or (np.isnan(got[0, 6]) and np.isnan(e.row[3])), e.name   # the doppler passes through
        assert got[0, 0] == e.row[0] and got[0, 1] == e.row[1] and got[0, 2] == e.row[2] + 1.0 and got[0, 7] == 7.0, (e.name, got)
        if e.vel is not None:
            assert same_bits(got[0, 3:6], np.array(e.vel)), (e.name, got[0, 3:6])
            if np.isnan(e.vel[0]):
                assert got[0, 3:6].view(np.uint64).tolist() == [0x7FF8000000000000] * 3, e.name       # the canonical quiet NaN
    by = {e.name: e for e in edges}
    assert by["z' == 2.5"].row[2] + 1.0 == 2.5 and by["z' == 2.5 + 1 ulp"].row[2] + 1.0 > 2.5
    assert by["z' == 0"].row[2] + 1.0 == 0.0 and by["z' == 0 + 1 ulp"].row[2] + 1.0 > 0.0
    if not f32:
        assert by["z' == 2.5 + 1 ulp"].row[2] + 1.0 == np.nextafter(2.5, 3.0)
        assert np.nextafter(1.5, 2.0) + 1.0 == 2.5                                # why one ulp of 1.5 is not enough
        u = by["r == 0 by underflow"].row
        assert u[1] > 0 and u[0] * u[0] + u[1] * u[1] + u[2] * u[2] == 0.0
        with np.errstate(over="ignore"):
            assert np.isinf(np.float64(by["r == inf by overflow"].row[0]) ** 2)


@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_edge_frames_put_the_edge_row_where_the_seams_are(max_pts):
    pos = rr.edge_positions(max_pts)
    assert pos[0] == 0 and pos[-1] == max_pts - 1 and {63, 64, 255} <= set(pos)
    assert all(256 * q in pos for q in range((max_pts + 255) // 256) if 256 * q < max_pts)
    for f32 in (False, True):
        for e, edge in enumerate(rr.edge_rows(f32)):
            raw = rr.edge_frame(max_pts, edge, 31 * max_pts + e)
            assert same_bits(raw[pos, :4], np.tile(np.array(edge.row), (len(pos), 1))), edge.name
            assert np.array_equal(raw[:, 4], np.arange(max_pts))
            out = rr.expected_rows(rr.EXACT, raw, max_pts)
            assert all((p in out[:, 7]) == edge.kept for p in pos), edge.name
            assert 0 < len(out) < max_pts


@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_fp32_variants_are_exactly_representable(max_pts):
    """What the fp32 entries are given: every value survives the round trip through float32 (NaN stays NaN), so the fp32 and the
    fp64 entry see the same numbers and one oracle call serves both."""
    def exact(a):
        a = np.asarray(a, np.float64)
        with np.errstate(over="ignore"):
            return bool(np.all((a.astype(np.float32).astype(np.float64) == a) | np.isnan(a)))
    for group in ("counts", "edges"):
        for sc in rr.scene_group(max_pts, group, f32=True):
            assert exact(sc.raw), (group, sc.tag)
    assert not exact(np.array([e.row for e in rr.edge_rows(False)]))             # (the fp64 list holds rows float32 cannot)
    tags, objs, counts = rr.tlv_group(max_pts)
    raw, _ = rr.decoded_rows(rr.tlv_bodies(objs, counts, max_pts), max_pts)
    assert exact(raw[..., :3]) and exact(raw[..., 4])


@pytest.mark.parametrize("max_pts", rr.MAX_PTS)
def test_a_wrong_block_offset_changes_the_expected_bytes(max_pts):
    """The compaction's output re-assembled in numpy from what each 64-row block keeps: with any two blocks swapped, or any one
    block's offset moved by one row either way (whichever block stores last where two then overlap), pts or n_out differs from
    the true expected output -- so the GPU tests, which compare every row below n_out, the sentinel above it and n_out itself,
    cannot pass with a wrong block offset."""
    for mount in (rr.EXACT, rr.DEFAULT):
        raw, _ = rr.seam_frame(max_pts, 1000 * max_pts)
        blocks = rr.blocks_of(mount, raw, max_pts)
        true, n_true = rr.assemble(blocks, max_pts)
        want = rr.expected_rows(mount, raw, max_pts)
        assert n_true == len(want) and same_bits(true[:n_true], want) and np.all(true[n_true:] == rr.SENTINEL)
        nb = len(blocks)
        assert nb == (max_pts + 63) // 64

        def differs(pts, n):
            return n != n_true or not same_bits(pts, true)

        for a, b in itertools.combinations(range(nb), 2):
            order = list(range(nb))
            order[a], order[b] = order[b], order[a]
            assert differs(*rr.assemble(blocks, max_pts, order=order)), (a, b)
        for b in range(nb):
            for d in (-1, 1):
                if b == 0 and d < 0:
                    continue                                                    # (an offset of -1: out of bounds, not a wrong row)
                for late in (None, b, b - 1 if b else None, b + 1 if b + 1 < nb else None):
                    assert differs(*rr.assemble(blocks, max_pts, shift=(b, d), late=late)), (b, d, late)
            # a repeated offset: block b stored where block b - 1 went
            if b:
                pts, n = rr.assemble(blocks, max_pts, shift=(b, -len(blocks[b - 1])), late=b)
                assert differs(pts, n), b
