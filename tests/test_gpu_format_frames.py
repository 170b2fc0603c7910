"""mmw_format_frames (k_format_frames, the 64-row sort of mmwave_msc_amd/csrc/mmw_sort.hpp) on the key frames of
tests/_sort_inputs.py, bit for bit against format_frames_ref: ties among real rows, real rows that tie with the pad rows, -0.0,
+-inf, keys that differ as fp64 and not as fp32, counts of 0, above 64 and -1 -- and NaN keys, which go last in row order.

NO expected value comes from a GPU call.  tests/test_sort_inputs.py shows on the CPU that these frames tell the right network
from one with a step missing, a step of the last merge reversed, ties broken by the larger row or fp32 keys.  One launch per
test; B * ring is no multiple of 4, so the last workgroup has idle waves and four frames of different m share a workgroup."""
import numpy as np
import pytest

from tests import _sort_inputs as si

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-77.25)
GUARD = 256   # floats behind feat[B * ring * 320]


def _run(which, ring):
    from mmwave_msc_amd import _lib
    from mmwave_msc_amd.batch import SceneBatch
    p = si.pack(which, ring)
    B = len(p.frames)
    sb = SceneBatch(_lib.default_config(fb_frames_batch=ring - 1, intensity_mu=si.MU, intensity_std=si.STD), 1, 64)
    assert sb.ring == ring and (sb.cfg.intensity_mu, sb.cfg.intensity_std) == (si.MU, si.STD)
    n = B * ring * 320
    fill = np.full(n + GUARD, SENTINEL, np.float32)
    b_fr, b_cnt, b_ref = sb.alloc(p.frames.nbytes).upload(p.frames), sb.alloc(p.counts.nbytes).upload(p.counts), sb.alloc(p.ref.nbytes).upload(p.ref)
    b_out = sb.alloc(fill.nbytes).upload(fill)
    sb._chk(sb.L.mmw_format_frames(sb.h, b_fr.ptr, b_cnt.ptr, b_ref.ptr, b_out.ptr, B))
    sb.synchronize()
    out = b_out.download(fill.shape, np.float32)
    for b in (b_fr, b_cnt, b_ref, b_out):
        b.free()
    sb.close()
    assert np.all(out[n:] == SENTINEL), f"written behind feat[B * ring * 320] at {np.flatnonzero(out[n:] != SENTINEL)[:8].tolist()}"
    return p, out[:n].reshape(B, ring, 64, 5)


def _compare(p, got):
    want = si.format_frames_ref(p.frames, p.counts, p.ref, si.MU, si.STD, p.ring)
    assert not np.any(got == SENTINEL), "a row of the output was not written"
    bad = []
    for b, item in enumerate(p.src):
        for k, kf in enumerate(item):
            g, w = got[b, k], want[b, k]
            if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
                rows = {r.tobytes() for r in g}
                lost = sum(1 for r in w if r.tobytes() not in rows)
                bad.append(f"item {b} frame {k} ({kf.tag if kf else 'absent'}): {int(np.any(g.view(np.uint32) != w.view(np.uint32), axis=1).sum())} "
                           f"rows differ, {lost} input rows are missing from the output")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("ring", [3, 1])
def test_ties_signed_zeros_infinities_and_counts(ring):
    """The stable sort on the fp64 key: ties by row position (the identity where all 64 keys are equal), real rows with x == 0 in
    front of the pad rows, -0.0 == 0.0, +-inf at the ends, b + 1 ulp behind b; rows at and past the count never show."""
    _compare(*_run("finite", ring))


@pytest.mark.parametrize("ring", [3, 1])
def test_nan_keys_go_last_in_row_order_and_every_row_is_written_once(ring):
    """NaN x in caller data: np.argsort puts those rows behind all others, +inf included, in row order.  The bare network is no
    permutation on them (both lanes of a pair keep the same element: rows lost, rows doubled -- tests/test_sort_inputs.py);
    k_format_frames sorts them as +inf with bit 6 of the row set."""
    p, got = _run("nan", ring)
    want = si.format_frames_ref(p.frames, p.counts, p.ref, si.MU, si.STD, ring)
    for b, item in enumerate(p.src):
        for k, kf in enumerate(item):
            if kf is not None and np.isnan(kf.keys).any():       # every input row exactly once
                assert sorted(r.tobytes() for r in got[b, k].view(np.uint32)) == sorted(r.tobytes() for r in want[b, k].view(np.uint32)), kf.tag
    _compare(p, got)
