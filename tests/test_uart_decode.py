"""The UART decode pinned to the reference itself (no library needed here): tests/golden/uart_decode.npz records the reference's
ReadIWR14xx.read (src/ReadDataIWR1443.py:27-201) under the numpy it pins, 1.26 (oracle/gen_uart_golden.py).  Here the numpy
restatement that checks the device path (radar.decode_tlv_bodies_numpy) meets every decoded body of that recording, and the
recording meets a fresh run of its generator.  The library's own decode is pinned in tests/test_gpu_uart.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mmwave_msc_amd import radar
from tests._uart_recording import DET_KEYS, load, meta, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recording_reaches_the_edges():
    """What the recording must hold for the pins below to mean anything."""
    streams = load()
    m = meta()
    assert m["numpy"].startswith("1.26"), m
    decoded = [(s, r) for s in streams for r in s.reads if r.ok]
    qs = {int(np.frombuffer(r.body[2:4], "<u2")[0]) for _, r in decoded}
    assert set(range(71)) | {65535} <= qs
    det = np.concatenate([r.det for _, r in decoded])
    assert np.isnan(det[:, :3]).any() and np.isposinf(det[:, :3]).any() and np.isneginf(det[:, :3]).any()
    names = {s.name for s in streams}
    assert {"q_format", "header_edges", "objects_past_packet", "stale_bytes", "over_max_obj", "splits", "multi_and_garbage", "random_mix"} <= names
    assert sum(r.raised for s in streams for r in s.reads) >= 1
    assert max(r.num_obj for _, r in decoded) > 1024
    assert {s.cfg["numDopplerBins"] for s in streams} >= {1.0, 2.0, 64 / 3}
    # the 2^15-byte rule dropped a chunk somewhere: a read whose buffer did not grow by its chunk while nothing was decoded
    dropped = any(not r.ok and not r.raised and len(r.chunk) > 0 and r.buflen == prev.buflen
                  for s in streams for prev, r in zip(s.reads, s.reads[1:]))
    assert dropped


def test_decode_tlv_bodies_numpy_matches_the_reference_recording():
    """radar.decode_tlv_bodies_numpy (the device path's checker) on every TLV body the reference decoded: x, y, z, doppler and
    peakVal bit-equal to what read() returned, NaN matching NaN and inf matching inf of the same sign (Q >= 63: the reference's
    `2 ** Q` is a numpy int64 and wraps)."""
    bad = []
    for s in load():
        for r in s.reads:
            if not r.ok:
                continue
            n = r.num_obj
            stride = 4 + 12 * max(n, 1)
            stride += stride & 1
            body = np.zeros((1, stride), np.uint8)
            body[0, : len(r.body)] = np.frombuffer(r.body, np.uint8)
            raw, cnt = radar.decode_tlv_bodies_numpy(body, s.cfg)
            assert cnt[0] == n
            for c, key in enumerate(DET_KEYS[:5]):
                if not same_bits(raw[0, :n, c], r.det[:, c]):
                    bad.append((s.name, r.index, key, int(np.frombuffer(r.body[2:4], "<u2")[0])))
    assert not bad, f"{len(bad)} decoded columns differ from the reference's read(), e.g. (stream, read, column, Q): {bad[:12]}"


def test_recorded_indices_are_the_bodies_words():
    """rangeIdx / peakVal as the reference returned them are the body's int16 words, and dopplerIdx is its wrap of them."""
    for s in load():
        for r in s.reads:
            if not r.ok:
                continue
            w = np.frombuffer(r.body[4:], "<i2").reshape(-1, 6)
            assert np.array_equal(w[:, 0], r.idx[:, 0]) and np.array_equal(w[:, 2], r.det[:, 4])
            dop = w[:, 1].copy()
            hi = dop > s.cfg["numDopplerBins"] / 2 - 1
            dop[hi] = (dop[hi].astype(np.int32) - 65535).astype(np.int16)
            assert np.array_equal(dop, r.idx[:, 1]), (s.name, r.index)


def _py126():
    for p in ("/opt/conda/bin/python3.9", shutil.which("python3.9") or ""):
        if p and os.path.exists(p):
            v = subprocess.run([p, "-c", "import numpy; print(numpy.__version__)"], capture_output=True, text=True)
            if v.returncode == 0 and v.stdout.strip().startswith("1.26"):
                return p
    return None


@pytest.mark.reference
def test_recording_is_what_the_generator_writes(tmp_path):
    """oracle/gen_uart_golden.py run again (numpy-1.26 interpreter, the reference's own read()) writes the same arrays."""
    py = _py126()
    if py is None:
        pytest.skip("no interpreter with numpy 1.26 to run the reference's read()")
    out = str(tmp_path / "uart_decode.npz")
    subprocess.run([py, os.path.join(ROOT, "oracle", "gen_uart_golden.py"), out], check=True, capture_output=True, timeout=600)
    a, b = np.load(out), np.load(os.path.join(ROOT, "tests", "golden", "uart_decode.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
