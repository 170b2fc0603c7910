"""The radar log (mmw_uart_log_*, include/mmw.h; radar.ExperimentLogger) as far as a machine without a GPU can check it: the header
declares the entries and the library exports them, the numpy layouts are the C structs', the kernels of csrc/k_uart_log.hip compile
without scratch, spills or LDS and store rows as 16-byte pieces, and ExperimentLogger writes the shards DataLogging.py's
write_thread writes -- read back through utils.OfflineManager bit for bit."""
import ctypes as C
import io
import os
import re

import numpy as np

from mmwave_msc_amd import _lib
from tests import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS_F = ["scene", "frame_number", "first", "count", "t", "q_format", "reserved_"]
FIELDS_O = ["x", "y", "z", "doppler", "peak_val", "range"]


def test_header_binding_and_library_agree_on_the_log_entries():
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bk_uart_log\.hip\b", mk, flags=re.M) and "api_uart_log.hip" in mk
    decl = open(os.path.join(csrc, "mmw_kernels.hpp")).read()
    assert len(re.findall(r"\bvoid\s+launch_uart_log\s*\(", decl)) == 1
    # the export scans with the shared kernel and decodes with the readers' own functions: called, not restated
    src = open(os.path.join(csrc, "k_uart_log.hip")).read()
    assert "launch_pair_scan(" in src and "__shared__" not in src
    for fn in ("decode_tlv_object(", "xyz_q_divisor("):
        assert fn in src, fn
    assert "uart_log_free(c)" in open(os.path.join(csrc, "api_context.hip")).read()   # (mmw_destroy releases the log)


def test_every_log_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    a, b = C.c_int32(7), C.c_int32(9)
    assert L.mmw_uart_log_enable(None, 1) == _lib.E_ARG
    assert L.mmw_uart_log_async(None, None, 0, None, 0, None, 1, 0, 0) == _lib.E_ARG
    assert L.mmw_uart_log_wait(None, 0, C.byref(a), C.byref(b)) == _lib.E_ARG
    assert L.mmw_uart_log(None, None, 0, None, 0, None, 1, 0, C.byref(a), C.byref(b)) == _lib.E_ARG
    assert (a.value, b.value) == (7, 9)


def test_log_layouts_match_the_c_structs():
    lay = _abi.c_layout()
    assert (lay["mmw_uart_frame"]["size"], lay["mmw_uart_object"]["size"]) == (32, 48)
    fdt, odt = _lib.UART_FRAME_DTYPE, _lib.UART_OBJECT_DTYPE
    assert (fdt.itemsize, odt.itemsize) == (32, 48)
    assert list(fdt.names) == FIELDS_F and list(odt.names) == FIELDS_O
    for f in FIELDS_O:
        assert odt.fields[f][0] == np.dtype("f8"), f
    assert fdt.fields["frame_number"][0] == np.dtype("u4") and fdt.fields["t"][0] == np.dtype("f8")
    for name in ("k_uart_log.hip", "api_uart_log.hip"):
        txt = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", name)).read()
        assert re.search(r"static_assert\(sizeof\(mmw_uart_frame\) == 32", txt), name
        assert re.search(r"static_assert\(sizeof\(mmw_uart_object\) == 48", txt), name


def test_log_kernels_use_no_scratch_no_lds_and_store_16_byte_pieces():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_uart_log",))["k_uart_log"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    assert sum("k_ulog_count" in n for n in names) == 1 and sum("k_ulog_write" in n for n in names) == 1 and len(names) == 2, names
    lds = dict(zip(names, [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", rep)]))
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        assert lds[name] == 0, (name, lds)
        body = kernel_body(asm, name, ".Lfunc_end")
        assert "scratch_" not in body and "ds_" not in body, name
        if "k_ulog_write" in name:
            assert occ >= 4, (name, occ)
            stores = re.findall(r"\b(global_store_\w+|flat_store_\w+|buffer_store_\w+)", body)
            # the rows leave as 16-byte pieces (and the 32-byte directory entry as two); the only narrower store is the scene's
            # `fresh` flag, one dword -- no object goes out by dword, dwordx2 or dwordx3
            assert stores.count("global_store_dwordx4") >= 1, stores
            assert sorted(set(stores) - {"global_store_dwordx4"}) == ["global_store_dword"] and stores.count("global_store_dword") == 1, stores
            assert "global_load_dwordx3" in body, name   # a wire object arrives as one 12-byte load


def _export(frames):
    """A hand-made export: frames = [(scene, frame_number, t, rows[k, 6])] -> (dir, rows) as radar_log_host returns them."""
    d = np.zeros(len(frames), _lib.UART_FRAME_DTYPE)
    rows = np.zeros(sum(len(f[3]) for f in frames), _lib.UART_OBJECT_DTYPE)
    first = 0
    for i, (scene, fn, t, r) in enumerate(frames):
        d[i] = (scene, fn, first, len(r), t, 9, 0)
        for c, name in enumerate(FIELDS_O):
            rows[name][first: first + len(r)] = np.asarray(r, np.float64).reshape(-1, 6)[:, c]
        first += len(r)
    return d, rows


def _objects(rng, k):
    r = np.zeros((k, 6))
    r[:, 0:3] = rng.integers(-3000, 3000, (k, 3)) / 512.0
    r[:, 3] = rng.integers(-12, 13, k) * 0.1252
    r[:, 4] = rng.integers(0, 5000, k)
    r[:, 5] = rng.integers(0, 200, k) * 0.0436
    return r


def _lines(path):
    with open(path) as fh:
        return fh.read().splitlines()


def test_logger_shards_flushes_and_zero_object_frames(tmp_path, monkeypatch):
    """write_thread's bookkeeping with small limits: a flush when the buffer holds FB_WRITE_BUFFER_SIZE ROWS, a flush and the
    next shard after FB_EXPERIMENT_FILE_SIZE FRAMES, a zero-object frame that adds no row but counts, close() for the rest;
    frames of a scene without a path are ignored, two scenes keep separate books."""
    from mmwave_msc_amd import constants as const
    from mmwave_msc_amd.radar import ExperimentLogger
    monkeypatch.setattr(const, "FB_WRITE_BUFFER_SIZE", 7)
    monkeypatch.setattr(const, "FB_EXPERIMENT_FILE_SIZE", 4)
    rng = np.random.default_rng(3)
    pa, pb = tmp_path / "a", tmp_path / "b"
    pa.mkdir(); pb.mkdir()
    lg = ExperimentLogger({5: str(pa), 6: str(pb)})
    counts = [3, 3, 0, 2, 1, 9, 2]                     # scene 5, frames 1 .. 7
    for f, k in enumerate(counts, start=1):
        frames = [(5, f, 100.0 + f, _objects(rng, k)), (9, f, 1.0, _objects(rng, 2))]
        if f == 2:
            frames.append((6, 77, 5.0005, _objects(rng, 1)))
        lg.write(*_export(frames))
        rows_on_disk = len(_lines(pa / "1.csv")) if (pa / "1.csv").exists() else 0
        if f == 1:
            assert rows_on_disk == 0                   # 3 rows < 7: buffered
        if f == 3:
            assert rows_on_disk == 0                   # 6 rows, three frames
        if f == 4:
            assert rows_on_disk == 8                   # 8 rows >= 7 AND the fourth frame: flushed, shard 2 begins
    assert not (pa / "3.csv").exists()
    assert len(_lines(pa / "2.csv")) == 10             # frame 5 (1 row: buffered), frame 6 (10 rows >= 7: flushed); frame 7 buffered
    assert not (pb / "1.csv").exists()                 # one row of scene 6: still buffered
    lg.close()
    assert len(_lines(pa / "2.csv")) == 12 and len(_lines(pb / "1.csv")) == 1
    assert lg.frames_written == {5: 7, 6: 1}
    first = _lines(pa / "1.csv")
    assert [int(l.split(",")[0]) for l in first] == [1, 1, 1, 2, 2, 2, 4, 4]      # frame 3 wrote no row
    assert _lines(pb / "1.csv")[0].split(",")[0] == "77" and _lines(pb / "1.csv")[0].split(",")[6] == str(round(5.0005 * 1000))
    assert sorted(os.listdir(tmp_path)) == ["a", "b"]  # scene 9 has no path: nothing of it anywhere


def test_logger_files_read_back_through_offline_manager_bit_for_bit(tmp_path):
    """39 frames numbered from 1 (below OfflineManager's refill quirk at frame 40), 0 .. 11 objects each, with the product's own
    limits: every x, y, z, doppler, peakVal and posix that OfflineManager returns equals the exported value bit for bit."""
    from mmwave_msc_amd.radar import ExperimentLogger
    from mmwave_msc_amd.utils import OfflineManager
    from tests._uart_recording import same_bits
    rng = np.random.default_rng(11)
    F = 39
    sent = {}
    lg = ExperimentLogger({0: str(tmp_path)})
    for f in range(1, F + 1):
        k = 0 if f in (7, 20) else int(rng.integers(1, 12))
        r = _objects(rng, k)
        r[:, 0:3] += rng.random((k, 3)) * 1e-3          # (digits that need all 17 significant figures)
        t = 1.7e9 + 0.1 * f + float(rng.random()) * 1e-3
        sent[f] = (r, round(t * 1000))
        lg.write(*_export([(0, f, t, r)]))
    lg.close()
    om = OfflineManager(str(tmp_path))
    seen = 0
    for f in range(1, F + 1):
        ok, fn, data = om.get_data()
        r, stamp = sent[f]
        assert fn == f and ok == (len(r) > 0), (f, ok)
        if not ok:
            continue
        seen += 1
        for c, key in enumerate(("x", "y", "z", "doppler", "peakVal")):
            assert same_bits(np.asarray(data[key], np.float64), r[:, c]), (f, key)
        assert list(data["posix"]) == [stamp] * len(r), f
    assert seen == F - 2


def test_logger_text_is_the_reference_writers_text(tmp_path):
    """The pandas statements of DataLogging.py's write_thread (60-82), typed here as data flow, on one frame: the same bytes on
    disk as ExperimentLogger leaves for that frame."""
    import pandas as pd
    from mmwave_msc_amd.radar import ExperimentLogger
    rng = np.random.default_rng(4)
    r = _objects(rng, 6)
    r[:, 0:3] += rng.random((6, 3)) * 1e-5
    t = 1712345678.4567
    det = {"x": r[:, 0].copy(), "y": r[:, 1].copy(), "z": r[:, 2].copy(), "doppler": r[:, 3].copy(), "peakVal": r[:, 4].astype(np.int16),
           "timestamp": round(t * 1000)}                # ReadDataIWR1443.py:160-171
    data = {"Frame": 31, "X": det["x"], "Y": det["y"], "Z": det["z"], "Doppler": det["doppler"], "Intensity": det["peakVal"],
            "Timestamp": det["timestamp"]}
    data_buffer = pd.DataFrame()
    df = pd.DataFrame(data)
    data_buffer = pd.concat([data_buffer, df], ignore_index=True)
    want = io.StringIO()
    pd.DataFrame(data_buffer).to_csv(want, mode="a", index=False, header=False)
    lg = ExperimentLogger({2: str(tmp_path)})
    lg.write(*_export([(2, 31, t, r)]))
    lg.close()
    with open(tmp_path / "1.csv", newline="") as fh:
        got = fh.read()
    assert got == want.getvalue() and got.count("\n") == 6
    assert got.splitlines()[0].split(",")[5] == str(int(r[0, 4])) and got.splitlines()[0].endswith(",1712345678457")
