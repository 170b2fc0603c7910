"""What the radar log costs, at the benchmark's shape (4096 scenes x 512 objects, one packet per chunk, as bench_uart_read.py):

  (a) k_uart_read of this build against another build's (--parent-tree: a checkout of the parent commit with its library built),
      each measured by ITS OWN scripts/bench_uart_read.py in a fresh process, alternating -- the log must not have moved it
  (b) k_uart_read_log (the log enabled) against k_uart_read (a second context without it) on the same chunks, in this process
  (c) mmw_uart_log -- count, scan, write and the copy of the counts -- against a device-to-device copy of exactly the bytes it
      writes (a 32-byte directory entry per scene and 48 bytes per object), in this process

    python scripts/bench_uart_log.py [--scenes 4096] [--pts 512] [--reps 7] [--parent-tree DIR] [--out profiles/uart_log_bench.json]

(b) and (c): after a warm-up of each, --reps times and ALTERNATING which goes first, each between two device events on the
context's stream (idle before the first).  Every export of (c) follows a read that staged a fresh frame in every scene (the read
is not timed).  Best and median in microseconds; no threshold is asserted, the ratios are quoted in profiles/README.md."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reader_in_fresh_processes(trees, scenes, pts, reps, rounds):
    """[(tree, uart_read_us of one run of its bench_uart_read.py)] -- `rounds` runs per tree, alternating"""
    out = []
    with tempfile.TemporaryDirectory() as d:
        for r in range(rounds):
            for tree in (trees if r % 2 == 0 else trees[::-1]):
                path = os.path.join(d, "r.json")
                subprocess.run([sys.executable, os.path.join(tree, "scripts", "bench_uart_read.py"), "--scenes", str(scenes), "--pts", str(pts),
                                "--reps", str(reps), "--out", path], check=True, cwd=tree, stdout=subprocess.DEVNULL, timeout=600)
                with open(path) as fh:
                    res = json.load(fh)
                out.append((tree, res["uart_read_us"], res["lib"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="(a): fresh processes per build")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uart_log_bench.json"))
    a = ap.parse_args()
    import numpy as np
    S, N, R = a.scenes, a.pts, a.reps
    summ = lambda v: {"best": min(v), "median": float(np.median(v)), "all": list(v)}
    res = {"workload": f"{S} scenes x {N} objects, one packet per chunk", "reps": R,
           "timing": "device events on the context's stream, idle before the first; microseconds"}
    if a.parent_tree:   # (before this process touches the GPU itself)
        runs = reader_in_fresh_processes([os.path.abspath(a.parent_tree), ROOT], S, N, R, a.rounds)
        for key, tree in (("parent", os.path.abspath(a.parent_tree)), ("branch", ROOT)):
            mine = [r for r in runs if r[0] == tree]
            res["a_uart_read_" + key] = {"lib": mine[0][2], "best_us": [r[1]["best"] for r in mine], "median_us": [r[1]["median"] for r in mine]}
        pa, br = res["a_uart_read_parent"], res["a_uart_read_branch"]
        res["a_ratio_of_medians"] = float(np.median(br["median_us"]) / np.median(pa["median_us"]))
        res["a_ratio_of_bests"] = min(br["best_us"]) / min(pa["best_us"])

    import torch
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_uart_log.py measures on the GPU: no device, no number")
    cfgp = {"rangeIdxToMeters": 0.0436, "dopplerResolutionMps": 0.1252, "numDopplerBins": 32.0}
    rng = np.random.default_rng(0)
    raw = np.zeros((S, N, 5))
    raw[..., 0] = rng.uniform(-3, 3, (S, N))
    raw[..., 1] = rng.uniform(0.3, 6, (S, N))
    raw[..., 2] = rng.uniform(-1.5, 0.5, (S, N))
    raw[..., 3] = rng.uniform(-2, 2, (S, N))
    raw[..., 4] = rng.uniform(0, 3000, (S, N))
    bodies = radar.encode_tlv_bodies(raw, np.full(S, N), 9, cfgp["dopplerResolutionMps"], stride=4 + 12 * N)
    total = (48 + 12 * N + 31) // 32 * 32
    packets = np.zeros((S, total), dtype=np.uint8)
    for s in range(S):
        head = bytes([2, 1, 4, 3, 6, 5, 8, 7]) + struct.pack("<IIIIIIIII", 0x01020304, total, 0xA1443, s, 1, N, 1, 1, 4 + 12 * N)
        packets[s, :44] = np.frombuffer(head, dtype=np.uint8)
        packets[s, 44: 48 + 12 * N] = bodies[s]
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    ctx = {}
    for name in ("plain", "log"):
        sb = SceneBatch(_lib.default_config(), S, N)
        sb.follow_torch_stream(st)
        sb.open_radars(cfgp, t0=0.0)
        ctx[name] = sb
    ctx["log"].enable_radar_log()
    d_chunks = torch.from_numpy(packets.reshape(-1)).to(dev)
    d_off = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * total).to(dev)
    mk = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    outs = {name: (mk(S * N * 8, torch.float64), mk(S, torch.int32), mk(S, torch.float64), mk(S, torch.int32), mk(S, torch.int32)) for name in ctx}
    fdt, odt = _lib.UART_FRAME_DTYPE.itemsize, _lib.UART_OBJECT_DTYPE.itemsize
    log_bytes = S * fdt + S * N * odt
    d_dir, d_rows = mk(S * fdt, torch.uint8), mk(S * N * odt, torch.uint8)
    copy_src, copy_dst = torch.randint(0, 255, (log_bytes,), dtype=torch.uint8, device=dev), mk(log_bytes, torch.uint8)
    clock = [0.0]

    def read(name):
        clock[0] += 0.1
        o = outs[name]
        ctx[name].read_radars_dev(d_chunks.data_ptr(), d_off.data_ptr(), S * total, clock[0], *[t.data_ptr() for t in o])

    def export():
        ctx["log"].radar_log_dev(d_dir.data_ptr(), S, d_rows.data_ptr(), S * N, ticket=0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    # (b) the twin against the reader
    for name in ("plain", "log", "plain", "log"):
        timed(lambda: read(name))
    t = {"plain": [], "log": []}
    for r in range(R):
        for name in (("plain", "log") if r % 2 == 0 else ("log", "plain")):
            t[name].append(timed(lambda: read(name)))
    st.synchronize()
    for k in range(5):
        assert torch.equal(outs["plain"][k], outs["log"][k]) or k == 2, k   # (dt differs: the two contexts read at different times)
    assert bool((outs["log"][3] == _lib.UART_POINTS).all())
    kept = int(outs["log"][1].sum().item())
    res["b_uart_read_us"], res["b_uart_read_log_us"] = summ(t["plain"]), summ(t["log"])
    res["b_ratio_best"] = min(t["log"]) / min(t["plain"])
    res["b_ratio_median"] = float(np.median(t["log"]) / np.median(t["plain"]))
    res["b_bytes"] = {"wire": S * total, "rows_written": kept * 64, "log_written": S * N * 12 + S * 32}

    # (c) the export against a copy of the bytes it writes
    def copy():
        with torch.cuda.stream(st):
            copy_dst.copy_(copy_src, non_blocking=True)

    def one_export():
        read("log")               # a fresh frame in every scene (not timed)
        us = timed(export)
        assert ctx["log"].radar_log_wait(0) == (S, S * N)
        return us

    one_export(); timed(copy); one_export(); timed(copy)
    t = {"export": [], "copy": []}
    for r in range(R):
        for which in (("export", "copy") if r % 2 == 0 else ("copy", "export")):
            t[which].append(one_export() if which == "export" else timed(copy))
    st.synchronize()
    d = np.frombuffer(d_dir.cpu().numpy().tobytes(), _lib.UART_FRAME_DTYPE)
    assert list(d["scene"][:3]) == [0, 1, 2] and int(d["count"].sum()) == S * N and int(d["first"][-1]) == (S - 1) * N
    res["c_uart_log_us"], res["c_copy_us"] = summ(t["export"]), summ(t["copy"])
    res["c_bytes"] = log_bytes
    res["c_copy_over_export_best"] = min(t["copy"]) / min(t["export"])
    res["c_copy_over_export_median"] = float(np.median(t["copy"]) / np.median(t["export"]))
    res["lib"] = _lib.load().mmw_version().decode()
    res["device"] = torch.cuda.get_device_name(0)
    for sb in ctx.values():
        sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
