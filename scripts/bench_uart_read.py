"""What the device-resident radar readers cost, at the benchmark's shape (4096 scenes x 512 objects): k_uart_read -- read() and
normalize_data for every scene, buffer discipline included -- against k_normalize_tlv on the same bodies, which needs the host
to have found every packet first.

    python scripts/bench_uart_read.py [--scenes 4096] [--pts 512] [--reps 5] [--out profiles/uart_read_bench.json]

Steady state: every scene's chunk is one whole packet (magic word, header, detected-points TLV with --pts objects, padded to 32
bytes), so the reader appends it to an empty buffer, finds the magic word at 0, decodes, and drops the packet -- both moves
are empty.  After a warm-up call of each, --reps times and ALTERNATING which goes first:
  uart_read      mmw_uart_read on the chunk block (offsets [S + 1] already on the device)
  normalize_tlv  mmw_normalize_tlv on the same block with each body's offset
each between two device events on the context's stream (idle before the first).  `find_tlv_host_us` is what the reader removes
from the host: S calls of mmw_find_tlv (one per packet, as a host that keeps the byte buffers itself makes them) plus the
upload of the S offsets.  Best and median in microseconds; no threshold is asserted, the ratio is quoted in profiles/README.md."""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--pts", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uart_read_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from mmwave_msc_amd import _lib, radar
    from mmwave_msc_amd.batch import SceneBatch
    if not torch.cuda.is_available():
        raise SystemExit("bench_uart_read.py measures on the GPU: no device, no number")
    S, N, R = a.scenes, a.pts, a.reps
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
    sb = SceneBatch(_lib.default_config(), S, N)
    st = torch.cuda.Stream(device=dev)
    sb.follow_torch_stream(st)
    sb.open_radars(cfgp, t0=0.0)
    ucfg = radar.uart_cfg(cfgp)
    d_chunks = torch.from_numpy(packets.reshape(-1)).to(dev)
    chunk_off = np.arange(S + 1, dtype=np.int64) * total
    d_off = torch.from_numpy(chunk_off).to(dev)
    d_body = torch.from_numpy(chunk_off[:S] + 44).to(dev)
    mk = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    pts_r, pts_t = mk(S * N * 8, torch.float64), mk(S * N * 8, torch.float64)
    n_r, n_t, dt_r, st_r, fr_r = mk(S, torch.int32), mk(S, torch.int32), mk(S, torch.float64), mk(S, torch.int32), mk(S, torch.int32)
    clock = [0.0]

    def uart_read():
        clock[0] += 0.1
        sb.read_radars_dev(d_chunks.data_ptr(), d_off.data_ptr(), S * total, clock[0], pts_r.data_ptr(), n_r.data_ptr(), dt_r.data_ptr(),
                           st_r.data_ptr(), fr_r.data_ptr())

    def normalize_tlv():
        sb.normalize_tlv_dev(d_chunks.data_ptr(), S * total, d_body.data_ptr(), ucfg, pts_t.data_ptr(), n_t.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        with torch.cuda.stream(st):
            e0.record(st)
            fn()
            e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for fn in (uart_read, normalize_tlv, uart_read, normalize_tlv):
        timed(fn)
    t = {"uart_read": [], "normalize_tlv": []}
    for r in range(R):
        for which in (("uart_read", "normalize_tlv") if r % 2 == 0 else ("normalize_tlv", "uart_read")):
            t[which].append(timed(uart_read if which == "uart_read" else normalize_tlv))
    st.synchronize()
    # the two paths gave the same rows, every scene decoded, and the readers are back in their steady state
    assert bool((st_r == _lib.UART_POINTS).all()) and torch.equal(n_r, n_t) and torch.equal(pts_r, pts_t)
    assert sb.radar_state(S - 1)[1] == 0
    host = []
    for r in range(R):
        t0 = time.perf_counter()
        offs = np.empty(S, dtype=np.int64)
        for s in range(S):
            found, off, n_obj, _, _, _ = radar.find_tlv(packets[s])
            offs[s] = s * total + off if found else -1
        torch.from_numpy(offs).to(dev)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    kept = int(n_r.sum().item())
    summ = lambda v: {"best": min(v), "median": float(np.median(v)), "all": v}
    res = {"workload": f"{S} scenes x {N} objects, one {total}-byte packet per chunk", "reps": R,
           "timing": "device events on the context's stream, idle before the first; microseconds",
           "lib": _lib.load().mmw_version().decode(), "device": torch.cuda.get_device_name(0),
           "uart_read_us": summ(t["uart_read"]), "normalize_tlv_us": summ(t["normalize_tlv"]),
           "ratio_best": min(t["uart_read"]) / min(t["normalize_tlv"]),
           "ratio_median": float(np.median(t["uart_read"]) / np.median(t["normalize_tlv"])),
           "find_tlv_host_us": summ(host), "rows_kept": kept, "wire_bytes": S * total, "row_bytes_written": kept * 64}
    sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
