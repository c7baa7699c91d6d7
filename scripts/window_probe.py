"""Column-window probe against the full-row and status-only probes on the C2 workload (100M YCSB
rows, 2^24 Zipf-0.9 keys per step, seeded): one table, one process, every shape warmed, the
shapes timed with device events in alternating rounds --

    rows         stage_probe_batch with d_records (the headline shape)
    win100       stage_probe_batch_window (100, 100): one YCSB column, source byte 108
    win1000      stage_probe_batch_window (0, 1000): the whole payload
    status       stage_probe_batch with d_records == NULL: the floor of the window shapes

-- then the host path: stage_probe_host against stage_probe_host_window (100, 100), pinned
buffers, the lean layout of bench.py's end-to-end leg (stage_set_output_layout(1008, 16)).
Prints one JSON line (and appends it to --out): per shape min / median / max and the bytes each
lookup moves, computed from the shapes.  The window outputs are checked against the row form's
bytes on the way."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stage-indexorganized_amd"))
import stage  # noqa: E402

KEY_PAD = 8
WINDOWS = {"win100": (100, 100), "win1000": (0, 1000)}


def stats(v, digits=4):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), digits), "median": round(float(np.median(v)), digits),
            "max": round(float(v.max()), digits)}


def window_heap_bytes(window, unit):
    """bytes of the aligned `unit`-B pieces of a heap row that hold the window"""
    s = KEY_PAD + window[0]
    return ((s + window[1] + unit - 1) // unit - s // unit) * unit


def device_bytes(tab, status_bytes):
    """per lookup, from the shapes: key in, status record out, heap bytes read for the output
    (16-B loads; in brackets the 128-B lines they lie in), output bytes written.  The index
    bytes every shape reads alike (separator nodes, leaf head, slot words) are not counted."""
    b = {"rows": {"key": 8, "status": status_bytes, "heap_read": tab.stride, "heap_lines_128B": tab.stride,
                  "out_write": tab.stride},
         "status": {"key": 8, "status": status_bytes, "heap_read": 0, "heap_lines_128B": 0, "out_write": 0}}
    for name, w in WINDOWS.items():
        b[name] = {"key": 8, "status": status_bytes, "heap_read": window_heap_bytes(w, 16),
                   "heap_lines_128B": window_heap_bytes(w, 128), "out_write": stage.window_stride(w[1])}
    for v in b.values():
        v["total"] = v["key"] + v["status"] + v["heap_read"] + v["out_write"]
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--theta", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-chunk", type=int, default=1 << 22, help="lookups per host-path call")
    ap.add_argument("--host-rounds", type=int, default=5, help="passes over the batch per host shape")
    ap.add_argument("--out", default=None, help="file the JSON line is appended to")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.steps >= 1
    if stage.device_count() < 1:
        raise SystemExit("no HIP device: this script measures on the GPU only")

    B = args.batch
    t0 = time.time()
    tab = stage.Table(key_width=8)
    tab.load_ycsb(0, args.rows, 8, mode=0)
    tab.sync()
    draws = stage.zipf_draws(args.rows - 1, args.theta, args.seed, B, nthreads=min(16, os.cpu_count() or 4))
    print(f"table of {args.rows} rows and {B} keys ready in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    s = stage.Stream()
    d_keys = stage.DeviceBuffer.from_numpy(draws)
    d_out = stage.DeviceBuffer(B * 32)
    d_rec = stage.DeviceBuffer(B * tab.stride)  # rows, or the windows (never larger)
    shapes = {
        "rows": lambda: tab.probe_device(d_keys.ptr, B, d_out.ptr, d_rec.ptr, stream=s.ptr),
        "win100": lambda: tab.probe_device_window(d_keys.ptr, B, WINDOWS["win100"], d_out.ptr, d_rec.ptr, stream=s.ptr),
        "win1000": lambda: tab.probe_device_window(d_keys.ptr, B, WINDOWS["win1000"], d_out.ptr, d_rec.ptr,
                                                   stream=s.ptr),
        "status": lambda: tab.probe_device(d_keys.ptr, B, d_out.ptr, None, stream=s.ptr),
    }
    # warm every shape, and check the windows against the row form (mode-0 rows: every payload
    # byte is the key's low byte) on the batch's first and last lookups
    k = min(B, 4096)
    check = {}
    shapes["rows"]()
    s.sync()
    ref_out = [d_out.to_numpy(np.uint8, k * 32, offset=o * 32) for o in (0, B - k)]
    ref_rows = [d_rec.to_numpy(np.uint8, k * tab.stride, offset=o * tab.stride).reshape(k, tab.stride)
                for o in (0, B - k)]
    for name, w in WINDOWS.items():
        shapes[name]()
        s.sync()
        ws = stage.window_stride(w[1])
        ok = True
        for j, o in enumerate((0, B - k)):
            win = d_rec.to_numpy(np.uint8, k * ws, offset=o * ws).reshape(k, ws)
            ok = ok and np.array_equal(win[:, :w[1]], ref_rows[j][:, KEY_PAD + w[0]:KEY_PAD + w[0] + w[1]])
            ok = ok and not win[:, w[1]:].any()
            ok = ok and d_out.to_numpy(np.uint8, k * 32, offset=o * 32).tobytes() == ref_out[j].tobytes()
            ok = ok and bool((win[:, :w[1]] == (draws[o:o + k] & np.uint64(0xFF)).astype(np.uint8)[:, None]).all())
        check[name] = bool(ok)
    shapes["status"]()
    s.sync()

    e0, e1 = stage.Event(), stage.Event()
    ms = {name: [] for name in shapes}
    for _ in range(args.rounds):
        for name, launch in shapes.items():
            e0.record(s)
            for _ in range(args.steps):
                launch()
            e1.record(s)
            s.sync()
            ms[name].append(e0.elapsed_ms(e1) / args.steps)
    dbytes = device_bytes(tab, 32)
    device = {name: {"step_ms": stats(v), "glookups_s": round(B / np.median(v) / 1e6, 3),
                     "bytes_per_lookup": dbytes[name]} for name, v in ms.items()}
    del d_rec, d_out, d_keys

    # host path: pinned keys and result rings, lean layout, alternating passes over the batch
    chunk = min(B, args.host_chunk)
    tab.set_output_layout(1008, 16)
    w = WINDOWS["win100"]
    ws = stage.window_stride(w[1])
    keys = stage.pinned_empty(B, np.uint64)
    keys[:] = draws
    out = stage.pinned_empty(chunk, stage.PROBE_OUT16_DTYPE)
    rows = stage.pinned_empty((chunk, tab.stride), np.uint8)
    win = stage.pinned_empty((chunk, ws), np.uint8)
    host_shapes = {
        "probe_host": lambda b: tab.probe_host(keys[b:b + chunk], out=out, rows=rows),
        "probe_host_window": lambda b: tab.probe_host(keys[b:b + chunk], out=out, rows=win, window=w),
    }
    starts = list(range(0, B - chunk + 1, chunk))
    for call in host_shapes.values():  # warm: the pipe's device buffers
        call(starts[-1])
    check["probe_host_window"] = bool(
        np.array_equal(win[:k, :w[1]], rows[:k, KEY_PAD + w[0]:KEY_PAD + w[0] + w[1]]) and not win[:k, w[1]:].any())
    rate = {name: [] for name in host_shapes}
    for _ in range(args.host_rounds):
        for name, call in host_shapes.items():
            t0 = time.perf_counter()
            for b in starts:
                call(b)
            rate[name].append(len(starts) * chunk / (time.perf_counter() - t0))
    d2h = {"probe_host": 16 + tab.stride, "probe_host_window": 16 + ws}
    host = {name: {"lookups_s": stats(v, 1), "pcie_bytes_per_lookup": {"h2d": 8, "d2h": d2h[name]},
                   "pcie_d2h_gbs": round(float(np.median(v)) * d2h[name] / 1e9, 2)} for name, v in rate.items()}
    tab.set_output_layout(0, 32)

    line = json.dumps({
        "script": "window_probe", "rows": args.rows, "batch": B, "theta": args.theta, "seed": args.seed,
        "rounds": args.rounds, "steps_per_round": args.steps, "windows": WINDOWS, "device": device,
        "host": host, "host_chunk": chunk, "host_rounds": args.host_rounds,
        "host_layout": "stage_set_output_layout(1008, 16): 16-B status records; packed 1008-B rows / 112-B windows",
        "delivers": {"rows": "key + 1000-B payload", "win100": "payload bytes 100..199",
                     "win1000": "payload bytes 0..999", "status": "status record only"},
        "check_equal": check, "version": stage.lib().stage_version().decode()})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(check.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
