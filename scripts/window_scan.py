"""Column-window range scan against the row scan on the C4 workload as bench.py defines it (100M
YCSB rows, 2^18 scans of 100 records per step, start keys fastrandom(seed) % rows): one table,
one process, every shape warmed, the shapes timed with device events in alternating rounds --

    rows            stage_scan_batch (the C4 leg's shape)
    win100          stage_scan_batch_window (100, 100): one YCSB column, source byte 108
    win4            stage_scan_batch_window (0, 4): the first 4 payload bytes (stock-level's OL_I_ID)
    win1000         stage_scan_batch_window (0, 1000): the whole payload
    <window>_keys   the same with d_row_keys (8 more bytes written per record)

Prints one JSON line (and appends it to --out): per shape min / median / max, the per-round
times, whether win100 and win4 beat the row scan in every round, and the bytes per scan each
shape moves by construction.  The window outputs are checked against the row form's bytes on the
way."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stage-indexorganized_amd"))
import stage  # noqa: E402
from stage._lib import check as stage_check  # noqa: E402

KEY_PAD = 8
WINDOWS = {"win100": (100, 100), "win4": (0, 4), "win1000": (0, 1000)}


def stats(v, digits=4):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), digits), "median": round(float(np.median(v)), digits),
            "max": round(float(v.max()), digits)}


def window_heap_bytes(window, unit):
    """bytes of the aligned `unit`-B pieces of a heap row that hold the window"""
    s = KEY_PAD + window[0]
    return ((s + window[1] + unit - 1) // unit - s // unit) * unit


def scan_bytes(tab, size):
    """per scan of `size` records, from the shapes: heap bytes read for the output (16-B loads; in
    brackets the 128-B lines they lie in) and output bytes written.  The index bytes every shape
    reads alike (separator nodes, leaf heads, key columns, slot words) are not counted.  The keys
    of a *_keys shape come from the head of the heap row: 8 more bytes read, in the row's first
    128-B line."""
    b = {"rows": {"heap_read": size * tab.stride, "heap_lines_128B": size * tab.stride, "out_write": size * tab.stride}}
    for name, w in WINDOWS.items():
        b[name] = {"heap_read": size * window_heap_bytes(w, 16), "heap_lines_128B": size * window_heap_bytes(w, 128),
                   "out_write": size * stage.window_stride(w[1])}
        lines = size * (window_heap_bytes(w, 128) + (128 if KEY_PAD + w[0] >= 128 else 0))
        b[name + "_keys"] = {"heap_read": b[name]["heap_read"] + size * KEY_PAD, "heap_lines_128B": lines,
                             "out_write": b[name]["out_write"] + size * KEY_PAD}
    for v in b.values():
        v["total"] = 8 + 4 + v["heap_read"] + v["out_write"]  # start key in, count out
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--scans", type=int, default=1 << 18, help="scans per step (bench.py's --scan-batch)")
    ap.add_argument("--scan-size", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None, help="file the JSON line is appended to")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.steps >= 1
    if stage.device_count() < 1:
        raise SystemExit("no HIP device: this script measures on the GPU only")

    B, size = args.scans, args.scan_size
    t0 = time.time()
    tab = stage.Table(key_width=8)
    tab.load_ycsb(0, args.rows, 8, mode=0)
    tab.sync()
    starts = (stage.fastrandom(args.seed, B) % np.uint64(args.rows)).astype(np.uint64)
    print(f"table of {args.rows} rows and {B} start keys ready in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    s = stage.Stream()
    d_keys = stage.DeviceBuffer.from_numpy(starts)
    d_cnt = stage.DeviceBuffer(B * 4)
    d_rec = stage.DeviceBuffer(B * size * tab.stride)  # rows, or the windows (never larger)
    d_rk = stage.DeviceBuffer(B * size * KEY_PAD)
    L = stage.lib()

    def rows():
        stage_check(L.stage_scan_batch(tab.h, d_keys.ptr, None, B, size, d_cnt.ptr, d_rec.ptr, s.ptr), "scan")

    def window(w, keys):
        return lambda: tab.scan_device_window(d_keys.ptr, B, size, w, d_cnt.ptr, d_rec.ptr,
                                              d_row_keys=d_rk.ptr if keys else None, stream=s.ptr)

    shapes = {"rows": rows}
    for name, w in WINDOWS.items():
        shapes[name] = window(w, False)
        shapes[name + "_keys"] = window(w, True)

    # warm every shape, and check the windows and keys against the row form on the batch's first
    # and last scans
    k = min(B, 256)
    offs = (0, B - k)
    check = {}
    rows()
    s.sync()
    ref_cnt = d_cnt.to_numpy(np.uint32, B)
    ref_rows = [d_rec.to_numpy(np.uint8, k * size * tab.stride, offset=o * size * tab.stride).reshape(k, size, tab.stride)
                for o in offs]
    check["rows"] = bool((ref_cnt > 0).all() and (ref_cnt == size).mean() > 0.99)  # bench.py's self check
    for name, launch in shapes.items():
        if name == "rows":
            continue
        w = WINDOWS[name.replace("_keys", "")]
        ws = stage.window_stride(w[1])
        d_rk.memset(0, stream=s.ptr)
        launch()
        s.sync()
        ok = d_cnt.to_numpy(np.uint32, B).tobytes() == ref_cnt.tobytes()
        for j, o in enumerate(offs):
            live = np.arange(size)[None, :] < ref_cnt[o:o + k, None]
            win = d_rec.to_numpy(np.uint8, k * size * ws, offset=o * size * ws).reshape(k, size, ws)
            ok = ok and np.array_equal(win[:, :, :w[1]][live], ref_rows[j][:, :, KEY_PAD + w[0]:KEY_PAD + w[0] + w[1]][live])
            ok = ok and not win[:, :, w[1]:][live].any()
            if name.endswith("_keys"):
                rk = d_rk.to_numpy(np.uint8, k * size * KEY_PAD, offset=o * size * KEY_PAD).reshape(k, size, KEY_PAD)
                ok = ok and np.array_equal(rk[live], ref_rows[j][:, :, :KEY_PAD][live])
        check[name] = bool(ok)

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
    sbytes = scan_bytes(tab, size)
    device = {name: {"step_ms": stats(v), "rounds_ms": [round(x, 4) for x in v],
                     "mscans_s": round(B / np.median(v) / 1e3, 3), "bytes_per_scan": sbytes[name]}
              for name, v in ms.items()}
    faster = {name: bool(all(a < b for a, b in zip(ms[name], ms["rows"]))) for name in shapes if name != "rows"}

    line = json.dumps({
        "script": "window_scan", "rows": args.rows, "scans_per_step": B, "scan_size": size, "seed": args.seed,
        "starts": "fastrandom(seed) % rows", "rounds": args.rounds, "steps_per_round": args.steps, "windows": WINDOWS,
        "device": device, "faster_than_rows_in_every_round": faster,
        "delivers": {"rows": "key + 1000-B payload per record", "win100": "payload bytes 100..199",
                     "win4": "payload bytes 0..3", "win1000": "payload bytes 0..999",
                     "*_keys": "the window and the record's 8 key bytes"},
        "check_equal": check, "version": L.stage_version().decode()})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(check.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
