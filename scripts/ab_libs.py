"""A/B of the probe across builds: each --pkg is a package directory (holding stage/ and
lib/libstage_hip.so, e.g. a copy of an older commit's build); the bench workload (100M rows,
2^24 Zipf-0.9 lookups) is timed with events, one process per package, so each run gets its
own table.  Prints one JSON line with the median launch time and an output digest.

--mode window times the column-window range scans instead (stage_scan_batch_window and
stage_index_scan_batch_window, --scan-size records per scan) on a table of the given geometry:
--key-width, --payload and --leaf-size select the scan_window_kernel instance (16-byte keys:
two key words; 40-byte payloads in 64-KiB leaves: 1024 slots).  Keys are big-endian row numbers
loaded in order, start keys random rows; the JSON line carries every launch's time per entry point."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pkg", required=True)
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--batch", type=int, default=1 << 24)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--theta", type=float, default=0.9)
ap.add_argument("--mode", choices=["probe", "scan", "window"], default="probe")
ap.add_argument("--scan-size", type=int, default=100)
ap.add_argument("--key-width", type=int, default=8, help="window mode: key bytes (8, 16, 24 or 32)")
ap.add_argument("--payload", type=int, default=40, help="window mode: payload bytes")
ap.add_argument("--leaf-size", type=int, default=64 * 1024, help="window mode: leaf node bytes")
ap.add_argument("--window", default="0,16", help="window mode: payload_off,len")
args = ap.parse_args()
if args.mode == "scan" and args.batch == 1 << 24:
    args.batch = 1 << 18
if args.mode == "window":
    if args.batch == 1 << 24:
        args.batch = 1 << 16
    if args.rows == 100_000_000:
        args.rows = 2_000_000

sys.path.insert(0, os.path.abspath(args.pkg))
import stage  # noqa: E402
from stage._lib import check  # noqa: E402

s = stage.Stream()
e0, e1 = stage.Event(), stage.Event()


def timed(step):
    step()
    ms = []
    for r in range(args.rounds):
        e0.record(s)
        step()
        e1.record(s)
        s.sync()
        ms.append(e0.elapsed_ms(e1))
    return ms


def window_mode():
    n, w, size, B = args.rows, args.key_width, args.scan_size, args.batch
    window = tuple(int(v) for v in args.window.split(","))
    keys = np.zeros((n, w), np.uint8)
    keys[:, w - 8:] = np.arange(n, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    tab = stage.Table(payload_size=args.payload, leaf_node_size=args.leaf_size, key_width=w)
    _, ins = tab.load_rows(keys, np.random.default_rng(1).integers(0, 256, (n, args.payload), dtype=np.uint8))
    assert ins == n
    tab.sync()
    starts = keys[stage.fastrandom(0x5EED, B) % np.uint64(n)]
    dk = stage.DeviceBuffer.from_numpy(tab.key_buffer(starts)[0])
    ws, kp = stage.window_stride(window[1]), (w + 7) // 8 * 8
    dc, dw = stage.DeviceBuffer(B * 4), stage.DeviceBuffer(B * size * ws)
    dkey, dst = stage.DeviceBuffer(B * size * kp), stage.DeviceBuffer(B * size)
    res = {"pkg": args.pkg, "mode": "window", "key_width": w, "payload": args.payload, "leaf_slots": tab.leaf_capacity,
           "key_words": tab.key_words, "rows": n, "scans": B, "scan_size": size, "window": window}
    h = hashlib.sha1()
    for name, st in (("scan", None), ("index_scan", dst.ptr)):
        for b in (dc, dw, dkey, dst):  # positions past a scan's count are not written
            b.memset(0, stream=s.ptr)
        ms = timed(lambda: tab.scan_device_window(dk.ptr, B, size, window, dc.ptr, dw.ptr, d_row_keys=dkey.ptr,
                                                  d_row_status=st, stream=s.ptr))
        res[name + "_ms"] = [round(v, 4) for v in ms]
        res[name + "_median_ms"] = round(float(np.median(ms)), 4)
        counts = dc.to_numpy(np.uint32, B)
        assert (counts == size).any()
        for buf, nb in ((dc, B * 4), (dw, B * size * ws), (dkey, B * size * kp)) + (((dst, B * size),) if st else ()):
            h.update(buf.to_numpy(np.uint8, nb).tobytes())
    res["digest"] = h.hexdigest()
    print(json.dumps(res), flush=True)


if args.mode == "window":
    window_mode()
    sys.exit(0)
tab = stage.Table(key_width=8)
tab.load_ycsb(0, args.rows, 8, 0)
tab.sync()
if args.mode == "probe":
    keys = stage.zipf_draws(args.rows - 1, args.theta, 0x5EED, args.batch, nthreads=16)
    dk = stage.DeviceBuffer.from_numpy(keys)
    do = stage.DeviceBuffer(args.batch * 32)
    dr = stage.DeviceBuffer(args.batch * tab.stride)
    def step():
        tab.probe_device(dk.ptr, args.batch, do.ptr, dr.ptr, stream=s.ptr)
    n_out, per_unit = 1 << 20, 2100
else:
    starts = (stage.fastrandom(0x5EED, args.batch) % np.uint64(args.rows)).astype(np.uint64)
    dk = stage.DeviceBuffer.from_numpy(starts)
    do = stage.DeviceBuffer(args.batch * 4)
    dr = stage.DeviceBuffer(args.batch * args.scan_size * tab.stride)
    L = stage.lib()
    def step():
        check(L.stage_scan_batch(tab.h, dk.ptr, None, args.batch, args.scan_size, do.ptr, dr.ptr, s.ptr), "scan")
    n_out, per_unit = 1 << 12, 201868
ms = timed(step)
h = hashlib.sha1(do.to_numpy(np.uint8, n_out * (32 if args.mode == "probe" else 4)).tobytes() +
                 dr.to_numpy(np.uint8, n_out * tab.stride * (1 if args.mode == "probe" else args.scan_size)).tobytes())
med = float(np.median(ms))
print(json.dumps({"pkg": args.pkg, "mode": args.mode, "median_ms": med, "min_ms": float(min(ms)),
                  "units_per_s": args.batch / med * 1e3, "frac_of_8TBs": per_unit * args.batch / (med * 1e-3) / 8e12,
                  "digest": h.hexdigest()}), flush=True)
