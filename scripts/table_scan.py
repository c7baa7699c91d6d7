"""Whole-table scan (stage_table_scan / stage_table_scan_window) on the YCSB table bench.py loads
(100M rows of 1000 B): one table, one process, every shape warmed, the shapes timed with device
events in alternating rounds --

    rows        stage_table_scan, raw mode, over the leaf range [0, L) whose rows fit --row-budget-gb
                (100M rows of 1008 B do not fit beside the table: a leaf sub-range, reported)
    win100      stage_table_scan_window (100, 100), raw mode, the whole table
    win4        stage_table_scan_window (0, 4), raw mode, the whole table
    snap100     stage_table_scan_window (100, 100) at the newest read id, the whole table
    count       stage_table_scan with max_records = 0, raw mode
    snap_count  the same at the newest read id (heads only)
    tiled100    the only way to the same records before: stage_scan_batch_window (100, 100) with
    tiled4      / (0, 4) with 100-record scans whose start keys tile the key range (every 100th
                key in KeyCompare order), in the same rounds

Prints one JSON line (and appends it to --out): per shape min / median / max and the per-round
times, ns per delivered record, whether the table scan's time per record is below the tiled form's
in every round, and per shape the bytes per record by construction with the resulting bytes/s
beside the achievable HBM rate (6.3 TB/s; reported, not a gate).

Checked on the way, by key (the keys are the row ids, so "sorted by key" is an array indexed by
key): the table scan delivers every key once; every record of the tiled (0, 4) scans, and the
first and last --check-records records of the tiled (100, 100) scans, equal the table scan's
record of the same key.  The tiled scans themselves do not partition the table -- a 100-record
scan collects a leaf's records in slot order, as the reference does -- and the keys they miss and
deliver twice are counted.  The snapshot's windows equal raw mode's (the table has no versions);
the row form's keys and bytes at 8 + off equal the window form's."""
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
FLIP = np.uint64(0x8080808080808080)
WINDOWS = {"win100": (100, 100), "win4": (0, 4)}
HBM_ACHIEVABLE = 6.3e12
LAST = 0xFFFFFFFE


def stats(v, digits=4):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), digits), "median": round(float(np.median(v)), digits),
            "max": round(float(v.max()), digits)}


def order_words(keys_le):
    """8-byte keys (little-endian words) -> the words whose unsigned order is KeyCompare's"""
    return (np.asarray(keys_le, np.uint64) ^ FLIP).byteswap()


def tile_starts(rows, size):
    """every size-th key of 0 .. rows-1 in KeyCompare order"""
    ow = np.sort(order_words(np.arange(rows, dtype=np.uint64)))[::size]
    return np.ascontiguousarray(ow.byteswap() ^ FLIP)


def window_heap_bytes(window, unit):
    """bytes of the aligned `unit`-B pieces of a heap row that hold the window"""
    s = KEY_PAD + window[0]
    return ((s + window[1] + unit - 1) // unit - s // unit) * unit


def record_bytes(stride, per_leaf, head_bytes=128):
    """per delivered record, from the shapes: index bytes (the leaf head in the count pass and
    again in the emit pass, the 32-B slot word in the emit pass -- this table has no deleted slot,
    so raw mode too counts from the heads), heap bytes (16-B loads; `lines`: the 128-B lines they
    lie in) and output bytes.  The tiled scans read the head, the slot word and the key column
    (8 B per slot); their separator-tree reads are not counted."""
    head = head_bytes / per_leaf
    b = {"rows": {"index": 2 * head + 32, "heap": stride, "lines": stride, "out": stride},
         "count": {"index": head, "heap": 0, "lines": 0, "out": 0},
         "snap_count": {"index": head, "heap": 0, "lines": 0, "out": 0}}
    for name, w in WINDOWS.items():
        heap, lines, out = window_heap_bytes(w, 16), window_heap_bytes(w, 128), stage.window_stride(w[1])
        b[name] = {"index": 2 * head + 32, "heap": heap, "lines": lines, "out": out}
        b["tiled" + name[3:]] = {"index": head + 32 + 8, "heap": heap, "lines": lines, "out": out}
    b["snap100"] = dict(b["win100"])
    for v in b.values():
        v["total"] = round(v["index"] + v["heap"] + v["out"], 1)
        v["total_lines"] = round(v["index"] + v["lines"] + v["out"], 1)
        v["index"] = round(v["index"], 1)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--scan-size", type=int, default=100, help="records per tiled scan")
    ap.add_argument("--row-budget-gb", type=float, default=16.0, help="output bytes of the raw-rows shape")
    ap.add_argument("--check-records", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None, help="file the JSON line is appended to")
    args = ap.parse_args()
    assert args.rounds >= 1 and args.steps >= 1 and args.rows >= 4 * args.scan_size
    if stage.device_count() < 1:
        raise SystemExit("no HIP device: this script measures on the GPU only")

    rows, size = args.rows, args.scan_size
    t0 = time.time()
    tab = stage.Table(key_width=8)
    tab.load_ycsb(0, rows, 8, mode=0)
    tab.sync()
    nl = tab.stats()["leaves"]
    starts = tile_starts(rows, size)
    B = starts.size
    print(f"table of {rows} rows in {nl} leaves and {B} tiling start keys ready in {time.time() - t0:.1f}s",
          file=sys.stderr, flush=True)

    s = stage.Stream()
    d_cnt = stage.DeviceBuffer(8)
    d_off = stage.DeviceBuffer((nl + 1) * 8)
    tab.table_scan_device(None, None, 0, d_cnt, d_off, stream=s)
    s.sync()
    total = int(d_cnt.to_numpy(np.uint64, 1)[0])
    offs = d_off.to_numpy(np.uint64, nl + 1)
    assert total == rows == int(offs[-1]), (total, rows)
    # the raw-rows shape: the longest leaf prefix whose rows fit the budget
    fit = int(args.row_budget_gb * 2 ** 30) // tab.stride
    row_leaves = nl if total <= fit else int(np.searchsorted(offs, fit, side="right")) - 1
    row_records = int(offs[row_leaves])
    ws_max = max(stage.window_stride(w[1]) for w in WINDOWS.values())
    d_out = stage.DeviceBuffer(max(row_records * tab.stride, B * size * ws_max))
    d_key = stage.DeviceBuffer(B * size * KEY_PAD)
    d_starts = stage.DeviceBuffer.from_numpy(starts)
    d_tcnt = stage.DeviceBuffer(B * 4)

    def table(leaves, rid, m, window, keys=False):
        return lambda: tab.table_scan_device(leaves, rid, m, d_cnt, None, d_out if m else None, window,
                                             d_key if keys else None, stream=s)

    def tiled(window, keys=False):
        return lambda: tab.scan_device_window(d_starts.ptr, B, size, window, d_tcnt.ptr, d_out.ptr,
                                              d_row_keys=d_key.ptr if keys else None, stream=s.ptr)

    shapes = {"rows": (table((0, row_leaves), None, row_records, None), row_records),
              "win100": (table(None, None, total, WINDOWS["win100"]), total),
              "tiled100": (tiled(WINDOWS["win100"]), total),
              "win4": (table(None, None, total, WINDOWS["win4"]), total),
              "tiled4": (tiled(WINDOWS["win4"]), total),
              "snap100": (table(None, LAST, total, WINDOWS["win100"]), total),
              "count": (table(None, None, 0, None), total),
              "snap_count": (table(None, LAST, 0, None), total)}

    # ---- warm every shape, and check the outputs against each other
    check, detail = {}, {}
    # The tiled scans do not partition the table: RangeScanBySize collects a leaf's records in slot
    # order, so where slot order is not key order a 100-record scan takes a later key and leaves an
    # earlier one out (some keys come twice, as many are missing).  So the outputs are compared by
    # key: every record a tiled scan delivers must be the table scan's record of that key.  Keys
    # are the row ids 0 .. rows-1, so "sorted by key" is an array indexed by key.
    C = min(args.check_records, total)
    w4, w100 = WINDOWS["win4"], WINDOWS["win100"]
    ws4, ws100 = stage.window_stride(w4[1]), stage.window_stride(w100[1])
    d_key.memset(0, stream=s.ptr)
    table(None, None, total, w4, keys=True)()
    s.sync()
    t_keys = d_key.to_numpy(np.uint64, total, stream=s.ptr)
    t_win4 = d_out.to_numpy(np.uint8, total * ws4, stream=s.ptr).reshape(total, ws4)
    ok = {"count": int(d_cnt.to_numpy(np.uint64, 1)[0]) == total, "keys_in_range": bool(t_keys.max() < rows)}
    ok["every_key_once"] = ok["keys_in_range"] and bool((np.bincount(t_keys.astype(np.int64), minlength=rows) == 1).all())
    ok["padding"] = not t_win4[:, w4[1]:].any()
    pos_of_key = np.empty(rows, np.int64)   # the table scan's position of each key
    pos_of_key[t_keys.astype(np.int64)] = np.arange(total)
    val4 = np.ascontiguousarray(t_win4[:, :4]).view(np.uint32).reshape(-1)
    d_key.memset(0, stream=s.ptr)
    tiled(w4, keys=True)()
    s.sync()
    tc = d_tcnt.to_numpy(np.uint32, B)
    # every scan but the last is full, so the tiled records are contiguous
    ok["tiled_counts"] = int(tc.sum()) == total and bool((tc[:-1] == size).all())
    s_keys = d_key.to_numpy(np.uint64, total, stream=s.ptr)
    s_win4 = d_out.to_numpy(np.uint8, total * ws4, stream=s.ptr).reshape(total, ws4)
    ok["tiled_keys_in_range"] = bool(s_keys.max() < rows)
    ok["windows_by_key"] = ok["tiled_keys_in_range"] and np.array_equal(
        val4[pos_of_key[s_keys.astype(np.int64)]], np.ascontiguousarray(s_win4[:, :4]).view(np.uint32).reshape(-1))
    seen = np.bincount(s_keys.astype(np.int64), minlength=rows)
    tiled_cover = {"distinct_keys": int((seen > 0).sum()), "keys_missing": int((seen == 0).sum()),
                   "keys_twice_or_more": int((seen > 1).sum())}
    detail["win4"] = {k: bool(v) for k, v in ok.items()}
    check["win4"] = check["tiled4"] = all(detail["win4"].values())
    del t_win4, s_win4, val4, seen

    # (100, 100): the tiled scans' first and last C records against the table scan's records of
    # the same keys, which lie in a leaf prefix / suffix a little longer than C
    d_key.memset(0, stream=s.ptr)
    tiled(w100, keys=True)()
    s.sync()
    ok = {"tiled_keys": np.array_equal(d_key.to_numpy(np.uint64, total, stream=s.ptr), s_keys)}
    s_win = (d_out.to_numpy(np.uint8, C * ws100, stream=s.ptr).reshape(C, ws100),
             d_out.to_numpy(np.uint8, C * ws100, stream=s.ptr, offset=(total - C) * ws100).reshape(C, ws100))
    table(None, None, total, w100)()
    s.sync()
    ok["count"] = int(d_cnt.to_numpy(np.uint64, 1)[0]) == total
    want = (pos_of_key[s_keys[:C].astype(np.int64)], pos_of_key[s_keys[total - C:].astype(np.int64)])
    P, S0 = int(want[0].max()) + 1, int(want[1].min())
    ok["ends_are_local"] = P <= 2 * C + 100000 and total - S0 <= 2 * C + 100000
    if ok["ends_are_local"]:
        t_win = (d_out.to_numpy(np.uint8, P * ws100, stream=s.ptr).reshape(P, ws100),
                 d_out.to_numpy(np.uint8, (total - S0) * ws100, stream=s.ptr, offset=S0 * ws100).reshape(total - S0, ws100))
        ok["first_windows_by_key"] = np.array_equal(t_win[0][want[0]], s_win[0])
        ok["last_windows_by_key"] = np.array_equal(t_win[1][want[1] - S0], s_win[1])
        ok["padding"] = not t_win[0][:, w100[1]:].any() and not t_win[1][:, w100[1]:].any()
        shapes["snap100"][0]()
        s.sync()
        snap = d_out.to_numpy(np.uint8, P * ws100, stream=s.ptr).reshape(P, ws100)
        check["snap100"] = bool(int(d_cnt.to_numpy(np.uint64, 1)[0]) == total and np.array_equal(snap, t_win[0]))
        shapes["rows"][0]()
        s.sync()
        k = min(P, row_records)
        head = d_out.to_numpy(np.uint8, k * tab.stride, stream=s.ptr).reshape(k, tab.stride)
        check["rows"] = bool(int(d_cnt.to_numpy(np.uint64, 1)[0]) == row_records and
                             np.array_equal(head[:, :KEY_PAD].reshape(-1).view(np.uint64), t_keys[:k]) and
                             np.array_equal(head[:, KEY_PAD + w100[0]:KEY_PAD + w100[0] + w100[1]], t_win[0][:k, :w100[1]]))
        del head, snap, t_win
    detail["win100"] = {k: bool(v) for k, v in ok.items()}
    check["win100"] = check["tiled100"] = all(detail["win100"].values())
    for name in ("count", "snap_count"):
        d_cnt.memset(0xA5, stream=s.ptr)
        shapes[name][0]()
        s.sync()
        check[name] = int(d_cnt.to_numpy(np.uint64, 1)[0]) == total
    del t_keys, s_keys, pos_of_key, s_win

    # ---- alternated rounds
    e0, e1 = stage.Event(), stage.Event()
    ms = {name: [] for name in shapes}
    for _ in range(args.rounds):
        for name, (launch, _) in shapes.items():
            e0.record(s)
            for _ in range(args.steps):
                launch()
            e1.record(s)
            s.sync()
            ms[name].append(e0.elapsed_ms(e1) / args.steps)
    rbytes = record_bytes(tab.stride, total / nl)
    device = {}
    for name, v in ms.items():
        n = shapes[name][1]
        med = float(np.median(v))
        device[name] = {"records": n, "step_ms": stats(v), "rounds_ms": [round(x, 4) for x in v],
                        "ns_per_record": round(med * 1e6 / n, 4), "bytes_per_record": rbytes[name],
                        "tb_s": round(rbytes[name]["total"] * n / (med * 1e-3) / 1e12, 3),
                        "tb_s_128B_lines": round(rbytes[name]["total_lines"] * n / (med * 1e-3) / 1e12, 3)}
    for w in ("100", "4"):  # the tiled scans per key they actually cover (reported beside the criterion)
        device["tiled" + w]["ns_per_distinct_record"] = round(
            float(np.median(ms["tiled" + w])) * 1e6 / tiled_cover["distinct_keys"], 4)
    faster = {w: bool(all(a < b for a, b in zip(ms["win" + w], ms["tiled" + w]))) for w in ("100", "4")}

    line = json.dumps({
        "script": "table_scan", "rows": rows, "leaves": nl, "records_per_leaf": round(total / nl, 2),
        "table": "the whole table (windows, counts); raw rows over a leaf sub-range" if row_leaves < nl else "the whole table",
        "row_leaves": row_leaves, "row_records": row_records, "tiled_scans": B, "scan_size": size,
        "rounds": args.rounds, "steps_per_round": args.steps, "windows": WINDOWS,
        "win4_checked_records": total, "win100_checked_records_each_end": C, "tiled_scans_cover": tiled_cover,
        "device": device,
        "table_scan_below_tiled_per_record_in_every_round": faster, "hbm_achievable_tb_s": HBM_ACHIEVABLE / 1e12,
        "check_equal": check, "check_detail": detail, "version": stage.lib().stage_version().decode()})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(check.values()) and all(faster.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
