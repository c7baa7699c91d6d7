"""Filtered whole-table scans (stage_table_scan_where_window, stage_table_scan_aggregate) on the YCSB
table bench.py loads (100M rows of 1000 B): one table, one process, every shape warmed, the shapes
timed with device events in alternating rounds --

    win4, win100        stage_table_scan_window (0, 4) / (100, 100), unfiltered: the parent's forms
    where100_pNN        stage_table_scan_where_window (100, 100) under one predicate on the 4-byte
                        column at payload offset 0, lo = 0 and hi = that column's own quantile for
                        about NN = 1, 10, 50, 100 % of the records
    where100x2_pNN      the same with a second, conjunctive predicate on the 4-byte column at payload
                        offset 500 -- another 128-B line of the heap row -- that holds for every
                        record, so the matches stay the same and the second line is what is added
    agg, agg_p10        stage_table_scan_aggregate of column (0, 4) without a predicate and under
                        the 10 % predicate

--read-id R runs every shape in snapshot mode at read id R (the kernels' VIS instances) instead
of raw mode.  STAGE_LIB=<another build's libstage_hip.so> times that build: alternate the two
for an A/B.

Prints one JSON line (and appends it to --out): per shape min / median / max and the per-round
times, the matches, bytes per scanned record by construction with the resulting bytes/s beside the
achievable HBM rate (6.3 TB/s; reported, not a gate), and two comparisons: whether the aggregate's
step is at or below the (0, 4) window's in every round, and the ~1 % filtered scan's step beside
the aggregate's.

Checked on the way, on the whole table: for every predicate the count, the windows and the keys
equal a numpy filter of the unfiltered (0, 4) and (100, 100) window scans, the (leaf, slot) numbers
increase strictly, and the aggregates equal numpy's count / sum / min / max of the column."""
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
W4, W100 = (0, 4), (100, 100)
COL, COL2 = (0, 4, False), (500, 4, False)
FRACTIONS = (1, 10, 50, 100)
HBM_ACHIEVABLE = 6.3e12


def stats(v, digits=4):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), digits), "median": round(float(np.median(v)), digits),
            "max": round(float(v.max()), digits)}


def heap_bytes(off, length, unit):
    """bytes of the aligned `unit`-B pieces of a heap row that hold payload bytes [off, off + length)"""
    s = KEY_PAD + off
    return ((s + length + unit - 1) // unit - s // unit) * unit


def record_bytes(per_leaf, cols, frac, window, head_bytes=128):
    """per scanned record, from the shapes.  Match pass (and the aggregate): the leaf head, the 32-B
    slot word, one 8-B word per column (`lines`: the 128-B line it lies in), 8 B of mask per 64 slots
    and 4 B of count per leaf.  Emit pass, per matching record (frac of the scanned ones): the slot
    word again, the window's 16-B pieces (`lines`: its 128-B lines) and the window written; per leaf
    the mask and the counts of its tile.  window None: no emit pass (the aggregate)."""
    head = head_bytes / per_leaf
    index = head + 32 + (8 + 4) / per_leaf
    heap = sum(heap_bytes(o, w, 8) for o, w, _ in cols)
    lines = 128 * len({(KEY_PAD + o) // 128 for o, w, _ in cols})
    out = 0.0
    if window is not None:
        index += (8 + 4) / per_leaf + frac * 32
        heap += frac * heap_bytes(window[0], window[1], 16)
        lines += frac * heap_bytes(window[0], window[1], 128)
        out = frac * stage.window_stride(window[1])
    return {"index": round(index, 1), "heap": round(heap, 1), "lines": round(lines, 1), "out": round(out, 1),
            "total": round(index + heap + out, 1), "total_lines": round(index + lines + out, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None, help="file the JSON line is appended to")
    ap.add_argument("--read-id", type=lambda v: int(v, 0), default=None,
                    help="snapshot mode at this read id (the VIS kernel instances); default: raw mode")
    args = ap.parse_args()
    rid = args.read_id
    assert args.rounds >= 1 and args.steps >= 1 and args.rows >= 1000
    if stage.device_count() < 1:
        raise SystemExit("no HIP device: this script measures on the GPU only")

    rows = args.rows
    t0 = time.time()
    tab = stage.Table(key_width=8)
    tab.load_ycsb(0, rows, 8, mode=0)
    tab.sync()
    nl = tab.stats()["leaves"]
    print(f"table of {rows} rows in {nl} leaves ready in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    s = stage.Stream()
    ws4, ws100 = stage.window_stride(W4[1]), stage.window_stride(W100[1])
    d_cnt = stage.DeviceBuffer(8)
    d_agg = stage.DeviceBuffer(32)
    d_out = stage.DeviceBuffer(rows * ws100)
    d_key = stage.DeviceBuffer(rows * KEY_PAD)
    d_slot = stage.DeviceBuffer(rows * 8)

    # ---- the unfiltered scans: what every filtered result is checked against
    tab.table_scan_device(None, rid, rows, d_cnt, None, d_out, W4, d_key, stream=s)
    s.sync()
    total = int(d_cnt.to_numpy(np.uint64, 1)[0])
    assert total == rows, (total, rows)
    keys = d_key.to_numpy(np.uint64, total, stream=s.ptr)
    col = np.ascontiguousarray(d_out.to_numpy(np.uint8, total * ws4, stream=s.ptr).reshape(total, ws4)[:, :4]) \
        .view(np.uint32).reshape(-1)
    tab.table_scan_device(None, rid, rows, d_cnt, None, d_out, W100, stream=s)
    s.sync()
    win100 = d_out.to_numpy(np.uint8, total * ws100, stream=s.ptr).reshape(total, ws100)
    order = np.sort(col)
    thresholds = {f: int(order[min(total - 1, max(0, total * f // 100 - 1))]) if f < 100 else 0xFFFFFFFF
                  for f in FRACTIONS}
    del order
    print(f"unfiltered scans on the host, thresholds {thresholds} in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    def preds(f, two):
        p = [stage.Pred(COL[0], COL[1], 0, thresholds[f])]
        return p + [stage.Pred(COL2[0], COL2[1], 0, 0xFFFFFFFF)] if two else p

    def where(f, two, keys_too=False):
        return lambda: tab.table_scan_where_device(None, rid, preds(f, two), rows, d_cnt, None, d_out, W100,
                                                   d_key if keys_too else None, d_slot if keys_too else None, stream=s)

    def agg(p):
        return lambda: tab.table_scan_aggregate_device(None, rid, p, COL, d_agg, stream=s)

    shapes = {"win4": (lambda: tab.table_scan_device(None, rid, rows, d_cnt, None, d_out, W4, stream=s), [COL], None, 1.0),
              "win100": (lambda: tab.table_scan_device(None, rid, rows, d_cnt, None, d_out, W100, stream=s), [], W100, 1.0)}
    matches = {}
    for two in (False, True):
        for f in FRACTIONS:
            name = f"where100{'x2' if two else ''}_p{f}"
            shapes[name] = (where(f, two), [COL, COL2] if two else [COL], W100, f)
    shapes["agg"] = (agg([]), [COL], None, 0.0)
    shapes["agg_p10"] = (agg(preds(10, False)), [COL], None, 0.0)

    # ---- warm every shape, and check the filtered results against the numpy filter
    check = {}
    for f in FRACTIONS:
        mask = col <= np.uint32(thresholds[f])
        n = int(mask.sum())
        matches[f] = n
        for two in (False, True):
            d_cnt.memset(0xA5, stream=s.ptr)
            where(f, two, keys_too=True)()
            s.sync()
            got = int(d_cnt.to_numpy(np.uint64, 1)[0])
            ok = {"count": got == n}
            if ok["count"]:
                ok["keys"] = np.array_equal(d_key.to_numpy(np.uint64, n, stream=s.ptr), keys[mask])
                slots = d_slot.to_numpy(np.uint64, n, stream=s.ptr)
                ok["slots_increase"] = bool((slots[1:] > slots[:-1]).all()) and bool((slots >> np.uint64(16) < nl).all())
                w = d_out.to_numpy(np.uint8, n * ws100, stream=s.ptr).reshape(n, ws100)
                ok["windows"] = np.array_equal(w, win100[mask])
                del w, slots
            check[f"where100{'x2' if two else ''}_p{f}"] = {k: bool(v) for k, v in ok.items()}
        for name, p in (("agg", []), ("agg_p10", preds(10, False))):
            if f != (100 if name == "agg" else 10):
                continue
            d_agg.memset(0xA5, stream=s.ptr)
            agg(p)()
            s.sync()
            x = col[mask].astype(np.uint64)
            want = (n, int(x.sum(dtype=np.uint64)), int(x.min()), int(x.max()))
            check[name] = {"aggregate": tuple(int(v) for v in d_agg.to_numpy(np.uint64, 4)) == want}
    del win100, keys
    for name in ("win4", "win100"):
        shapes[name][0]()
    s.sync()
    print(f"checks done in {time.time() - t0:.1f}s: {check}", file=sys.stderr, flush=True)

    # ---- alternated rounds
    e0, e1 = stage.Event(), stage.Event()
    ms = {name: [] for name in shapes}
    for _ in range(args.rounds):
        for name, sh in shapes.items():
            e0.record(s)
            for _ in range(args.steps):
                sh[0]()
            e1.record(s)
            s.sync()
            ms[name].append(e0.elapsed_ms(e1) / args.steps)
    device = {}
    for name, v in ms.items():
        _, cols, window, f = shapes[name]
        frac = matches[f] / total if window is not None and name.startswith("where") else (1.0 if window else 0.0)
        if name == "win4":  # the unfiltered (0, 4) window: table_scan.py's accounting
            head = 128 / (total / nl)
            b = {"index": round(2 * head + 32, 1), "heap": 16, "lines": 128, "out": ws4}
            b["total"], b["total_lines"] = round(b["index"] + 16 + ws4, 1), round(b["index"] + 128 + ws4, 1)
        elif name == "win100":
            head = 128 / (total / nl)
            hb, hl = heap_bytes(W100[0], W100[1], 16), heap_bytes(W100[0], W100[1], 128)
            b = {"index": round(2 * head + 32, 1), "heap": hb, "lines": hl, "out": ws100}
            b["total"], b["total_lines"] = round(b["index"] + hb + ws100, 1), round(b["index"] + hl + ws100, 1)
        else:
            b = record_bytes(total / nl, cols, frac, window)
        med = float(np.median(v))
        device[name] = {"scanned": total, "matches": matches.get(f) if name.startswith("where") else None,
                        "step_ms": stats(v), "rounds_ms": [round(x, 4) for x in v],
                        "ns_per_scanned_record": round(med * 1e6 / total, 4), "bytes_per_scanned_record": b,
                        "tb_s": round(b["total"] * total / (med * 1e-3) / 1e12, 3),
                        "tb_s_128B_lines": round(b["total_lines"] * total / (med * 1e-3) / 1e12, 3)}
    device["agg_p10"]["matches"] = matches[10]
    compare = {
        "aggregate_at_or_below_win4_in_every_round": bool(all(a <= b for a, b in zip(ms["agg"], ms["win4"]))),
        "aggregate_p10_at_or_below_win4_in_every_round": bool(all(a <= b for a, b in zip(ms["agg_p10"], ms["win4"]))),
        "where100_p1_minus_aggregate_ms": round(float(np.median(ms["where100_p1"]) - np.median(ms["agg"])), 4),
        "where100_p1_over_aggregate": round(float(np.median(ms["where100_p1"]) / np.median(ms["agg"])), 3),
    }
    ok = all(all(c.values()) for c in check.values())
    line = json.dumps({
        "script": "table_scan_where", "rows": rows, "leaves": nl, "records_per_leaf": round(total / nl, 2),
        "rounds": args.rounds, "steps_per_round": args.steps, "read_id": rid, "window": W100, "predicate_column": COL,
        "second_predicate_column": COL2, "thresholds": thresholds, "matches": matches, "device": device,
        "comparisons": compare, "hbm_achievable_tb_s": HBM_ACHIEVABLE / 1e12, "check_equal": check,
        "version": stage.lib().stage_version().decode(), "lib": os.environ.get("STAGE_LIB") or "this tree"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
