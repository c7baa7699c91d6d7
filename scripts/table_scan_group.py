"""Grouped aggregates (stage_table_scan_group_aggregate) on the YCSB table bench.py loads (100M rows
of 1000 B, payload mode 0): one table, one process, every shape warmed and checked, the shapes timed
with device events in alternating rounds beside

    agg                 stage_table_scan_aggregate of column (0, 4) without a predicate: the same
                        leaf heads, slot words and heap lines, no groups -- the memory floor

Every grouped call aggregates the same column (0, 4); its group column lies on the same 128-B heap
line (row bytes 0 .. 12).  Payload mode 0 fills a row's payload with the byte key & 0xFF, so the
table offers these integer columns: the key's fields (in_key) and that byte.  Per n_groups G in
4, 16, 256, STAGE_GROUP_LDS_MAX, STAGE_GROUP_LDS_MAX + 1, 65536, 2^20:

    spread_G            the group column is the key's low 1 (G <= 256), 2 (G <= 65536) or 4 bytes,
                        base 0: consecutive records fall into consecutive groups, every group
                        receives the same number of records (+-1), and the records whose value is
                        G or above go to the rest group (`in_groups` is the fraction that does not)
    hot_G               the group column is the payload byte (4, 1) under the predicate
                        Pred(4, 1, 1, 1) that pins it: every matching record in group 1

and, beyond that list, the shapes the data allow with every record in a group:

    runs_1048576        the key's bytes 1 .. 4 (key >> 8), 2^20 groups: runs of 256 consecutive
                        records share a group, 390 625 groups in use
    one_G               the key's top byte (always 0), G = 4 and STAGE_GROUP_LDS_MAX + 1: every record
                        of the table in group 0, no predicate -- the most lanes on one entry

--read-id R runs every shape in snapshot mode at read id R (the kernels' VIS instances).
--sweep times every shape again under stage_set_scan_group_tuning's choices (tier: default or the
global tier always; lanes of equal groups combined: never, the first lane's group, all) and checks
that each leaves the default call's bytes.  --no-check skips the host-side checks (a profiler run).

Prints one JSON line (and appends it to --out): per shape min / median / max and the per-round
times, the records in groups, the ratio of its median to the ungrouped aggregate's median of the
same job and whether that is below 2 (`bar`; reported, the exit status is the checks').

Checked on the way, on the whole table: every timed shape's n_groups + 1 records equal numpy's
(np.bincount / np.add.at / np.minimum.at / np.maximum.at over the unfiltered window scan's
columns and keys), and their fold equals the device's ungrouped aggregate."""
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
COL = (0, 4, False)          # the aggregate column
GBYTE = (4, 1)               # the payload byte next to it
W8 = (0, 8)                  # the window that holds both
LDS_MAX = stage.GROUP_LDS_MAX
GROUPS = (4, 16, 256, LDS_MAX, LDS_MAX + 1, 65536, 1 << 20)
SWEEP = [(lds_max, combine) for lds_max in (-1, 0) for combine in (0, 1, 64)]
BAR = 2.0


def stats(v, digits=4):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), digits), "median": round(float(np.median(v)), digits),
            "max": round(float(v.max()), digits)}


def key_column(width):
    return 1 if width <= 256 else 2 if width <= 65536 else 4


def make_shapes():
    """name -> (Group, preds)"""
    G, P = stage.Group, stage.Pred
    shapes = {}
    for n in GROUPS:
        shapes[f"spread_{n}"] = (G(0, key_column(n), 0, n, in_key=True), [])
    for n in GROUPS:
        shapes[f"hot_{n}"] = (G(GBYTE[0], GBYTE[1], 0, n), [P(GBYTE[0], GBYTE[1], 1, 1)])
    shapes[f"runs_{1 << 20}"] = (G(1, 4, 0, 1 << 20, in_key=True), [])
    for n in (4, LDS_MAX + 1):
        shapes[f"one_{n}"] = (G(7, 1, 0, n, in_key=True), [])
    return shapes


def numpy_groups(group, preds, keys, win):
    """-> uint64 [n_groups + 1, 4]: count, sum, min, max of column (0, 4) per group, from the
    unfiltered scan's keys and (0, 8) windows"""
    x = np.ascontiguousarray(win[:, :4]).view(np.uint32).reshape(-1).astype(np.uint64)
    if group.in_key:
        val = (keys >> np.uint64(8 * group.off)) if group.off else keys
        if group.width < 8:
            val = val & np.uint64((1 << (8 * group.width)) - 1)
        val = val.astype(np.int64)  # keys are below 2^63 here
    else:
        val = win[:, group.off].astype(np.int64)
        assert group.width == 1
    m = None
    for p in preds:
        assert (p.off, p.width, p.signed, p.negate) == (GBYTE[0], 1, False, False)
        b = win[:, p.off]
        m = (b >= p.lo) & (b <= p.hi)
    if m is not None:
        val, x = val[m], x[m]
    n = group.n_groups
    ids = np.where((val >= group.base) & (val - group.base < n), val - group.base, n)
    total, mn, mx = np.zeros(n + 1, np.uint64), np.full(n + 1, 0xFFFFFFFF, np.uint64), np.zeros(n + 1, np.uint64)
    np.add.at(total, ids, x)
    np.minimum.at(mn, ids, x)
    np.maximum.at(mx, ids, x)
    return np.stack([np.bincount(ids, minlength=n + 1).astype(np.uint64), total, mn, mx], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None, help="file the JSON line is appended to")
    ap.add_argument("--read-id", type=lambda v: int(v, 0), default=None,
                    help="snapshot mode at this read id (the VIS kernel instances); default: raw mode")
    ap.add_argument("--sweep", action="store_true", help="time the tier and combining choices too")
    ap.add_argument("--no-check", action="store_true", help="skip the host-side checks")
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
    L = stage.lib()
    shapes = make_shapes()
    d_agg = stage.DeviceBuffer(32)
    d_groups = stage.DeviceBuffer(32 * ((1 << 20) + 1))

    def grouped(name):
        g, p = shapes[name]
        return lambda: tab.table_scan_group_aggregate_device(None, rid, p, g, COL, d_groups, stream=s)

    def result(name):
        n = shapes[name][0].n_groups + 1
        d_groups.memset(0xA5, stream=s.ptr)
        grouped(name)()
        s.sync()
        return d_groups.to_numpy(np.uint64, 4 * n, stream=s.ptr).reshape(n, 4)

    calls = {"agg": lambda: tab.table_scan_aggregate_device(None, rid, [], COL, d_agg, stream=s)}
    calls.update({name: grouped(name) for name in shapes})

    # ---- warm every shape, keep its result, and check it against numpy on the whole table
    got = {name: result(name) for name in shapes}
    check, in_groups = {}, {}
    for name, r in got.items():
        tot = int(r[:, 0].sum())
        in_groups[name] = {"records": tot, "in_groups": round(float(r[:-1, 0].sum()) / max(tot, 1), 4),
                           "groups_in_use": int((r[:-1, 0] != 0).sum())}
    if not args.no_check:
        d_cnt = stage.DeviceBuffer(8)
        d_out = stage.DeviceBuffer(rows * stage.window_stride(W8[1]))
        d_key = stage.DeviceBuffer(rows * KEY_PAD)
        tab.table_scan_device(None, rid, rows, d_cnt, None, d_out, W8, d_key, stream=s)
        s.sync()
        total = int(d_cnt.to_numpy(np.uint64, 1)[0])
        assert total == rows, (total, rows)
        keys = d_key.to_numpy(np.uint64, total, stream=s.ptr)
        ws = stage.window_stride(W8[1])
        win = np.ascontiguousarray(d_out.to_numpy(np.uint8, total * ws, stream=s.ptr).reshape(total, ws)[:, :8])
        del d_out, d_key
        print(f"unfiltered scan on the host in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        calls["agg"]()
        s.sync()
        x = np.ascontiguousarray(win[:, :4]).view(np.uint32).reshape(-1)
        whole = (total, int(x.sum(dtype=np.uint64)), int(x.min()), int(x.max()))
        check["agg"] = {"aggregate": tuple(int(v) for v in d_agg.to_numpy(np.uint64, 4)) == whole}
        for name, (g, p) in shapes.items():
            want = numpy_groups(g, p, keys, win)
            r = got[name]
            ok = {"groups": bool(np.array_equal(r, want))}
            if not p:  # the fold of every record of the table is the ungrouped aggregate
                with np.errstate(over="ignore"):
                    fold = (int(r[:, 0].sum()), int(r[:, 1].sum(dtype=np.uint64)), int(r[:, 2].min()), int(r[:, 3].max()))
                ok["fold"] = fold == whole
            check[name] = ok
            print(f"  {name}: {ok} {in_groups[name]} at {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        del keys, win, x

    # ---- alternated rounds
    e0, e1 = stage.Event(), stage.Event()

    def timed(names, rounds):
        ms = {name: [] for name in names}
        for _ in range(rounds):
            for name in names:
                e0.record(s)
                for _ in range(args.steps):
                    calls[name]()
                e1.record(s)
                s.sync()
                ms[name].append(e0.elapsed_ms(e1) / args.steps)
        return ms

    ms = timed(list(calls), args.rounds)
    floor = float(np.median(ms["agg"]))
    device = {"agg": {"step_ms": stats(ms["agg"]), "rounds_ms": [round(x, 4) for x in ms["agg"]]}}
    for name in shapes:
        g, p = shapes[name]
        med = float(np.median(ms[name]))
        device[name] = {"n_groups": g.n_groups, "group_column": [g.off, g.width, "key" if g.in_key else "payload"],
                        "predicates": len(p), **in_groups[name], "step_ms": stats(ms[name]),
                        "rounds_ms": [round(x, 4) for x in ms[name]], "over_agg": round(med / floor, 3),
                        "bar": bool(med < BAR * floor)}
    missed = [name for name in shapes if not device[name]["bar"]]

    # ---- the tier and combining choices: medians, and the same bytes as the default call
    sweep = None
    if args.sweep:
        sweep = {}
        try:
            for lds_max, combine in SWEEP:
                assert L.stage_set_scan_group_tuning(tab.h, lds_max, combine) == 0
                same = all(np.array_equal(result(name), got[name]) for name in shapes)
                v = timed(["agg"] + list(shapes), max(args.rounds // 2, 2))
                sweep[f"lds_max={lds_max},combine={combine}"] = {
                    "same_bytes": bool(same), **{name: round(float(np.median(x)), 4) for name, x in v.items()}}
                check[f"sweep lds_max={lds_max} combine={combine}"] = {"same_bytes": bool(same)}
        finally:
            assert L.stage_set_scan_group_tuning(tab.h, -1, -1) == 0

    ok = all(all(c.values()) for c in check.values())
    line = json.dumps({
        "script": "table_scan_group", "rows": rows, "leaves": nl, "rounds": args.rounds, "steps_per_round": args.steps,
        "read_id": rid, "aggregate_column": COL, "group_lds_max": LDS_MAX, "bar_over_agg": BAR, "device": device,
        "missed_bar": missed, "sweep_median_ms": sweep, "check_equal": check if not args.no_check else None,
        "version": L.stage_version().decode(), "lib": os.environ.get("STAGE_LIB") or "this tree"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
