"""In-process A/B of the point probe's two forms (stage_set_probe_form) on the C2 table: one
100M-row table, the forms alternated per round, device events around --steps launches
(cdna_hip_programming.md §5.4 rule 24).  Shapes: rows, status records only and rows with read
ids at Zipf 0.9, plus the uniform and the pre-sorted batch of theta_sweep.py.  Prints min /
median / max of the per-step time per shape and form, and the LANE form's gain against the WAVE
form's own spread (the bar: gain > 3 x noise).  The outputs of both forms are compared once per
shape before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stage-indexorganized_amd"))
import stage  # noqa: E402
from stage._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--batch", type=int, default=1 << 24)
ap.add_argument("--payload", type=int, default=1000, help="payload bytes per row (600: 128-slot leaves)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--forms", default="0,1", help="stage_set_probe_form values, comma separated")
ap.add_argument("--max-blocks", default="0", help="grid caps to time each form at (0 = default), comma separated")
ap.add_argument("--shapes", default="rows,status,rows_rid,uniform,sorted")
args = ap.parse_args()
forms = [int(f) for f in args.forms.split(",")]
caps = [int(c) for c in args.max_blocks.split(",")]
shapes = args.shapes.split(",")

tab = stage.Table(key_width=8, payload_size=args.payload)
tab.load_ycsb(0, args.rows, 8, 0)
tab.sync()
L = stage.lib()
B = args.batch
zipf = stage.zipf_draws(args.rows - 1, 0.9, 0x5EED, B, nthreads=16)
batches = {"zipf": zipf}
if "uniform" in shapes:
    batches["uniform"] = np.random.default_rng(1).integers(0, args.rows, B).astype(np.uint64)
if "sorted" in shapes:
    batches["sorted"] = np.sort(zipf)
d_keys = {k: stage.DeviceBuffer.from_numpy(v) for k, v in batches.items()}
d_rids = stage.DeviceBuffer.from_numpy(np.random.default_rng(2).integers(0, 1 << 30, B).astype(np.uint32))
d_out = stage.DeviceBuffer(B * 32)
d_rec = stage.DeviceBuffer(B * tab.stride)
# shape -> (batch, rows?, read ids?)
SHAPES = {"rows": ("zipf", True, False), "status": ("zipf", False, False), "rows_rid": ("zipf", True, True),
          "uniform": ("uniform", True, False), "sorted": ("sorted", True, False)}
s = stage.Stream()


def launch(shape):
    b, rows, rid = SHAPES[shape]
    tab.probe_device(d_keys[b].ptr, B, d_out.ptr, d_rec.ptr if rows else None,
                     d_read_ids=d_rids.ptr if rid else None, stream=s.ptr)


def select(form, cap):
    check(L.stage_set_probe_form(tab.h, form), "stage_set_probe_form")
    check(L.stage_set_probe_tuning(tab.h, 8, cap), "stage_set_probe_tuning")


# the forms write the same bytes (first 2^20 probes' status records and rows)
m = min(B, 1 << 20)
for shape in shapes:
    ref = None
    for form in forms:
        select(form, 0)
        check(L.stage_dev_memset(d_out.ptr, 0xA5, m * 32, s.ptr), "memset")
        check(L.stage_dev_memset(d_rec.ptr, 0xA5, m * tab.stride, s.ptr), "memset")
        launch(shape)
        s.sync()
        got = (d_out.to_numpy(np.uint8, m * 32).tobytes(),
               d_rec.to_numpy(np.uint8, m * tab.stride).tobytes() if SHAPES[shape][1] else b"")
        if ref is None:
            ref = got
        assert got == ref, f"form {form} differs from form {forms[0]} at shape {shape}"
print(json.dumps({"outputs_equal": True, "shapes": shapes, "forms": forms}), flush=True)

variants = [(f, c) for f in forms for c in caps]
res = {(sh, v): [] for sh in shapes for v in variants}
e0, e1 = stage.Event(), stage.Event()
for r in range(args.rounds):
    for shape in shapes:
        for v in variants:
            select(*v)
            launch(shape)  # warm-up of this variant at this shape
            e0.record(s)
            for _ in range(args.steps):
                launch(shape)
            e1.record(s)
            s.sync()
            res[(shape, v)].append(e0.elapsed_ms(e1) / args.steps)
for shape in shapes:
    base = np.array(res[(shape, variants[0])])
    noise = float((base.max() - base.min()) / np.median(base))
    for v in variants:
        ms = np.array(res[(shape, v)])
        print(json.dumps({"shape": shape, "form": v[0], "max_blocks": v[1], "min_ms": round(float(ms.min()), 4),
                          "median_ms": round(float(np.median(ms)), 4), "max_ms": round(float(ms.max()), 4),
                          "glookups_s": round(B / float(np.median(ms)) / 1e6, 3),
                          "gain_vs_first": round(1.0 - float(np.median(ms) / np.median(base)), 4),
                          "first_noise": round(noise, 4)}), flush=True)
