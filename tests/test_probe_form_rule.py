"""CPU: the lane-per-probe form of the read probe (probe_rows_kernel) keeps the dispatch rule C3's
overlap rests on (test_dispatch_rule.py), checked on the built library's gfx950
kernel metadata; and stage_set_probe_form's argument rules (no device call).

Beside a read probe whose 256-thread, LDS-free workgroups fill every CU, a write-chain workgroup
gets the slot one retired probe wave frees: that wave's registers, in the 8-register granules
gfx950 allocates.  A probe form that allocates fewer registers than a write-chain kernel needs
would leave that kernel waiting for the probe's last dispatch."""
import os
import re
import subprocess
import tempfile

import pytest

import stage
from test_dispatch_rule import LIB, LLVM, VGPR_GRANULE, WRITE_CHAIN, gfx950_code_objects

ROWS_PROBE = "_ZN5stage17probe_rows_kernelI"
E_ARG = -1
FORM_WAVE, FORM_LANE = 0, 1
KEYS = "name|vgpr_count|agpr_count|max_flat_workgroup_size|group_segment_fixed_size|private_segment_fixed_size"


def kernels(co):
    """test_dispatch_rule.kernels with the scratch size: name -> the metadata fields of KEYS"""
    with tempfile.NamedTemporaryFile(suffix=".o") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], check=True,
                               capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        if re.match(r"\s+- \.agpr_count:", line):  # a kernel's entry starts with its first key
            cur = {}
        m = re.match(rf"\s+-?\s*\.({KEYS}):\s+(\S+)", line)
        if m:
            k, v = m.group(1), m.group(2)
            cur[k] = v if k == "name" else int(v)
            if k == "name":
                out[v] = cur
    return out


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("libstage_hip.so or the ROCm LLVM tools are missing")
    ks = {}
    for co in gfx950_code_objects(LIB):
        ks.update(kernels(co))
    return ks


def rows_probes(table):
    probes = {k: v for k, v in table.items() if k.startswith(ROWS_PROBE)}
    assert len(probes) == 3, sorted(probes)  # 64-slot leaves with 32- and 16-B records, 128-slot leaves
    return probes


def budget(table):
    """the VGPRs (arch + acc) a retired wave of the smallest rows-probe instance leaves free"""
    used = min(v["vgpr_count"] + v.get("agpr_count", 0) for v in rows_probes(table).values())
    return -(-used // VGPR_GRANULE) * VGPR_GRANULE


def test_rows_probe_workgroups(table):
    for name, v in rows_probes(table).items():
        assert v["max_flat_workgroup_size"] == 256, (name, v)
        assert v["group_segment_fixed_size"] == 0, (name, v)    # no LDS
        assert v["private_segment_fixed_size"] == 0, (name, v)  # no scratch


def test_write_chain_fits_beside_the_rows_probe(table):
    least = budget(table)
    seen = set()
    for name, v in table.items():
        short = next((w for w in WRITE_CHAIN if f"{len(w)}{w}E" in name), None)
        if short is None:
            continue
        seen.add(short)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= least, (short, v, least)
    assert seen == set(WRITE_CHAIN), set(WRITE_CHAIN) - seen


def test_write_path_sort_fits_beside_the_rows_probe(table):
    least = budget(table)
    sort = {k: v for k, v in table.items()
            if "onesweep_iteration" in k and "EmjEE" in k and "kernel_configILj256E" in k and "target_archE950" in k}
    assert sort, "the write path's onesweep kernels were not found"
    for name, v in sort.items():
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= least, (name[:120], v, least)


def test_set_probe_form_arguments():
    L = stage.lib()
    assert L.stage_set_probe_form(None, FORM_LANE) == E_ARG
    tab = stage.Table(key_width=8)
    for bad in (-1, 2, 8):
        assert L.stage_set_probe_form(tab.h, bad) == E_ARG
    assert L.stage_set_probe_form(tab.h, FORM_LANE) == 0
    assert L.stage_set_probe_form(tab.h, FORM_WAVE) == 0
    tab.set_probe_form(FORM_LANE)
