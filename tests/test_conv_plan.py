"""The conv / GEMM planner (csrc/conv_plan.hpp) chooses what the parent commit's dispatch chose.

tests/golden/conv_plan_parent.json holds, per row of scripts/conv_plan_probe.py's table, the
`fs2::` kernels (name, workgroups) the parent's library launched for that call on an MI355X
(kernel trace, dispatch order).  fs2_debug_conv_plan launches nothing, so this runs on the CPU.
"""
import ctypes
import importlib
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_parent.json")
OPS = {"gemm": 0, "gemm_ex": 0, "ln": 1, "ln_bwd": 2, "wgrad": 3, "k1_multi": 4}
VEC, HAS_Y, HAS_LENS, HAS_DB, DW16, WS16 = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def plan(lib, r, cu_count):
    facts = HAS_Y | DW16 | WS16
    if r["c_out"] % 8 == 0:
        facts |= VEC  # the probe's tensors are 16-B aligned with ld = channels
    if r["lens"]:
        facts |= HAS_LENS
    if r["db"]:
        facts |= HAS_DB
    jobs = (ctypes.c_int64 * (8 * max(len(r["jobs"]), 1)))()
    for j, (ci, co, db) in enumerate(r["jobs"]):
        jobs[8 * j + 5], jobs[8 * j + 6], jobs[8 * j + 7] = db, ci, co
    out = ctypes.create_string_buffer(256)
    for k, v in r["knobs"].items():
        lib.fs2_set_tuning(int(k), v)
    try:
        lib.fs2_debug_conv_plan(OPS[r["op"]], r["rows"], r["T"], r["c_in"], r["c_out"], r["taps"],
                                r["pad"], r["dil"], r["flags"], facts,
                                ctypes.cast(jobs, ctypes.c_void_p) if r["jobs"] else None,
                                len(r["jobs"]), cu_count, ctypes.cast(out, ctypes.c_void_p), 256)
    finally:
        for k in r["knobs"]:
            lib.fs2_set_tuning(int(k), 0)
    m = re.fullmatch(r"(.+) grid=(\d+) group=(\d+) kz=(\d+) reduce=(.+) reduce_grid=(\d+)",
                     out.value.decode())
    assert m, out.value
    kernels = [[m.group(1), int(m.group(2))]]
    if m.group(5) != "-":
        kernels.append([m.group(5), int(m.group(6))])
    return kernels


def test_planner_matches_parent_trace(golden):
    lib = importlib.import_module("mid-attribute-speaker-generation_amd._lib").lib
    assert len(golden["rows"]) >= 100
    bad = []
    for i, r in enumerate(golden["rows"]):
        got = plan(lib, r, golden["cu_count"])
        if r["op"] == "ln_bwd":  # fs2_conv_gemm_ln_bwd ends with fs2_ln_bwd_final: not a conv plan
            assert r["kernels"][-1][0] == "colsum_final_multi"
            got.append(r["kernels"][-1])
        if got != r["kernels"]:
            bad.append((i, r["note"], got, r["kernels"]))
    assert not bad, bad


def test_every_instance_is_recorded_or_explained(golden):
    """tests/golden/conv_plan_instances.txt lists every kernel instance the conv dispatch builds
    (the library's kernel symbols of these families).  Each is produced by a recorded row or is
    listed as not reached, with a reason; nothing else is recorded."""
    with open(os.path.join(os.path.dirname(GOLDEN), "conv_plan_instances.txt")) as f:
        built = set(f.read().split("\n")) - {""}
    seen = {k[0] for r in golden["rows"] for k in r["kernels"]} - {"colsum_final_multi"}
    excused = set(golden["not_reached"])
    assert all(golden["not_reached"].values())
    assert not (seen & excused)
    assert seen | excused == built, (sorted(built - seen - excused), sorted((seen | excused) - built))


def test_debug_entry_rejects_degenerate_shapes():
    dll = importlib.import_module("mid-attribute-speaker-generation_amd._lib").lib.load()
    out = ctypes.create_string_buffer(64)
    o = ctypes.cast(out, ctypes.c_void_p)
    assert dll.fs2_debug_conv_plan(3, 4096, 0, 256, 256, 3, 1, 1, 0, 0, None, 0, 256, o, 64) == -1  # seq_len 0
    assert dll.fs2_debug_conv_plan(0, 4096, 128, 0, 256, 9, 4, 1, 0, 3, None, 0, 256, o, 64) == -1  # c_in 0


def test_knob_4_is_retired():
    lib = importlib.import_module("mid-attribute-speaker-generation_amd._lib").lib
    assert lib.load().fs2_set_tuning(4, 1) == -1  # FS2_ERR_ARG
    assert b"gone" in lib.load().fs2_last_error()
    lib.fs2_set_tuning(4, 0)
