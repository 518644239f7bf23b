"""One bf16 conv / GEMM call per table row, in a fixed order, for a kernel trace.

    rocprofv3 --kernel-trace -d <dir> -o probe --output-format csv -- \
        python3 scripts/conv_plan_probe.py run
    python3 scripts/conv_plan_probe.py golden <probe_kernel_trace.csv> <parent hash> <out.json>

`run` issues, per row of table(): the row's knobs, one fs2_conv_gemm / _ex / _ln / _ln_bwd /
fs2_conv_wgrad / _k1_multi call, the knobs back to 0, and one fs2_cast_bf16 of 1 element as the
row separator in the trace.  Run it against the library whose choices are to be recorded
(FS2HIP_LIB); `golden` cuts the trace at the separators and writes tests/golden/
conv_plan_parent.json, which tests/test_conv_plan.py holds the planner to on the CPU.  The
shapes are the smallest that satisfy each branch's grid thresholds on a 256-CU device.
"""
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BIAS, RELU, ADD_AUX, RELU_MASK, OUT_BF16, AUX_BF16, LRELU = 1, 2, 4, 8, 16, 32, 64
(T_GEMM_STAGES, T_WGRAD_STAGES, T_WGRAD_TILE, T_WGRAD_SPLITS, _, T_NT_GROUP, T_NT_HALO, T_WGRAD_HALO,
 T_HALO_SPLITK, _, T_NT_TILE, T_LN_TILE, T_WGRAD_K1, T_NT_K1, _, T_TAPREG, T_WGRAD_BAND, _,
 T_K1M_STAGES, T_WGRAD_WIDE) = range(20)
SEPARATOR = "cast_bf16_kernel"


def table():
    rows = []

    def add(note, op, rows_, T, cin, cout, taps, knobs=None, dil=1, flags=OUT_BF16, lens=0, db=1,
            jobs=None):
        rows.append(dict(note=note, op=op, rows=rows_, T=T, c_in=cin, c_out=cout, taps=taps,
                         pad=(taps - 1) * dil // 2, dil=dil, flags=flags, lens=lens, db=db,
                         knobs={str(k): v for k, v in (knobs or {}).items()}, jobs=jobs or []))

    # ---- tap-register kernel
    add("decoder k=9 forward", "gemm", 24576, 512, 256, 1024, 9, flags=OUT_BF16 | BIAS | RELU)
    add("decoder k=9 data gradient", "gemm", 24576, 512, 1024, 256, 9)
    add("PostNet 512 -> 512 k=5", "gemm", 24576, 512, 512, 512, 5)
    add("k=5 narrow output", "gemm", 24576, 512, 512, 256, 5)
    for v in (1, 3, -1):
        add(f"FS2_TUNE_TAPREG {v}", "gemm", 4096, 128, 256, 1024, 9, {T_TAPREG: v})
    add("tap-register with FS2_TUNE_NT_GROUP 2", "gemm", 24576, 512, 256, 1024, 9, {T_NT_GROUP: 2})
    # ---- halo kernel
    add("k=3 256 -> 1024 at T 512: 8-wave 256 x 128", "gemm", 24576, 512, 256, 1024, 3, lens=1)
    add("... FS2_TUNE_NT_HALO 1: 4-wave 128 x 128", "gemm", 24576, 512, 256, 1024, 3, {T_NT_HALO: 1})
    add("T % 128 == 64: 64 x 128", "gemm", 24576, 192, 256, 1024, 3)
    add("k=3 512 -> 512 at T 128: 128 x 128", "gemm", 16384, 128, 512, 512, 3)
    add("... forced split of 128 x 128", "gemm", 16384, 128, 512, 512, 3, {T_HALO_SPLITK: 2})
    add("128 x 64", "gemm", 4096, 128, 256, 512, 3)
    add("... forced split of 128 x 64", "gemm", 4096, 128, 512, 512, 3, {T_HALO_SPLITK: 2})
    add("FS2_TUNE_NT_HALO 2 on a small grid", "gemm", 4096, 128, 256, 512, 3, {T_NT_HALO: 2})
    add("encoder k=9 data gradient (T 128): 128 x 64 split-K", "gemm", 6144, 128, 1024, 256, 9, lens=1)
    for v in (-1, -2, 2, 4):
        add(f"... FS2_TUNE_HALO_SPLITK {v}", "gemm", 6144, 128, 1024, 256, 9, {T_HALO_SPLITK: v})
    add("T % 128 != 0: 64 x 64 split-K", "gemm", 6144, 192, 1024, 256, 9)
    add("64 x 64 unsplit", "gemm", 1024, 128, 256, 256, 3)
    add("k=9 with FS2_TUNE_TAPREG -1, NT_HALO -1: tap-major 64 x 64, K >= 4096", "gemm", 1024, 128, 512,
        256, 9, {T_TAPREG: -1, T_NT_HALO: -1})
    # vocoder epilogue / dilation on the four 4-wave halo tiles (HX 16 and 64)
    for name, r, T, co in (("128 x 128", 16384, 128, 512), ("64 x 128", 16320, 192, 512),
                           ("128 x 64", 4096, 128, 512), ("64 x 64", 1024, 128, 256)):
        add(f"vocoder epilogue, halo {name}", "gemm_ex", r, T, 128, co, 3, flags=OUT_BF16 | LRELU)
        add(f"dilated vocoder conv, halo {name}", "gemm_ex", r, T, 128, co, 3, dil=9)
    # narrow vocoder convs
    add("vocoder c_out <= 32", "gemm_ex", 16384, 128, 64, 32, 7, flags=OUT_BF16 | LRELU)
    add("vocoder c_out <= 32, c_in % 64 != 0", "gemm_ex", 16384, 128, 80, 32, 7, flags=OUT_BF16 | LRELU)
    add("vocoder c_out == 64, HX 16", "gemm_ex", 16384, 128, 64, 64, 3, flags=OUT_BF16 | LRELU)
    add("vocoder c_out == 64, HX 64", "gemm_ex", 16384, 128, 64, 64, 3, dil=9)
    add("vocoder c_out == 64, no halo (T % 128 != 0)", "gemm_ex", 16320, 192, 64, 64, 3, flags=OUT_BF16 | LRELU)
    add("vocoder c_out == 64, no halo, c_in % 64 != 0", "gemm_ex", 16384, 128, 80, 64, 3, flags=OUT_BF16 | LRELU)
    add("vocoder c_out == 64, FS2_TUNE_NT_HALO -1", "gemm_ex", 16384, 128, 64, 64, 3, {T_NT_HALO: -1}, dil=3)
    # ---- tap-major kernel: three tilings x stages x (K1, tap-aligned, general), vocoder builds
    tiles = (("128 x 128", 16384, 512), ("128 x 64", 4096, 512), ("64 x 64", 1024, 256))
    for name, r, co in tiles:
        for st in (0, 1, 2, 3, 4):
            kn = {T_GEMM_STAGES: st} if st else {}
            add(f"k=1 {name}, stages knob {st}: K1", "gemm", r, 128, 256, co, 1, kn, flags=OUT_BF16 | BIAS)
            add(f"... FS2_TUNE_NT_K1 -1", "gemm", r, 128, 256, co, 1, {**kn, T_NT_K1: -1})
            add(f"... c_in % 64 != 0", "gemm", r, 128, 80, co, 1, kn)
        add(f"vocoder k=1 {name}", "gemm_ex", r, 128, 256, co, 1, flags=OUT_BF16 | LRELU)
        add(f"vocoder k=1 {name}, c_in % 64 != 0", "gemm_ex", r, 128, 80, co, 1, flags=OUT_BF16 | LRELU)
    add("64 x 64 with K >= 4096: four stages", "gemm", 1024, 128, 4096, 256, 1)
    add("... general build", "gemm", 1024, 128, 4096, 256, 1, {T_NT_K1: -1})
    add("not vec: c_out 1, fp32 output", "gemm", 1024, 128, 256, 1, 1, flags=BIAS)
    for v in (1, 2, 3):
        add(f"FS2_TUNE_NT_TILE {v}", "gemm", 4096, 128, 256, 512, 1, {T_NT_TILE: v})
    # FS2_TUNE_GEMM_STAGES on k=5 / k=9 shapes: no effect on the halo and tap-register kernels
    for st in (1, 2, 3, 4):
        add(f"k=5 halo, stages knob {st}", "gemm", 4096, 128, 256, 512, 5, {T_GEMM_STAGES: st})
        add(f"k=9 tap-register, stages knob {st}", "gemm", 24576, 512, 256, 1024, 9, {T_GEMM_STAGES: st})
        add(f"k=5 c_in % 64 != 0 (tap-major), stages knob {st}", "gemm", 4096, 128, 80, 512, 5, {T_GEMM_STAGES: st})
    # ---- LayerNorm epilogues
    for op in ("ln", "ln_bwd"):
        add(f"{op} K1", op, 1024, 128, 256, 256, 1, lens=1)
        add(f"{op} tap-aligned", op, 1024, 128, 256, 256, 1, {T_NT_K1: -1})
        add(f"{op} tap-aligned k=3", op, 1024, 128, 256, 256, 3)
        add(f"{op} c_in % 64 != 0", op, 1024, 128, 80, 256, 1)
        add(f"{op} FS2_TUNE_LN_TILE 1", op, 1024, 128, 256, 256, 1, {T_LN_TILE: 1})
        add(f"{op} FS2_TUNE_LN_TILE 1, c_in % 64 != 0", op, 1024, 128, 80, 256, 1, {T_LN_TILE: 1})
    # ---- weight gradient
    add("k=1 grouped, 1 job", "wgrad", 4096, 128, 256, 768, 1)
    add("k=1 grouped, 3 jobs", "k1_multi", 4096, 128, 0, 0, 1,
        jobs=[[256, 768, 1], [256, 256, 0], [1024, 256, 1]])
    for v in (2, 3):
        add(f"k=1 grouped, FS2_TUNE_WGRAD_K1M_STAGES {v}", "wgrad", 4096, 128, 256, 768, 1, {T_K1M_STAGES: v})
    for taps in (3, 5, 9):
        add(f"80-channel conv k={taps} (wide, split)", "wgrad", 4096, 128, 80, 512, taps, lens=1)
    add("wide without splits", "wgrad", 256, 128, 80, 512, 5)
    add("FS2_TUNE_WGRAD_WIDE 1 on 64-multiples", "wgrad", 4096, 128, 256, 256, 3, {T_WGRAD_WIDE: 1})
    add("FS2_TUNE_WGRAD_WIDE 4", "wgrad", 4096, 128, 256, 256, 3, {T_WGRAD_WIDE: 4}, db=0)
    add("FS2_TUNE_WGRAD_WIDE 3", "wgrad", 4096, 128, 256, 256, 3, {T_WGRAD_WIDE: 3})
    add("k=9 (band)", "wgrad", 4096, 128, 256, 1024, 9, lens=1)
    add("non-64-multiple k=3 (band; wide off)", "wgrad", 4096, 128, 80, 512, 3, {T_WGRAD_WIDE: -1})
    add("non-64-multiple k=5 (band; wide off)", "wgrad", 4096, 128, 80, 512, 5, {T_WGRAD_WIDE: -1})
    add("FS2_TUNE_WGRAD_BAND 4", "wgrad", 4096, 128, 512, 512, 3, {T_WGRAD_BAND: 4})
    add("FS2_TUNE_WGRAD_BAND 3 below 128 tiles", "wgrad", 4096, 128, 80, 512, 3, {T_WGRAD_WIDE: -1, T_WGRAD_BAND: 3})
    add("64-multiple k=3 (halo + wgrad_reduce_rows)", "wgrad", 4096, 128, 256, 256, 3)
    add("64-multiple k=5 (halo + wgrad_reduce_rows)", "wgrad", 4096, 128, 512, 512, 5, db=0)
    add("k=9 FS2_TUNE_WGRAD_HALO 1 (halo)", "wgrad", 4096, 128, 256, 1024, 9, {T_WGRAD_HALO: 1})
    add("taps x c_in > 9216 (wgrad_reduce_taps)", "wgrad", 4096, 128, 1088, 64, 9, {T_WGRAD_HALO: 1})
    for tile in (0, 64, 128):
        add(f"k=3 FS2_TUNE_WGRAD_HALO -1, tile {tile} (tap-major)", "wgrad", 4096, 128, 256, 256, 3,
            {T_WGRAD_HALO: -1, T_WGRAD_TILE: tile})
        add(f"k=3 FS2_TUNE_WGRAD_HALO 1, tile {tile}", "wgrad", 4096, 128, 256, 256, 3,
            {T_WGRAD_HALO: 1, T_WGRAD_TILE: tile})
    for name, ci, co in (("64-wide", 256, 256), ("128-wide", 1024, 1024)):
        for st in (0, 1, 2, 3, 4):
            add(f"FS2_TUNE_WGRAD_K1 -1, {name} tiles, stages knob {st}", "wgrad", 4096, 128, ci, co, 1,
                {T_WGRAD_K1: -1, T_WGRAD_STAGES: st})
    add("FS2_TUNE_WGRAD_K1 -1 with FS2_TUNE_WGRAD_SPLITS 3", "wgrad", 4096, 128, 256, 256, 1,
        {T_WGRAD_K1: -1, T_WGRAD_SPLITS: 3})
    add("FS2_TUNE_WGRAD_K1 -1 with FS2_TUNE_WGRAD_SPLITS 7", "wgrad", 4096, 128, 256, 256, 1,
        {T_WGRAD_K1: -1, T_WGRAD_SPLITS: 7})
    return rows


def run():
    import torch
    from importlib import import_module
    lib = import_module("mid-attribute-speaker-generation_amd._lib").lib
    dev = "cuda:0"
    bf, f32 = torch.bfloat16, torch.float32
    sep_src = torch.zeros(8, dtype=f32, device=dev)
    sep_dst = torch.zeros(8, dtype=bf, device=dev)

    def p(t):
        return t.data_ptr() if t is not None else None

    for i, r in enumerate(table()):
        R, T, ci, co, taps, pad = r["rows"], r["T"], r["c_in"], r["c_out"], r["taps"], r["pad"]
        lens = torch.full((max(R // T, 1) + 1,), T - 3, dtype=torch.int64, device=dev) if r["lens"] else None
        for k, v in r["knobs"].items():
            lib.fs2_set_tuning(int(k), v)
        try:
            if r["op"] in ("gemm", "gemm_ex", "ln", "ln_bwd"):
                x = torch.zeros(R, ci, dtype=bf, device=dev)
                w = torch.zeros(co, taps * ci, dtype=bf, device=dev)
                bias = torch.zeros(co, dtype=f32, device=dev)
            if r["op"] in ("gemm", "gemm_ex"):
                out_bf = r["flags"] & OUT_BF16
                y = torch.zeros(R, co, dtype=bf if out_bf else f32, device=dev)
                b = bias if r["flags"] & BIAS else None
                if r["op"] == "gemm":
                    lib.fs2_conv_gemm(1, p(x), ci, p(w), p(y), co, R, T, ci, co, taps, pad, p(lens), p(b),
                                      r["flags"], None, 0, None)
                else:
                    lib.fs2_conv_gemm_ex(1, p(x), ci, p(w), p(y), co, R, T, ci, co, taps, pad, r["dil"],
                                         p(lens), p(b), r["flags"], None, 0, 0.1, 1.0, None, 0.0, None)
            elif r["op"] == "ln":
                g = torch.ones(256, dtype=f32, device=dev)
                o, xh = (torch.zeros(R, 256, dtype=f32, device=dev) for _ in range(2))
                ot = torch.zeros(R, 256, dtype=bf, device=dev)
                rs = torch.zeros(R, dtype=f32, device=dev)
                lib.fs2_conv_gemm_ln(p(x), ci, p(w), R, T, ci, 256, taps, pad, p(lens), p(bias), None, p(g),
                                     p(g), p(o), p(ot), p(xh), p(rs), 0.0, None, 0, None)
            elif r["op"] == "ln_bwd":
                g, dg, dbeta, dbias = (torch.ones(256, dtype=f32, device=dev) for _ in range(4))
                aux, xh, dres = (torch.zeros(R, 256, dtype=f32, device=dev) for _ in range(3))
                dyt = torch.zeros(R, 256, dtype=bf, device=dev)
                rs = torch.ones(R, dtype=f32, device=dev)
                n = lib.fs2_ln_bwd_ws_bytes(R, 256)
                ws = torch.zeros(n // 4 + 4, dtype=f32, device=dev)
                lib.fs2_conv_gemm_ln_bwd(p(x), ci, p(w), R, T, ci, 256, taps, pad, p(lens), p(aux), p(xh),
                                         p(rs), p(g), p(dg), p(dbeta), p(dbias), 0.0, None, 0, p(dres), 0,
                                         p(dyt), p(ws), n, None)
            elif r["op"] == "wgrad":
                dy = torch.zeros(R, co, dtype=bf, device=dev)
                x = torch.zeros(R, ci, dtype=bf, device=dev)
                dw = torch.zeros(co, ci * taps, dtype=f32, device=dev)
                db = torch.zeros(co, dtype=f32, device=dev) if r["db"] else None
                n = lib.fs2_conv_wgrad_ws_bytes(R, ci, co, taps)
                ws = torch.zeros(n // 4 + 4, dtype=f32, device=dev)
                lib.fs2_conv_wgrad(1, p(dy), co, p(x), ci, p(dw), p(db), R, T, ci, co, taps, pad, p(lens),
                                   p(ws), n, None)
            else:
                keep, jobs = [], []
                for jci, jco, jdb in r["jobs"]:
                    dy = torch.zeros(R, jco, dtype=bf, device=dev)
                    x = torch.zeros(R, jci, dtype=bf, device=dev)
                    dw = torch.zeros(jco, jci, dtype=f32, device=dev)
                    db = torch.zeros(jco, dtype=f32, device=dev) if jdb else None
                    keep += [dy, x, dw, db]
                    jobs += [p(dy), jco, p(x), jci, p(dw), p(db) or 0, jci, jco]
                jt = torch.tensor(jobs, dtype=torch.int64)
                n = lib.fs2_conv_wgrad_k1_multi_ws_bytes(jt.data_ptr(), len(r["jobs"]), R)
                ws = torch.zeros(n // 4 + 4, dtype=f32, device=dev)
                lib.fs2_conv_wgrad_k1_multi(1, jt.data_ptr(), len(r["jobs"]), R, T, p(lens), p(ws), n, None)
        finally:
            for k in r["knobs"]:
                lib.fs2_set_tuning(int(k), 0)
        lib.fs2_cast_bf16(p(sep_src), p(sep_dst), 1, None)
        torch.cuda.synchronize()
    print(f"conv_plan_probe: {i + 1} rows issued")


def golden(trace_csv, parent, out_json, cu_count=256):
    import csv
    rows = table()
    per_row, cur = [], []
    trace = sorted(csv.DictReader(open(trace_csv)), key=lambda d: int(d["Dispatch_Id"]))  # dispatch order
    for d in trace:
        name = d["Kernel_Name"]
        if "fs2::" not in name:
            continue
        wgs = 1
        for ax in "XYZ":
            wgs *= int(d["Grid_Size_" + ax]) // max(int(d["Workgroup_Size_" + ax]), 1)
        short = name.split("fs2::", 1)[1].split("(")[0]
        if short == SEPARATOR:
            per_row.append(cur)
            cur = []
        else:
            cur.append([short, wgs])
    assert len(per_row) == len(rows), (len(per_row), len(rows))
    for r, k in zip(rows, per_row):
        r["kernels"] = k
    with open(out_json, "w") as f:  # one row per line
        f.write('{"parent": %s, "cu_count": %d,\n "not_reached": %s,\n "rows": [\n  ' %
                (json.dumps(parent), cu_count, json.dumps(NOT_REACHED)))
        f.write(",\n  ".join(json.dumps(r) for r in rows) + "\n ]}\n")
    print(f"{out_json}: {len(rows)} rows, {len({k[0] for r in rows for k in r['kernels']})} kernel instances")


# kernel instances the dispatch builds but no call reaches, with the reason
NOT_REACHED = {
    "conv_gemm_nt_glds<128, 32, 2, true, false, true>": "128 x 32 tiles are chosen for vocoder calls only; the non-vocoder builds come with the tile's template",
    "conv_gemm_nt_glds<128, 32, 2, true, false, false>": "as above",
    "conv_gemm_nt_glds<128, 32, 2, false, false, false>": "as above",
}

if __name__ == "__main__":
    if sys.argv[1] == "run":
        signal.alarm(240)  # the probe's own time limit
        run()
    else:
        golden(sys.argv[2], sys.argv[3], sys.argv[4])
