"""Generator of tests/golden/gemm_plans.json: what the default dispatch of vis_gemm_bf16 / vis_gemm_fp8 launches, over a sweep.

Needs no GPU: hip.gemm_plan / hip.gemm_fp8_plan are host arithmetic (vis_gemm_bf16_plan / vis_gemm_fp8_plan make no HIP call).
The sweep crosses every branch of both plan functions: M around the tile heights, the 1024-row threshold of the mixed plans
and the 32768-row cap of the plan slots; N with ragged tails, thin remainders and the production widths; K from one K-step
to the down projection's 18944; no activation and SwiGLU (where N % 32 == 0), with and without a residual; for fp8 the
plain and the split-K call.  (M = 127 is left out to keep the file under 300 KB: no branch tells it from M = 1 or 128.)

The file holds the sweep's axes and, in the order of points(), one short list per call:
    [wide, nt, kernel id, first W row, W rows, tiles_m, tiles_n (, kernel id, first W row, ...: one group per launch)]
The arguments are not repeated per row - points() IS the key, and tests/test_gemm_exact.py checks that the axes in the
file are the axes here before it compares.

Usage:  python tests/golden/gen_gemm_plans.py [--out FILE]
VIS_HIP_LIB=<another build of libvis_hip.so> records that build instead: the committed table was recorded from the build of
the commit BEFORE a change to the dispatch, and the changed build must reproduce it byte for byte.  Re-record it, on purpose,
only when a change is meant to move the default dispatch.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "gemm_plans.json")
ACT_NONE, ACT_SWIGLU = 0, 3
AXES = {
    "M": [1, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2249, 2816, 4900, 5156, 19600, 32769],
    "N": [128, 252, 256, 260, 768, 1280, 3584, 3840, 4608, 5120, 6144, 12296, 37888],
    "K_bf16": [64, 128, 512, 1024, 1088, 1280, 3584, 4096, 5120, 18944],
    "K_fp8": [128, 512, 1024, 1152, 1280, 3584, 4096, 5120, 18944],
}
GEMM_ENV = ("VIS_GEMM_TILE", "VIS_GEMM8_TILE", "VIS_GEMM_MIX1", "VIS_GEMM_HALF", "VIS_GEMM_WIDE", "VIS_GEMM_NT")


def points(entry: str):
    """(M, N, K, act, residual, split) of every call of the sweep, in the order of the table's rows.  SwiGLU takes no
    residual and needs N % 32 == 0; a split-K call takes no SwiGLU and needs N % 8 == 0 (both entries reject the rest)."""
    for split in ((False,) if entry == "bf16" else (False, True)):
        for M in AXES["M"]:
            for N in AXES["N"]:
                if split and N % 8:
                    continue
                for K in AXES["K_" + entry]:
                    yield M, N, K, ACT_NONE, False, split
                    yield M, N, K, ACT_NONE, True, split
                    if N % 32 == 0 and not split:
                        yield M, N, K, ACT_SWIGLU, False, split


def plan_rows(hip, entry: str) -> list:
    names = hip.GEMM_KERNEL_NAMES if entry == "bf16" else hip.GEMM_FP8_KERNEL_NAMES
    ids = {name: k for k, name in names.items()}
    rows = []
    for M, N, K, act, residual, split in points(entry):
        if entry == "bf16":
            p = hip.gemm_plan(M, N, K, act=act, residual=residual)
        else:
            p = hip.gemm_fp8_plan(M, N, K, act=act, residual=residual, split=split)
        row = [int(p["wide"]), int(p["nt"])]
        for l in p["launches"]:
            row += [ids[l["kernel"]], l["n0"], l["ncols"], l["tiles_m"], l["tiles_n"]]
        rows.append(row)
    return rows


def dumps(table: dict) -> str:
    """One row per line, no spaces: the file stays small and a moved plan shows as one changed line."""
    out = ['{"axes":' + json.dumps(table["axes"], separators=(",", ":"))]
    for entry in ("bf16", "fp8"):
        out.append(',"%s":[\n%s\n]' % (entry, ",\n".join(json.dumps(r, separators=(",", ":")) for r in table[entry])))
    return "\n".join(out) + "}\n"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    for v in GEMM_ENV:
        if v in os.environ:
            raise SystemExit(f"{v} is set: the table records the default dispatch")
    from vision_inspection_system_amd import hip
    table = {"axes": AXES, "bf16": plan_rows(hip, "bf16"), "fp8": plan_rows(hip, "fp8")}
    with open(args.out, "w") as f:
        f.write(dumps(table))
    print(f"{args.out}: {len(table['bf16'])} bf16 rows, {len(table['fp8'])} fp8 rows from {hip.LIB_PATH}")


if __name__ == "__main__":
    main()
