"""The exact-GEMM case table is what it claims to be (no GPU): through the host-only plan queries (vis_gemm_bf16_plan /
vis_gemm_fp8_plan - the launchers launch from the same plan) every kernel the default dispatch can choose is reached with
both epilogue forms and every epilogue kind, the production shapes resolve to the kernels the comments name, and the
builders' own conditions (representability, live k, canaries) hold for every case."""
import os

import pytest
import torch

import gemm_exact as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    if not os.path.exists(os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")):
        import __graft_entry__ as g
        g.build()
    for v in ("VIS_GEMM_TILE", "VIS_GEMM_MIX1", "VIS_GEMM_HALF", "VIS_GEMM_WIDE", "VIS_GEMM_NT", "VIS_GEMM8_TILE"):
        assert v not in os.environ, f"{v} is set: the table is stated for the default dispatch"
    from vision_inspection_system_amd import hip as h
    h.load()
    return h


def plan_of(hip, case):
    lda, ldw, ldc, ldr, off = case.ld()
    fn = hip.gemm_plan if case.entry == "bf16" else hip.gemm_fp8_plan
    return fn(case.M, case.N, case.K, act=case.act, ldc=ldc, ldr=ldr, residual=case.has_residual, aligned16=off == 0)


def plan_class(case, plan):
    """The name of the dispatch branch a case runs."""
    k = plan["kernels"]
    if case.entry == "fp8" and k == ("128x128",):
        return "128x128 (M < 1024)" if case.M < 1024 else "128x128 (by cost)"
    return " + ".join(k)


REQUIRED = {
    "bf16": ["128x128", "128x256_pp", "256x256_pp", "256x256_pp + 128x256_pp", "256x256_pp + 128x128"],
    "fp8": ["128x128 (M < 1024)", "128x128 (by cost)", "256x256_pp", "256x256_pp + 128x128"],
}


def test_table_reaches_every_kernel_epilogue_and_kind(hip):
    seen, nt = set(), set()
    for c in G.CASES:
        p = plan_of(hip, c)
        seen.add((c.entry, plan_class(c, p), p["wide"], c.kind))
        if p["nt"]:
            nt.add(c.entry)
    missing = []
    for entry, classes in REQUIRED.items():
        for cls in classes:
            for wide in (True, False):
                for kind in G.KINDS:
                    if entry == "fp8" and kind == "bias_swiglu":
                        continue
                    if (entry, cls, wide, kind) not in seen:
                        missing.append(f"{entry} {cls} {'wide' if wide else 'direct'} {kind}")
    assert not missing, "no case runs: " + "; ".join(missing)
    assert nt == {"bf16", "fp8"}, f"non-temporal stores only reached for {sorted(nt)}"
    # SwiGLU in a mixed plan: the remainder's output columns start at n_off / 2
    assert any(c.act == 3 and len(plan_of(hip, c)["launches"]) == 2 for c in G.CASES if c.entry == "bf16")
    assert any(c.act == 3 and len(plan_of(hip, c)["launches"]) == 2 for c in G.CASES if c.entry == "fp8")


def test_pingpong_kernels_see_odd_and_even_k_tile_counts(hip):
    """Both parities of the K-tile count on each ping-pong kernel (their schedules alternate buffers), by the plan query."""
    parity = {}
    for c in G.CASES:
        for k in plan_of(hip, c)["kernels"]:
            if k.endswith("_pp"):
                parity.setdefault((c.entry, k), set()).add((c.K // c.kstep) % 2)
    assert set(parity) == {("bf16", "256x256_pp"), ("bf16", "128x256_pp"), ("fp8", "256x256_pp")}
    assert all(v == {0, 1} for v in parity.values()), parity


def test_table_has_the_edges():
    """M around the tile heights, N tails that are not multiples of 8, the K values of the issue."""
    for entry in ("bf16", "fp8"):
        cs = [c for c in G.CASES if c.entry == entry]
        assert {1, 127, 128, 129, 255, 256, 257} <= {c.M for c in cs}
        assert {4, 124, 132, 252, 260} <= {c.N % 256 for c in cs if c.N % 8 == 4} | {c.N for c in cs}
        ks = {c.K for c in cs}
        assert {128, 512, 18944} <= ks
        assert ({64, 576, 1088} <= ks) if entry == "bf16" else (1152 in ks)
    assert max(c.M * c.N * c.K for c in G.CASES) < 2e11
    assert all(c.M <= 600 for c in G.CASES if c.K == 18944)


# what each production shape runs (M, N, K, kind) -> launches as (kernel, first W row, tiles_m, tiles_n)
PRODUCTION = [
    ((2249, 4608, 3584, "bias"), [("256x256_pp", 0, 9, 18)]),                                   # LLM qkv
    ((2249, 3584, 3584, "residual"), [("128x256_pp", 0, 18, 14)]),                              # LLM o
    ((2249, 37888, 3584, "swiglu"), [("256x256_pp", 0, 9, 142), ("128x256_pp", 36352, 18, 6)]), # LLM gate/up
    ((4900, 5120, 1280, "bias_quickgelu"), [("256x256_pp", 0, 20, 20)]),                        # ViT fc1
    ((4900, 1280, 5120, "residual"), [("128x256_pp", 0, 39, 5)]),                               # ViT fc2
    ((4900, 3840, 1280, "bias"), [("256x256_pp", 0, 20, 12), ("128x256_pp", 3072, 39, 3)]),     # ViT qkv: 300 tiles = 1 round + 44
    ((2300, 768, 1024, "bias"), [("128x256_pp", 0, 18, 3)]),
    ((2049, 12296, 1088, "bias"), [("256x256_pp", 0, 9, 49)]),
    ((4096, 6144, 1024, "residual"), [("256x256_pp", 0, 16, 24)]),
    # one whole round + a thin remainder (VIS_GEMM_MIX1; the four-image shapes of tools/probes/gemm_mix_probe.py):
    ((5156, 3584, 3584, "residual"), [("256x256_pp", 0, 21, 12), ("128x256_pp", 3072, 41, 2)]),   # LLM o x4: 294 tiles = 1 round + 38
    ((2816, 6144, 4096, "bias"), [("256x256_pp", 0, 11, 23), ("128x256_pp", 5888, 22, 1)]),       # Auditor qkv x4: 264 = 1 round + 8
    ((5156, 4608, 3584, "bias"), [("256x256_pp", 0, 21, 18)]),                                    # LLM qkv x4: 378 tiles, two rounds
    ((2816, 4096, 4096, "residual"), [("256x256_pp", 0, 11, 16)]),                                # Auditor o x4: 176 tiles
]


@pytest.mark.parametrize("shape,want", PRODUCTION, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_production_shapes_resolve_to_their_kernels(hip, shape, want):
    M, N, K, kind = shape
    p = hip.gemm_plan(M, N, K, act=G.ACT_OF[kind], residual=kind.endswith("residual"))
    got = [(l["kernel"], l["n0"], l["tiles_m"], l["tiles_n"]) for l in p["launches"]]
    assert got == want
    assert p["wide"]                                   # contiguous, N % 8 == 0
    assert p["nt"] == (M * (N // 2 if kind == "swiglu" else N) * 2 >= 64 << 20)
    # the launches tile the W rows exactly once
    assert sum(l["ncols"] for l in p["launches"]) == N and p["launches"][0]["n0"] == 0
    for a, b in zip(p["launches"], p["launches"][1:]):
        assert b["n0"] == a["n0"] + a["ncols"] and a["ncols"] % 256 == 0


def test_fp8_production_plans(hip):
    big, small = "256x256_pp", "128x128"
    want = {(2249, 4608, 3584): [(big, 0, 9, 18)], (2249, 3584, 3584): [(small, 0, 18, 28)],
            (2249, 37888, 3584): [(big, 0, 9, 142), (small, 36352, 18, 12)],
            (4900, 5120, 1280): [(big, 0, 20, 20)], (4900, 1280, 5120): [(small, 0, 39, 10)],
            (4900, 3840, 1280): [(big, 0, 20, 12), (small, 3072, 39, 6)], (300, 520, 1024): [(small, 0, 3, 5)],
            # four images (378 / 294 / 264 big tiles: whole rounds on the big tile, the rest on the small one)
            (5156, 4608, 3584): [(big, 0, 21, 12), (small, 3072, 41, 12)], (5156, 3584, 3584): [(big, 0, 21, 12), (small, 3072, 41, 4)],
            (2816, 6144, 4096): [(big, 0, 11, 23), (small, 5888, 22, 2)], (2816, 4096, 4096): [(big, 0, 11, 16)]}
    for (M, N, K), w in want.items():
        got = [(l["kernel"], l["n0"], l["tiles_m"], l["tiles_n"]) for l in hip.gemm_fp8_plan(M, N, K)["launches"]]
        assert got == w, (M, N, K)
        assert hip.gemm_fp8_plan(M, N, K, split=True)["kernels"] == (big,)     # split-K: always the big tile


@pytest.fixture(scope="module")
def plan_table():
    """tests/golden/gemm_plans.json: the default dispatch over a sweep, recorded by tests/golden/gen_gemm_plans.py."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_gemm_plans as gen
    with open(gen.OUT) as f:
        table = json.load(f)
    assert table["axes"] == gen.AXES, "the recorded table was made for another sweep: re-record it (gen_gemm_plans.py)"
    return gen, table


def test_plans_match_the_recorded_table(hip, plan_table):
    """The default dispatch did not move: every plan of the sweep (launch list, wide, nt) equals the recorded one."""
    gen, table = plan_table
    for entry in ("bf16", "fp8"):
        points, got = list(gen.points(entry)), gen.plan_rows(hip, entry)
        assert len(points) == len(got) == len(table[entry])
        moved = [(p, g, w) for p, g, w in zip(points, got, table[entry]) if g != w]
        assert not moved, (f"{entry}: {len(moved)} plans differ from the table; first (M, N, K, act, residual, split) = "
                           f"{moved[0][0]}: now {moved[0][1]}, recorded {moved[0][2]}")


def test_kernel_names_cover_exactly_what_the_plans_can_return(hip, plan_table):
    _, table = plan_table
    seen = {e: {k for row in table[e] for k in row[2::5]} for e in ("bf16", "fp8")}
    assert seen == {"bf16": {1, 7, 8}, "fp8": {1, 7}}
    assert set(hip.GEMM_KERNEL_NAMES) == seen["bf16"] and set(hip.GEMM_FP8_KERNEL_NAMES) == seen["fp8"]
    assert all(hip.GEMM_FP8_KERNEL_NAMES[k] == hip.GEMM_KERNEL_NAMES[k] for k in seen["fp8"])   # an id means one tile


_OVERRIDE_CHILD = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from vision_inspection_system_amd import hip
lib = hip.load()
buf = (ctypes.c_int * 23)()
ptr = ctypes.cast(buf, ctypes.c_void_p)
out = {}
n = lib.vis_gemm_bf16_plan(2249, 4608, 3584, 4608, 0, 0, 0, 1, ptr, 23)
out["bf16"] = list(buf[:3 + 5 * n]) if n else 0
n = lib.vis_gemm_fp8_plan(2249, 4608, 3584, 4608, 0, 0, 0, 1, 0, ptr, 23)
out["fp8"] = list(buf[:3 + 5 * n]) if n else 0
import torch
out["gpu_initialised"] = torch.cuda.is_initialized()
print(json.dumps(out))
"""


def test_tile_override_values(hip):
    """VIS_GEMM_TILE takes 1, 7, 8 and VIS_GEMM8_TILE 1, 7 - the ids of kernels that exist; any other non-zero value makes
    the plan query return 0 (and the launchers VIS_ERR_ARG) instead of quietly running the default; VIS_GEMM_PP is no longer
    read.  The variables are read once per process, hence the children (all started at once; they only ask for plans)."""
    import json
    import subprocess
    import sys
    # (VIS_GEMM_TILE, VIS_GEMM8_TILE) -> (kernel id every bf16 launch must have or 0, the same for fp8); None: unset
    settings = {("1", "1"): (1, 1), ("7", "7"): (7, 7), ("8", "4"): (8, 0), ("2", "2"): (0, 0), ("4", None): (0, None),
                ("5", None): (0, None), ("6", None): (0, None), ("3", None): (0, None)}
    base = {k: v for k, v in os.environ.items() if not k.startswith("VIS_GEMM")}

    def start(env):
        return subprocess.Popen([sys.executable, "-c", _OVERRIDE_CHILD, ROOT], env={**base, **env}, stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)
    procs = {key: start({k: v for k, v in zip(("VIS_GEMM_TILE", "VIS_GEMM8_TILE"), key) if v is not None}) for key in settings}
    procs["pp"] = start({"VIS_GEMM_PP": "0"})
    results = {}
    for key, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, f"{key}: {se[-2000:]}"
        results[key] = json.loads(so.strip().splitlines()[-1])
        assert not results[key]["gpu_initialised"]
    lib = hip.load()
    import ctypes
    buf = (ctypes.c_int * 23)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    n = lib.vis_gemm_bf16_plan(2249, 4608, 3584, 4608, 0, 0, 0, 1, ptr, 23)
    default = {"bf16": list(buf[:3 + 5 * n])}
    n = lib.vis_gemm_fp8_plan(2249, 4608, 3584, 4608, 0, 0, 0, 1, 0, ptr, 23)
    default["fp8"] = list(buf[:3 + 5 * n])
    assert default["bf16"][3::5] == [7] and default["fp8"][3::5] == [7]
    for key, want in settings.items():
        for entry, kernel in zip(("bf16", "fp8"), want):
            got = results[key][entry]
            if kernel is None:                       # this entry's variable is unset: its default plan
                assert got == default[entry], (key, entry)
            elif kernel == 0:
                assert got == 0, (key, entry, got)
            else:
                assert got != 0 and got[0] >= 1 and set(got[3::5]) == {kernel}, (key, entry, got)
                assert got[1:3] == default[entry][1:3]                       # epilogue form and store policy: not the tile's business
    assert {e: results["pp"][e] for e in ("bf16", "fp8")} == default


def test_plan_query_argument_checks(hip):
    import ctypes
    lib = hip.load()
    buf = (ctypes.c_int * 23)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vis_gemm_bf16_plan(128, 128, 64, 128, 0, 0, 0, 1, ptr, 23) == 1
    assert list(buf[:8]) == [1, 1, 0, 1, 0, 128, 1, 1]
    assert lib.vis_gemm_bf16_plan(128, 128, 40, 128, 0, 0, 0, 1, ptr, 23) == 0          # K % 64
    assert lib.vis_gemm_bf16_plan(128, 130, 64, 132, 0, 0, 0, 1, ptr, 23) == 0          # N % 4
    assert lib.vis_gemm_bf16_plan(128, 128, 64, 130, 0, 0, 0, 1, ptr, 23) == 0          # ldc % 4
    assert lib.vis_gemm_bf16_plan(128, 128, 64, 128, 0, 0, 0, 1, None, 23) == 0
    assert lib.vis_gemm_bf16_plan(2249, 37888, 3584, 18944, 0, 3, 0, 1, ptr, 8) == 0    # two launches need 13 ints
    assert lib.vis_gemm_fp8_plan(128, 128, 64, 128, 0, 0, 0, 1, 0, ptr, 23) == 0        # K % 128
    assert lib.vis_gemm_fp8_plan(128, 128, 128, 128, 0, 0, 0, 1, 0, ptr, 23) == 1
    # epilogue form: N % 8, ldc % 8, ldr % 8, 16-byte alignment
    assert hip.gemm_plan(128, 128, 64)["wide"] and not hip.gemm_plan(128, 132, 64)["wide"]
    assert not hip.gemm_plan(128, 128, 64, ldc=132)["wide"] and not hip.gemm_plan(128, 128, 64, aligned16=False)["wide"]
    assert not hip.gemm_plan(128, 128, 64, residual=True, ldr=132)["wide"]
    assert hip.gemm_plan(128, 128, 64, residual=True, ldr=136)["wide"]


def test_builders_hold_for_every_case():
    """build() asserts representability (f32-exact pre-activation, bf16-exact output), live k and |x| <= 16 itself; here
    additionally the layouts are what the case says and the tolerance of an activation case stays near one bf16 ulp."""
    for c in G.CASES:
        ops = G.build(c)
        lda, ldw, ldc, ldr, off = c.ld()
        assert ops["ref"].shape == (c.M, c.n_out) and ops["ref"].dtype == torch.float64
        assert (ops["A"].ld, ops["W"].ld, ops["C"].ld, ops["C"].offset) == (lda, ldw, ldc, off)
        assert (ops["R"] is not None) == c.has_residual and (ops["bias"] is not None) == c.has_bias
        if c.layout != "packed":
            assert lda > c.K and ldw > c.K and ldc > c.n_out and ldr != ldc
            assert not bool(torch.isfinite(ops["A"].flat.view(torch.float8_e4m3fn if c.entry == "fp8" else torch.bfloat16)
                                           .float()[~ops["A"].inside()]).any())
        if ops["tol"] is None:
            assert float(ops["ref"].abs().max()) <= 256
        else:
            assert float(ops["pre"].abs().max()) <= 16 and float(ops["pre"].abs().max()) > 2     # not saturated, not trivial
            assert bool((ops["tol"] <= 1.01 * G.bf16_ulp(ops["ref"]) + 1e-5).all())
        if c.entry == "fp8" and c.act != 3:               # neighbouring rows / columns never share a scale
            assert bool((ops["sa"][1:] != ops["sa"][:-1]).all()) and bool((ops["sw"][1:] != ops["sw"][:-1]).all())
        assert G.canary_intact(ops["C"], ops["C"].flat)


def test_canary_checker_sees_a_stray_write():
    c = G.Case("bf16", 5, 8, 64, "plain", "offset8")
    ops = G.build(c)
    flat = ops["C"].flat.clone()
    ops["C"].view(flat).copy_(ops["ref"].to(torch.bfloat16))
    G.check(c, ops, flat)
    for pos in (0, ops["C"].offset + c.n_out, flat.numel() - 1):          # before C, right of row 0, below the last row
        f2 = flat.clone()
        f2[pos] = 1.0
        with pytest.raises(AssertionError, match="outside C"):
            G.check(c, ops, f2)
    f2 = flat.clone()
    ops["C"].view(f2)[4, 7] += 1.0
    with pytest.raises(AssertionError, match="wrong elements"):
        G.check(c, ops, f2)


def test_swiglu_interleave_matches_the_packer():
    from vision_inspection_system_amd.weights import interleave_gate_up
    g, u = torch.arange(64 * 8.0).reshape(64, 8), -torch.arange(64 * 8.0).reshape(64, 8)
    assert torch.equal(G.interleave16(g, u), interleave_gate_up(g, u))
