"""The exact MXFP4 operands are what they claim to be (no GPU): the independent decode agrees with hip.dequantize_mxfp4 on all
16 x 248 (code, byte) pairs, every builder's exactness assertions hold for every shape of tests/test_mxfp4_exact_gpu.py, and
the kernels' walks - restated in mxfp4_exact.walk_gemv / walk_gemm - reach the edge each shape was chosen for."""
import numpy as np
import pytest
import torch

import gemv_exact as G
import mxfp4_exact as M


# ----------------------------------------------------------------------------- decode
def test_decode_agrees_with_the_library_on_every_code_and_byte():
    from vision_inspection_system_amd import hip
    assert M.E2M1.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert M.BYTES[0] == 3 and M.BYTES[-1] == 250 and len(M.BYTES) == 248
    ws = torch.tensor(M.BYTES, dtype=torch.uint8)[:, None]
    wq = (torch.arange(16, dtype=torch.uint8) * 0x11)[None, :].repeat(len(M.BYTES), 1)      # elements 2 c, 2 c + 1 = code c
    mine = M.decode(wq, ws)
    assert torch.equal(mine, hip.dequantize_mxfp4(wq, ws).double())
    want = M.E2M1.repeat_interleave(2)[None, :] * torch.tensor([2.0 ** (b - 127) for b in M.BYTES], dtype=torch.float64)[:, None]
    assert torch.equal(mine, want)
    nz = mine[mine != 0].abs()
    assert float(nz.min()) == 2.0 ** -125 and float(nz.max()) == 6 * 2.0 ** 123
    assert torch.equal(mine.to(torch.bfloat16).double(), mine), "a weight is not an exact (normal) bf16"
    # nibble order: byte 0x21 = code 1 then code 2
    assert M.decode(torch.tensor([[0x21] + [0] * 15], dtype=torch.uint8), torch.tensor([[127]], dtype=torch.uint8))[0, :2].tolist() == [0.5, 1.0]
    assert torch.equal(M.pack(M.unpack(wq)), wq)


# ----------------------------------------------------------------------------- the GEMV walk
def test_gemv_shapes_reach_their_edges():
    w = M.walk_gemv(40968, 32)                       # <8, 2> above 1024 blocks; waves with 1 and with 2 groups
    assert (w["rows"], w["seg"]) == (8, 2) and w["raw_blocks"] > 1024 and w["blocks"] == 1056 and not w["capped"]
    assert set(w["groups"].tolist()) == {1, 2} and w["crossings"] == {"AB"}
    w = M.walk_gemv(152064, 64)                      # the lm_head row count: 3 and 4 groups, odd and even task counts
    assert (w["rows"], w["seg"]) == (8, 2) and w["n_grps"] == 19008 and w["blocks"] == 1490
    assert set(w["groups"].tolist()) == {3, 4} and set(w["tasks"].tolist()) == {3, 4} and w["crossings"] == {"AB", "BA"}
    w = M.walk_gemv(300032, 32)                      # the 2048 cap
    assert w["capped"] and w["blocks"] == 2048 and int(w["groups"].max()) >= 4
    w = M.walk_gemv(75776, 64, swiglu=True)          # <8, 2> SwiGLU, more than one group per wave
    assert (w["rows"], w["seg"]) == (8, 2) and w["n_grps"] == 9472 and int(w["groups"].max()) == 2 and w["blocks"] > 1024
    w = M.walk_gemv(8200, 10272)                     # <2, 5>, nseg = 2, waves with 2 groups: a ring of A B A B
    assert (w["rows"], w["seg"]) == (2, 5) and w["nseg"] == 2 and set(w["groups"].tolist()) == {1, 2}
    assert set(w["tasks"].tolist()) == {2, 4} and w["crossings"] == {"BA"} and w["blocks"] == 1024
    w = M.walk_gemv(8200, 20512)                     # nseg = 3: odd task count, idle lanes in the last segment
    assert w["nseg"] == 3 and set(w["tasks"].tolist()) == {3, 6} and w["tail_blocks"] == 1 and w["crossings"] == {"AB"}
    # the fused norm: (6, 4128) takes the loop path of gv_stage_x_rmsnorm<true> (516 chunks of x).  More than 512 chunks
    # means K > 4096, which the launcher gives to <2, 5>: the loop path cannot meet <2, 2>, which (1002, 704) runs
    w = M.walk_gemv(6, 4128)
    assert w["nch8"] == 516 and (w["rows"], w["seg"]) == (2, 5) and w["nseg"] == 1 and w["idle_waves"] == 1
    w = M.walk_gemv(1002, 704)
    assert (w["rows"], w["seg"]) == (2, 2) and w["nch8"] == 88 and 704 % 128 != 0 and w["nch"] == 22
    assert M.walk_gemv(64, 256, swiglu=True)["rows"] == 2 and M.walk_gemv(16448, 64, swiglu=True)["rows"] == 8
    assert int(M.walk_gemv(16448, 64, swiglu=True)["groups"].max()) == 1     # <8, 2> SwiGLU, one group per wave
    w = M.walk_gemv(M.EVERY_N, M.EVERY_K)
    assert w["seg"] == 5 and w["nch"] == 248 and w["nseg"] == 1
    for N, K in M.GEMV_SHAPES + M.GEMV_NORM_SHAPES + M.GEMV_ROWS_NORM_SHAPES:
        w = M.walk_gemv(N, K)
        assert int(w["groups"].sum()) == w["n_grps"] and w["blocks"] <= 2048 and K % 32 == 0 and K * 2 <= 60 * 1024
    assert all(K * 8 <= 152 * 1024 for _, K in M.GEMV_ROWS_NORM_SHAPES)          # four staged rows in LDS
    # what the older kernel-level shapes reach, as the reason for this file: never two groups, never more than two tasks
    for N, K in [(8, 32), (1002, 704), (260, 2080), (96, 8192), (130, 18944), (8200, 96), (3584, 18944)]:
        w = M.walk_gemv(N, K)
        assert int(w["groups"].max()) <= 1 and int(w["tasks"].max()) <= 2 and w["blocks"] <= 1024


# ----------------------------------------------------------------------------- the MFMA projection's walk
def _reuse(w):
    """(on-the-spot flushes, tiles that START in the reused last set) over all ranges."""
    spot = [(i, e) for i, r in enumerate(w["ranges"]) for e in r if e[5]]
    after = [(i, e) for i, r in enumerate(w["ranges"]) for k, e in enumerate(r) if k > 0 and r[k - 1][5]]
    return spot, after


def test_gemm_shapes_reach_their_edges():
    for B in (33, 64):                               # 5 whole tiles per range > NSEG = 4; 2 valid blocks in the step
        w = M.walk_gemm(131200, 64, B)
        assert w["NSEG"] == 4 and w["per"] == 5 and w["nk"] == 1 and set(w["tiles_per_range"].tolist()) == {5}
        assert not w["starts_inside"].any() and not w["ends_inside"].any() and w["last_step_blocks"] == 2 and w["nslots"] == 1
        assert len(_reuse(w)[0]) == w["nwg"] == 205
    w = M.walk_gemm(131200, 512, 64)                 # per = 9 on nk = 2: cut tiles, 5 tiles per range, 2 slots
    assert w["per"] == 9 and w["nk"] == 2 and w["nslots"] == 2 and int(w["tiles_per_range"].max()) == 5
    assert w["starts_inside"].any() and w["ends_inside"].any()
    spot, after = _reuse(w)
    # a tile flushed on the spot always ran to its last K-step (steps are left in the range, so the kernel's n_here was
    # nk - c_kt): the kernel passes tile_done = true there for every shape.  The cut meets the reuse in the tile AFTER it: a
    # tile that starts in the just-reset set, ends with the range (tile_done false, slot 0) and is completed by the next
    # workgroup in slot 1 - and a range that starts inside a tile (slot 1) and later flushes on the spot
    assert spot and all(e[4] for _, e in spot)
    assert any(not e[4] and e[6] == 0 for _, e in after), "no cut tile starts in the reused set"
    assert any(r[0][2] != 0 and r[0][6] == 1 and any(e[5] for e in r) for r in w["ranges"])
    w = M.walk_gemm(131200, 768, 33)                 # per = 13 on nk = 3
    assert w["per"] == 13 and w["nk"] == 3 and w["NSEG"] == 4 and int(w["tiles_per_range"].max()) >= 5
    assert {r[0][2] for r in w["ranges"]} == {0, 1, 2} and _reuse(w)[0]
    for B, MB in ((5, 1), (17, 2)):                  # 9 tiles per range > NSEG = 8
        w = M.walk_gemm(262272, 64, B)
        assert w["MB"] == MB and w["NSEG"] == 8 and w["per"] == 9 and int(w["tiles_per_range"].max()) == 9 and _reuse(w)[0]
    w = M.walk_gemm(262272, 512, 17)                 # the cut case for NSEG = 8
    assert w["NSEG"] == 8 and w["per"] == 17 and int(w["tiles_per_range"].max()) >= 9 and w["nslots"] == 2
    spot, after = _reuse(w)
    assert spot and any(not e[4] and e[6] == 0 for _, e in after)
    for B, MB in ((5, 1), (17, 2), (33, 4)):         # 4 valid blocks in the ragged last step at every MB, with a cut
        w = M.walk_gemm(65664, 384, B)
        assert w["MB"] == MB and w["last_step_blocks"] == 4 and w["nk"] == 2 and w["per"] == 5 and w["ends_inside"].any()
    N, K, B = M.GEMM_DIRECT                          # direct: 5 whole tiles per workgroup
    w = M.walk_gemm(N, K, B, direct=True)
    assert w["MB"] == 4 and w["per"] == 5 and set(w["tiles_per_range"].tolist()) == {5} and w["nslots"] == 1
    assert not w["ends_inside"].any() and _reuse(w)[0]
    # every flush on the spot has tile_done = true, in every table entry (see above)
    for N, K, Bs in M.GEMM_SHAPES + M.GEMM_WIDE_SHAPES:
        for B in Bs:
            w = M.walk_gemm(N, K, B)
            assert all(e[4] for _, e in _reuse(w)[0])
            done = {}
            for r in w["ranges"]:                   # the slots of a tile are 0 .. n - 1, the last one passes tile_done
                for e in r:
                    done.setdefault(e[0], []).append((e[6], e[4]))
            assert len(done) == w["tiles"]
            for t, segs in done.items():
                assert [s for s, _ in segs] == list(range(len(segs))) and [d for _, d in segs] == [False] * (len(segs) - 1) + [True]
                assert len(segs) <= w["nslots"]
    # the older tests' shapes never reuse a set: at most 4 tiles per range ((1408, 256); 2 in the exact ones), NSEG >= 4
    for N, K in [(128, 64), (1000, 704), (260, 2112), (4608, 3584), (132, 18944), (1408, 256), (256, 704)]:
        for B in (5, 17, 64):
            w = M.walk_gemm(N, K, B)
            assert int(w["tiles_per_range"].max()) <= (4 if N == 1408 else 2) and not _reuse(w)[0]


def test_gemm_slot_count_is_the_librarys():
    from vision_inspection_system_amd import hip
    shapes = [(N, K) for N, K, _ in M.GEMM_SHAPES + M.GEMM_WIDE_SHAPES] + [(M.EVERY_N, M.EVERY_K), (4608, 3584), (132, 18944)]
    for N, K in shapes:
        assert M.walk_gemm(N, K, 64)["nslots"] == hip.decode_gemm_mxfp4_ksplit(N, K), (N, K)


# ----------------------------------------------------------------------------- the builders' own assertions
def _order_check(c, rows=16):
    """The float64 reference equals an f32 evaluation in two orders (first rows of the matrix)."""
    w = M.decode(c["wq"][:rows], c["ws"][:rows])
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(w, c["x"][0].double(), 32, reverse), c["ref"][0, :rows])


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("N,K", M.GEMV_SHAPES)
def test_gemv_case(family, N, K):
    if family == "wide" and K > M.WIDE_MAX_K:
        return
    c = M.case(family, N, K)                         # (asserts the bound, the codes, the scale bytes and the epilogue)
    _order_check(c)
    assert torch.equal(c["ref_br"], (c["ref"] + c["bias"].double()) + c["R"].double())
    if family == "wide" and K // 32 >= M.WIDE_ALL_BYTES_FROM:
        assert set(torch.unique(c["ws"]).tolist()) == set(M.BYTES)


def test_wide_family_covers_all_bytes_on_one_matrix():
    c = M.case("wide", 8200, 10272)
    assert set(torch.unique(c["ws"]).tolist()) == set(M.BYTES)
    w = M.decode(c["wq"][:256], c["ws"][:256])
    p = (w * c["x"][0].double()[None, :]).abs()
    assert float(p.max()) <= 192 and torch.equal(p * 8, (p * 8).round())
    ws = c["ws"].long()
    assert bool((ws[1:] != ws[:-1]).all()) and bool((ws[:, 1:] != ws[:, :-1]).all()), "a neighbour shares a scale byte"


@pytest.mark.parametrize("N,K", M.GEMV_SWIGLU_SHAPES)
def test_swiglu_case(N, K):
    from vision_inspection_system_amd.weights import interleave_gate_up
    c = M.swiglu_case(N, K)
    I = N // 2
    o = torch.arange(I)
    r0 = ((o >> 4) << 5) + (o & 15)                  # the kernel's row mapping (g4_rows)
    rows = torch.cat([r0[:24], r0[:24] + 16])
    w = M.decode(c["wq"][rows], c["ws"][rows])
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(w, c["x"].double(), 32, reverse), torch.cat([c["gate"][:24], c["up"][:24]]))
    g = torch.arange(N, dtype=torch.float32)[:, None]
    assert torch.equal(G.interleave16(g[:I], g[I:]), interleave_gate_up(g[:I], g[I:]))
    tol = G.swiglu_tolerance(c["ref"])
    live = c["gate"] != 0
    wrongs = [torch.roll(c["ref"], 1), torch.nn.functional.silu(c["up"]) * c["gate"]] + ([torch.roll(c["ref"], 16)] if I > 16 else [])
    for wrong in wrongs:
        assert float(((wrong - c["ref"]).abs() > 8 * tol)[live].float().mean()) > 0.9


@pytest.mark.parametrize("N,K,B", [(n, k, 1) for n, k in M.GEMV_NORM_SHAPES] +
                         [(n, k, b) for n, k in M.GEMV_ROWS_NORM_SHAPES for b in (2, 3, 4)])
def test_norm_case(N, K, B):
    c = M.norm_case(N, K, B)                         # (gemv_exact.norm_operands proves the staged row in float64)
    staged = torch.sign(c["x"].double()) * c["norm_w"].double()[None, :]
    assert len({tuple(r.tolist()) for r in torch.sign(c["x"].float())}) == B
    w = M.decode(c["wq"][:6], c["ws"][:6])
    for b in range(B):
        assert torch.equal(G.f32_sum(w, staged[b], 32, b % 2 == 1), c["ref"][b, :6])


@pytest.mark.parametrize("N,K", sorted({(n, k) for n, k, _ in M.GEMM_SHAPES}))
def test_gemm_case_narrow(N, K):
    c = M.case("narrow", N, K, 64)
    _order_check(c, rows=4)
    assert c["bound"] < 2 ** 21


@pytest.mark.parametrize("N,K", sorted({(n, k) for n, k, _ in M.GEMM_WIDE_SHAPES}))
def test_gemm_case_wide(N, K):
    c = M.case("wide", N, K, 64)
    _order_check(c, rows=4)
    assert {3, 250} <= set(torch.unique(c["ws"]).tolist())


def test_every_code_case():
    c = M.every_code_case()                          # (asserts want = x @ decode^T and the 16 x 248 pairs)
    assert c["want"].shape == (M.EVERY_B, M.EVERY_N) and set(c["want"][0].abs().tolist()) == {0, 0.5, 1, 1.5, 2, 3, 4, 6}
    assert c["ws"][:, 0].tolist() == [3] * M.EVERY_N and c["ws"][0].tolist() == M.BYTES
    assert M.EVERY_K % 64 == 0 and M.EVERY_K * 2 <= 60 * 1024
