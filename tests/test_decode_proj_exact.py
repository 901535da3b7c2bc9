"""The exact decode-projection operands and the restated launch geometry are what tests/test_decode_proj_exact_gpu.py
claims (no GPU): segment-block ids never collide, every shape reaches the edge it is named for, the builders' references are
exact and order-independent."""
import numpy as np
import pytest
import torch

import decode_proj_exact as D
import gemv_exact as G


def _shapes():
    return [(N, K, fp8) for N, K, _, _, _ in D.STREAMK_SHAPES for fp8 in (False, True)]


# ----------------------------------------------------------------------------- segment-block ids
def _check_ids(N, K, fp8):
    g = D.streamk_geometry(N, K * (2 if fp8 else 1), fp8)
    ids = g["seg_ids"]
    assert len(np.unique(ids)) == len(ids), f"({N}, {K}): two segments share a block"
    assert ids.size == 0 or (int(ids.min()) >= 0 and int(ids.max()) < g["nblocks"])
    assert ids.size == int(g["ns"][g["ns"] > 1].sum())
    assert int(g["ns"].max()) <= D.MAX_SEGS and g["nwg"] <= D.MAX_WG
    for rows in (16, 32, 64):
        assert g["ws_bytes"][rows] == D.CNT_BYTES + g["nblocks"] * rows * 128 * 4
    return g


@pytest.mark.parametrize("N,K,fp8", _shapes())
def test_segment_block_ids_of_the_shapes(N, K, fp8):
    _check_ids(N, K, fp8)


def test_segment_block_ids_sweep():
    """Small (N, K): every tile count 1 .. 40 against every K-step count 1 .. 130."""
    for tiles in list(range(1, 41)) + [255, 256, 257, 1000]:
        for nk in range(1, 131):
            _check_ids(tiles * 128 - 28, nk * 64, False)


# ----------------------------------------------------------------------------- every shape reaches its edge
def test_streamk_edges_reached():
    geo = {(N, K): D.streamk_geometry(N, K) for N, K, _, _, _ in D.STREAMK_SHAPES}
    for (N, K), g in geo.items():                          # the fp8 twin (K doubled) has the same cut
        g8 = D.streamk_geometry(N, 2 * K, True)
        assert (g8["spb"], g8["nwg"], g8["lcm"], g8["nblocks"]) == (g["spb"], g["nwg"], g["lcm"], g["nblocks"])

    def ns(N, K):
        return sorted(set(geo[(N, K)]["ns"].tolist()))

    def per_range(N, K):
        return sorted(set(geo[(N, K)]["wg_tiles"].tolist()))

    g = geo[(128, 64)]
    assert (g["total"], g["spb"], g["nwg"]) == (1, 1, 1) and g["total"] < 4
    g = geo[(128, 256)]
    assert (g["spb"], g["nwg"], ns(128, 256)) == (4, 1, [1]) and g["spb"] < D.stream_consts(64)["DEPTH"]   # never refilled
    assert ns(128, 1280) == [5] and D.stream_consts(64)["GRP"] == 4 and 5 % 4 == 1       # two rounds, the second of one
    assert ns(128, 4096) == [16] == [D.MAX_SEGS]
    assert [16 // D.stream_consts(B)["GRP"] for B in (16, 32, 64)] == [1, 2, 4]
    g = geo[(128, 6400)]
    assert (g["wg"], g["spb"], g["nwg"], ns(128, 6400), g["lcm"]) == (16, 7, 15, [15], g["total"] + 1)
    assert all(geo[s]["wg"] == D.MAX_WG for s in geo if s != (128, 6400))                # the only shape that halves wg
    assert g["spb"] == D.stream_consts(32)["DEPTH"] == D.stream_consts(64)["DEPTH"] + 1
    g = geo[(384, 640)]
    assert ns(384, 640) == [3] and per_range(384, 640) == [1, 2] and g["lcm"] == 20 < g["total"] and g["nk"] % g["spb"] != 0
    g = geo[(256, 704)]
    assert ns(256, 704) == [3, 4] and g["lcm"] == g["total"] + 1
    assert 1000 % 128 == 104 and 1000 % 32 != 0
    assert ns(6144, 128) == [1] and per_range(6144, 128) == [2]
    g = geo[(262272, 64)]
    assert ns(262272, 64) == [1] and int(g["wg_tiles"].max()) == 9 > D.stream_consts(16)["NSEG"] > D.stream_consts(64)["NSEG"]
    g = geo[(262272, 192)]
    assert g["spb"] == 25 and ns(262272, 192) == [1, 2] and int(g["wg_tiles"].max()) == 9
    # ranges whose tile beyond the NSEG-th is cut between workgroups (tick_s[NSEG - 1], the move of set NSEG - 1 to set 0)
    for B in (17, 64):
        nseg = D.stream_consts(B)["NSEG"]
        s0 = np.arange(g["nwg"]) * g["spb"]
        first_tile = s0 // g["nk"]
        late_cut = [w for w in range(g["nwg"]) for t in range(first_tile[w] + nseg, first_tile[w] + g["wg_tiles"][w])
                    if g["ns"][t] > 1]
        assert late_cut, f"B={B}: no cut tile in the overflow path"
    g = geo[(3584, 18944)]
    assert ns(3584, 18944) == [9, 10]


@pytest.mark.parametrize("fp8", [False, True])
def test_colpar_edges_reached(fp8):
    kstep = 128 if fp8 else 64
    assert D.colpar_geometry(40992, kstep, 4, fp8) is None and D.colpar_geometry(1000, kstep, 4, fp8) is None

    def cnts(N, B):
        g = D.colpar_geometry(N, kstep, B, fp8)
        return g, sorted(g["kinds"])

    for B in D.BATCHES:
        narrow = B > 32
        g, c = cnts(32, B)
        assert (g["nwg"], c, g["kinds"][1]["narrow"]) == (1, [1], narrow)
        g, c = cnts(512, B)
        assert (g["nwg"], c, g["kinds"][1]["depth"]) == (16, [1], 10)
        assert [k // 64 for k in D.COLPAR_K_512] == [1, 9, 10, 11, 56] == D.colpar_nks(512, B, fp8)
        g, c = cnts(9600, B)
        assert (g["units"], c) == (300, [1, 2]) and g["kinds"][1]["narrow"] == narrow and not g["kinds"][2]["narrow"]
        assert 257 <= g["units"] <= 511
        g, c = cnts(19200, B)
        assert c == [2, 3]
        g, c = cnts(35200, B)
        assert (g["units"], c) == (1100, [4, 5]) and g["kinds"][5]["has1"] and not g["kinds"][4]["has1"]
        g, c = cnts(40960, B)
        assert c == [5] and int(g["cnt"].min()) == 5 == D.CP_MAX_UNITS
        for N, _ in D.COLPAR_N:                            # K-steps one below, at and one above every ring depth, and 1
            g = D.colpar_geometry(N, kstep, B, fp8)
            nks = D.colpar_nks(N, B, fp8)
            assert 1 in nks
            for kind in g["kinds"].values():
                assert 3 <= kind["depth"] <= D.CP_MAX_DEPTH and (kind["depth"] - 2) * kind["per"] <= 63
                assert {kind["depth"] - 1, kind["depth"], kind["depth"] + 1} <= set(nks)
    # the depths the restated geometry gives (bf16 / fp8, up to 32 rows / 33..64 rows)
    depth = {(N, B): {c: k["depth"] for c, k in D.colpar_geometry(N, kstep, B, fp8)["kinds"].items()}
             for N in (9600, 19200, 35200, 40960) for B in (32, 64)}
    if not fp8:
        assert depth == {(9600, 32): {1: 10, 2: 10}, (9600, 64): {1: 10, 2: 9}, (19200, 32): {2: 10, 3: 9},
                         (19200, 64): {2: 9, 3: 7}, (35200, 32): {4: 7, 5: 6}, (35200, 64): {4: 6, 5: 5},
                         (40960, 32): {5: 6}, (40960, 64): {5: 5}}
    else:
        assert depth == {(9600, 32): {1: 10, 2: 10}, (9600, 64): {1: 10, 2: 8}, (19200, 32): {2: 10, 3: 8},
                         (19200, 64): {2: 8, 3: 7}, (35200, 32): {4: 7, 5: 6}, (35200, 64): {4: 6, 5: 5},
                         (40960, 32): {5: 6}, (40960, 64): {5: 5}}


# ----------------------------------------------------------------------------- builder self-checks
SMALL = [("bf16", 128, 64), ("bf16", 256, 704), ("bf16", 1000, 192), ("fp8", 128, 128), ("fp8", 384, 1280), ("fp8", 32, 8192)]


@pytest.mark.parametrize("kind,N,K", SMALL)
def test_case_is_exact_and_order_independent(kind, N, K):
    c = D.case(kind, N, K)                                 # (asserts the 2^24 bound, value coverage, the planted column)
    fp8 = kind == "fp8"
    if fp8:
        scale = torch.ldexp(torch.ones((64, K), dtype=torch.float64), (c["xs"].long() - 127).repeat_interleave(32, 1))
        x = G.E4M3[c["xq"].long()] * scale
        w = G.E4M3[c["Wq"].long()]
        assert set(torch.unique(c["Wq"]).tolist()) == set(G.FP8_CODES.tolist()) - {0x80} | {0}
        assert int(c["xs"].min()) == 127 and int(c["xs"].max()) == 127 + D.fp8_smax(K)
        assert bool((c["xs"][:, 1:] != c["xs"][:, :-1]).all()) and bool((c["xs"][1:] != c["xs"][:-1]).all())
    else:
        x, w = c["x"].double(), c["W"].double()
        assert set(torch.unique(w).tolist()) == set(range(-8, 9)) == set(torch.unique(x[0]).tolist())
    assert len({tuple(r.tolist()) for r in x}) == 64, "rows of x must differ"
    for b in (0, 63):
        for reverse in (False, True):
            got = G.f32_sum(w, x[b], 16 if fp8 else 8, reverse) * c["sw"].double()
            assert torch.equal(got, c["acc"][b]), f"f32 sum of row {b}, reverse={reverse}"
    y = (c["acc"] + c["R"].double()).float()
    assert torch.equal(y.double(), c["acc"] + c["R"].double()) and torch.equal(y.to(torch.bfloat16), c["y"])
    assert torch.equal((c["y"].float() * c["nw"].float()[None, :]).to(torch.bfloat16), c["yw"])
    assert len(torch.unique(c["nw"].view(torch.int16) & 0x7F)) == min(N, 128)
    ref = D.ssq_ref(c["y"], 5)
    assert ref.shape == ((N + 31) // 32, 5) and torch.equal(ref.sum(0), (c["y"][:5].double() ** 2).sum(1))


def test_fp8_ranges_follow_k():
    assert [D.fp8_smax(K) for K in (128, 8192, 16383, 16384, 32767, 37888)] == [3, 3, 3, 2, 2, 1]
    for K in (8192, 37888):
        assert 128 * 2 ** D.fp8_smax(K) * K < 2 ** 24


@pytest.mark.parametrize("kind,N,K", [("bf16", 128, 64), ("bf16", 6144, 128), ("fp8", 128, 128), ("fp8", 384, 1280)])
def test_swiglu_case_pairing(kind, N, K):
    c = D.swiglu_case(kind, N, K)                          # (asserts row 0's gate targets and the modulo-32 up sums)
    I = N // 2
    fp8 = kind == "fp8"
    if fp8:
        scale = torch.ldexp(torch.ones((64, K), dtype=torch.float64), (c["xs"].long() - 127).repeat_interleave(32, 1))
        x, w = G.E4M3[c["xq"].long()] * scale, G.E4M3[c["Wq"].long()] * c["sw"].double()[:, None]
        assert bool((c["xs"][0] == 127).all())
    else:
        x, w = c["x"].double(), c["W"].double()
    v = (w @ x.t()).t().reshape(64, N // 32, 2, 16)        # the project's layout: g0..g15, u0..u15, g16..
    assert torch.equal(v[:, :, 0].reshape(64, I), c["gate"]) and torch.equal(v[:, :, 1].reshape(64, I), c["up"])
    assert bool((c["gate"][0].abs() <= 2).all()) and bool((c["gate"][0] == 0).any())
    win = c["up"][0, :I // 32 * 32].reshape(-1, 32)
    assert bool((win.sort(1).values.diff(dim=1) != 0).all())
    assert len({tuple(r.tolist()) for r in x}) == 64


def test_norm_case_and_candidates():
    for tiles_in in D.TILES_IN:
        n = D.norm_case(tiles_in)
        big = n["big"]
        assert big.shape == (tiles_in + 3, 64) and bool(torch.isnan(big[tiles_in:]).all())
        part = big[:tiles_in].double()
        assert torch.equal(part, part.round()) and torch.equal(part.sum(0), n["tot"]) and float(n["tot"].max()) < 2 ** 24
        assert n["norm_dim"] == 32 * tiles_in
        assert torch.allclose(n["r64"], torch.rsqrt(n["tot"] / n["norm_dim"] + 1e-6), rtol=1e-9)
    acc = torch.tensor([[3.0, -7.0, 1024.0]], dtype=torch.float64)
    r = torch.tensor([0.3], dtype=torch.float32)
    one, = D.scaled_candidates(acc, r, None)
    assert torch.equal(one, acc.float() * r)
    cands = D.scaled_candidates(acc, r, torch.tensor([0.25, -0.5, 0.75], dtype=torch.float64))
    assert len(cands) == 4 and all(t.dtype == torch.float32 for t in cands)
    assert bool(((cands[0] - cands[1]).abs() <= 2.0 ** -23 * cands[0].abs()).all())
    assert D.RS_REL_BOUND == 2 * D.RS_MEASURED_REL
    g31 = float(D.ssq_tolerance(torch.ones(1, dtype=torch.float64)))
    assert 31 * 2.0 ** -24 < g31 < 32 * 2.0 ** -24
