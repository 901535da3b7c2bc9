"""The exact-GEMV operands are what they claim to be (no GPU): for every shape of tests/test_gemv_exact_gpu.py the bound that
makes an f32 sum exact holds, the float64 reference equals an f32 evaluation in two different summation orders, the SwiGLU
layout is the project's, and the kernels' task walk - restated in gemv_exact.walk - reaches the edge each shape was chosen
for."""
import pytest
import torch

import gemv_exact as G


def _ids(shapes):
    return [f"{n}x{k}" for n, k in shapes]


# ----------------------------------------------------------------------------- exact in any order
@pytest.mark.parametrize("N,K", G.BF16_SHAPES, ids=_ids(G.BF16_SHAPES))
def test_bf16_reference_is_order_independent(N, K):
    c = G.bf16_case(N, K)                                  # (asserts the 2^24 bound and the value coverage itself)
    assert K <= G.K_MAX and K % 8 == 0
    w, x = c["W"].float(), c["x"][0].float()
    assert float(w.abs().max()) <= 8 and float(x.abs().max()) <= 8
    assert torch.equal(w, w.round()) and torch.equal(x, x.round())
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(w, x, 8, reverse), c["ref"][0]), f"f32 sum, reverse={reverse}"
    assert torch.equal(c["ref_br"][0], c["ref"][0] + c["bias"].double() + c["R"][0].double())
    assert torch.equal(c["ref_br"], c["ref_br"].float().double())


@pytest.mark.parametrize("N,K", G.FP8_SHAPES, ids=_ids(G.FP8_SHAPES))
def test_fp8_reference_is_order_independent(N, K):
    c = G.fp8_case(N, K)
    assert K <= G.K_MAX and K % 16 == 0
    x = c["x"][0].float()
    assert float(x.abs().max()) <= 4 and float(c["deq"].abs().max()) <= 8
    assert set(torch.unique(c["Wq"]).tolist()) <= set(G.FP8_CODES.tolist())
    assert torch.equal(c["deq"], c["Wq"].view(torch.float8_e4m3fn).float().double())
    sc = c["scale"].double()
    assert set(torch.log2(sc).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(c["deq"], x, 16, reverse) * sc, c["ref"][0]), f"f32 sum, reverse={reverse}"
    assert torch.equal(c["ref_br"][0], c["ref"][0] + c["bias"].double() + c["R"][0].double())


@pytest.mark.parametrize("kind,N,K", [("bf16", n, k) for n, k in G.ROWS_BF16_SHAPES] +
                         [("fp8", n, k) for n, k in G.ROWS_FP8_SHAPES])
@pytest.mark.parametrize("B", [2, 3, 4])
def test_rows_reference_is_order_independent(kind, N, K, B):
    c = G.bf16_case(N, K, B) if kind == "bf16" else G.fp8_case(N, K, B)
    w = c["W"].float() if kind == "bf16" else c["deq"]
    sc = 1.0 if kind == "bf16" else c["scale"].double()
    for b in range(B):
        for reverse in (False, True):
            assert torch.equal(G.f32_sum(w, c["x"][b].float(), 8 if kind == "bf16" else 16, reverse) * sc, c["ref"][b])
    assert len({tuple(r.tolist()) for r in c["x"]}) == B, "the input rows must differ"


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_norm_case_stages_sign_times_weight(kind):
    """norm_operands proves in float64 that bf16(x * rstd) is +-1 (it asserts); here: the reference is the plain product with
    sign * norm_w in two f32 orders, the shape takes the loop path of gv_stage_x_rmsnorm (more than 512 x-chunks), the norm
    weights use all of -8 .. 8 and |x| is one power of two."""
    N, K = G.BF16_NORM_SHAPE if kind == "bf16" else G.FP8_NORM_SHAPE
    c = G.bf16_norm_case(N, K) if kind == "bf16" else G.fp8_norm_case(N, K)
    assert K // 8 > 512 and (N, K) in (G.BF16_SHAPES if kind == "bf16" else G.FP8_SHAPES)
    x, nw = c["x"][0].double(), c["norm_w"].double()
    assert len(torch.unique(x.abs())) == 1 and float(torch.log2(x.abs()[0])) % 1 == 0
    assert set(nw.tolist()) == set(range(-8, 9)) and len(torch.unique(torch.sign(x))) == 2
    staged = torch.sign(x) * nw
    w = c["W"].float() if kind == "bf16" else G.E4M3[c["Wq"].long()]
    sc = 1.0 if kind == "bf16" else c["scale"].double()
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(w, staged, 8 if kind == "bf16" else 16, reverse) * sc, c["ref"][0])
    assert torch.equal(c["ref_br"][0], c["ref"][0] + c["bias"].double() + c["R"][0].double())


def test_one_hot_columns_are_in_range():
    N, K = G.ONE_HOT_SHAPE
    assert (N, K) in G.BF16_SHAPES and max(G.ONE_HOT_K) == K - 1 and all(0 <= k < K for k in G.ONE_HOT_K)


@pytest.mark.parametrize("K", G.PICK_K)
def test_pick_case(K):
    c = G.pick_case(K)
    assert sorted(c["perm"].tolist()) == list(range(K)) and not torch.equal(c["perm"], torch.arange(K))
    assert torch.equal(c["W"].double() @ c["x"].double(), c["x"][c["perm"]].double())
    for reverse in (False, True):
        got = G.f32_sum(c["W"][:16].float(), c["x"].float(), 8, reverse)
        assert torch.equal(got, c["x"][c["perm"][:16]].double())


# ----------------------------------------------------------------------------- SwiGLU
def test_interleave_is_the_projects():
    from vision_inspection_system_amd.weights import interleave_gate_up
    g = torch.arange(48 * 8, dtype=torch.float32).reshape(48, 8)
    u = -g - 1
    assert torch.equal(G.interleave16(g, u), interleave_gate_up(g, u))


@pytest.mark.parametrize("kind,N,K", [("bf16",) + s for s in G.BF16_SWIGLU_SHAPES] + [("fp8",) + s for s in G.FP8_SWIGLU_SHAPES])
def test_swiglu_reference(kind, N, K):
    from vision_inspection_system_amd.weights import interleave_gate_up
    c = G.swiglu_case(kind, N, K)
    I = N // 2
    w = c["W"].double() if kind == "bf16" else G.E4M3[c["Wq"].long()]
    assert torch.equal(w, interleave_gate_up(c["gate_w"], c["up_w"]))
    # the kernels' own row mapping: output `o` pairs gate row ((o >> 4) << 5) + (o & 15) with the row 16 below it
    o = torch.arange(I)
    r0 = ((o >> 4) << 5) + (o & 15)
    x = c["x"].double()
    sc = torch.ones(N, dtype=torch.float64) if kind == "bf16" else c["scale"].double()
    gate, up = (w[r0] @ x) * sc[r0], (w[r0 + 16] @ x) * sc[r0 + 16]
    assert torch.equal(gate, c["gate"]) and torch.equal(up, c["up"])
    assert set(gate.tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert torch.equal(c["ref"], torch.nn.functional.silu(gate) * up)
    chunk = 8 if kind == "bf16" else 16
    rows = torch.cat([r0[:24], r0[:24] + 16])
    for reverse in (False, True):
        assert torch.equal(G.f32_sum(w[rows], x, chunk, reverse) * sc[rows], torch.cat([gate[:24], up[:24]]))
    # a pairing that is off by one output, one 16-group, or takes the up row for the gate row is far outside the tolerance
    tol = G.swiglu_tolerance(c["ref"])
    live = gate != 0
    wrongs = [torch.roll(c["ref"], 1), torch.nn.functional.silu(up) * gate] + ([torch.roll(c["ref"], 16)] if I > 16 else [])
    for wrong in wrongs:
        assert float(((wrong - c["ref"]).abs() > 8 * tol)[live].float().mean()) > 0.9
    if kind == "fp8":
        assert G.fp8_task_shape(N, K, True) == ((2, 8) if N == 64 else (4, 4))


# ----------------------------------------------------------------------------- the edges the shapes were chosen for
def test_bf16_shapes_reach_their_edges():
    wk = {s: G.walk("bf16", *s) for s in G.BF16_SHAPES}
    assert wk[(1, 8)]["nch"] == 1 and wk[(1, 8)]["idle_waves"] == 3
    assert wk[(7, 704)]["nch"] == 88 and wk[(7, 704)]["n_units"] == 4 and wk[(7, 704)]["blocks"] == 1
    assert wk[(6, 4096)]["nseg"] == 1 and wk[(6, 4096)]["tail_chunks"] == 512            # one full segment: 8 x 64 chunks
    assert wk[(6, 4104)]["nseg"] == 2 and wk[(6, 4104)]["tail_chunks"] == 1
    assert wk[(5, 18944)]["nseg"] == 5
    assert wk[(6, 30720)]["nch"] == 15 * 256 and 30720 == G.K_MAX                       # the staging loop's last pass
    assert wk[(1001, 256)]["blocks"] == 126 and wk[(1001, 256)]["max_units"] == 1
    big = wk[(8202, 4104)]
    assert big["blocks"] == 1024 and big["max_units"] == 2 and big["nseg"] == 2 and big["crossings"] == {"BA"}
    assert wk[(16400, 64)]["max_units"] == 2 and wk[(16400, 64)]["nseg"] == 1 and wk[(16400, 64)]["crossings"] == {"AB"}
    assert wk[(24583, 64)]["max_units"] == 3 and wk[(24583, 64)]["crossings"] == {"AB", "BA"}
    for (N, K), w in wk.items():
        assert w["blocks"] <= 2048 and int(w["begin"][-1]) == w["n_units"]
    assert G.walk("bf16", 16448, 64, swiglu=True)["max_units"] >= 2
    assert G.walk("bf16", 32, 64, swiglu=True)["n_units"] == 16


def test_fp8_shapes_reach_both_task_shapes_and_their_edges():
    for s in G.FP8_SHAPES_2x8:
        assert G.fp8_task_shape(*s) == (2, 8), s
    for s in G.FP8_SHAPES_4x4:
        assert G.fp8_task_shape(*s) == (4, 4), s
    wk = {s: G.walk("fp8", *s) for s in G.FP8_SHAPES}
    assert wk[(1, 16)]["nch"] == 1
    assert wk[(7, 1424)]["nch"] == 89
    assert wk[(6, 8192)]["nseg"] == 1 and wk[(6, 8192)]["tail_chunks"] == 512
    assert wk[(6, 8208)]["nseg"] == 2 and wk[(6, 8208)]["tail_chunks"] == 1
    assert wk[(5, 18944)]["nseg"] == 3 and wk[(6, 30720)]["nseg"] == 4
    assert 8197 % 4 == 1 and wk[(8197, 64)]["n_units"] == 2050
    assert 8198 % 4 == 2 and wk[(8198, 4112)]["nseg"] == 2 and wk[(8198, 4112)]["tail_chunks"] == 1
    assert wk[(16402, 128)]["max_units"] == 2 and wk[(16402, 128)]["crossings"] == {"AB"}
    assert wk[(40962, 64)]["max_units"] == 3 and wk[(40962, 64)]["crossings"] == {"AB", "BA"}
    for s in G.ROWS_FP8_SHAPES:
        assert s in G.FP8_SHAPES
    for s in G.ROWS_BF16_SHAPES:
        assert s in G.BF16_SHAPES


@pytest.mark.parametrize("N,K", G.ARGMAX_SHAPES)
def test_argmax_ties_sit_where_the_labels_say(N, K):
    c = G.argmax_case(N, K)
    ties, labels, wk = c["ties"], c["labels"], c["walk"]
    assert int(torch.argmax(c["logits"])) == ties[0]
    assert torch.nonzero(c["logits"] == c["logits"].max()).flatten().tolist() == ties and len(ties) >= 3
    where = [(r // 2, G.unit_wave(wk, r // 2)) for r in ties]          # (pair, wave); workgroup = wave // 4
    for j in range(1, len(ties)):
        (p0, w0), (p1, w1) = where[j - 1], where[j]
        if labels[j] == "two rows of one pair":
            assert p0 == p1
        elif labels[j] == "two pairs of one wave":
            assert p0 != p1 and w0 == w1
        elif labels[j] == "two waves of one workgroup":
            assert w0 != w1 and w0 // 4 == w1 // 4
        else:
            assert w0 // 4 != w1 // 4
    need = {"two rows of one pair", "two waves of one workgroup", "two workgroups", "last row of an odd N"}
    if wk["max_units"] >= 2:
        need.add("two pairs of one wave")
    assert need <= set(labels)
    assert ties[-1] == N - 1 and N % 2 == 1
    if wk["blocks"] > 512:       # two tied workgroups 256 apart: the same thread of the merging launch
        blocks = [w // 4 for _, w in where]
        assert any(b - a == 256 for a in blocks for b in blocks)
    m = G.allow_mask(N, ties[:2])
    bits = [(int(m[i // 64]) >> (i % 64)) & 1 for i in range(N)]
    assert [i for i in range(N) if not bits[i]] == ties[:2] and m.numel() == (N + 63) // 64
    assert all(((int(m[-1]) >> b) & 1) == 0 for b in range(N % 64, 64))


def test_e4m3_code_set():
    vals = sorted(set(G.E4M3[G.FP8_CODES.long()].abs().tolist()))
    assert vals == [i / 4 for i in range(0, 17)] + [4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0]
    assert len(G.E4M3_FINITE) == 254 and bool(torch.isfinite(G.E4M3[G.E4M3_FINITE]).all())
    assert bool(torch.isnan(G.E4M3[[0x7F, 0xFF]]).all())
