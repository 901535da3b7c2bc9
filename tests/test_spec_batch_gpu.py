"""Speculative decoding of a batch on the GPU.  The kernels of csrc/spec.hip's batch forms against their definitions -
vis_decode_attn_draft_batch against R successive batched vis_decode_attn launches (torch.equal, outputs and caches),
vis_spec_accept_batch against the single-sequence entries and spec.accept_ref / accept_ref_sampled, vis_spec_draft_batch against
spec.propose - and an engine built with ``batch_speculative`` against one without: the same replies, token for token, with the
counters a model-free walk of the drafter over the plain replies predicts; a batch that cannot speculate runs the plain step."""
import numpy as np
import pytest
import torch

import spec_batch_cases as C

pytestmark = pytest.mark.gpu

POISON = 0x7F7F


# ------------------------------------------------------------------------------------------ vis_decode_attn_draft_batch
def _attn_case(device, Hq, Hkv, T, B, R, seed, guard=4096):
    """Random rows, tables and caches of B sequences (what lies behind a sequence's step is garbage like the rest); the
    caches sit inside poisoned buffers."""
    g = torch.Generator().manual_seed(seed)
    nq = (Hq + 2 * Hkv) * 128
    qkv = torch.randn((B * R, nq), generator=g).to(torch.bfloat16).to(device)
    ang = torch.rand((B, T, 128), generator=g) * 6.283
    cos, sin = torch.cos(ang).to(device), torch.sin(ang).to(device)
    n = B * Hkv * T * 128
    buf = torch.full((2, n + 2 * guard), POISON, dtype=torch.int16, device=device).view(torch.bfloat16)
    kc, vc = (buf[i, guard:guard + n].view(B, Hkv, T, 128) for i in range(2))
    kc.copy_(torch.randn((B, Hkv, T, 128), generator=g).to(torch.bfloat16))
    vc.copy_(torch.randn((B, Hkv, T, 128), generator=g).to(torch.bfloat16))
    return qkv, cos, sin, kc, vc, buf, guard, n


def _successive_batch(hip, qkv, cos, sin, kc, vc, steps, R, Hq, Hkv, nsplit):
    """The reference: R plain batched launches at advancing steps on copies of the caches.  A sequence whose row lies past the
    cache is not part of that launch's result: its caches are put back and its output row keeps the poison."""
    B, T, dev = kc.shape[0], kc.shape[2], kc.device
    kw, vw = kc.clone(), vc.clone()
    want = torch.full((B * R, Hq * 128), POISON, dtype=torch.int16, device=dev).view(torch.bfloat16)
    po = torch.zeros(B * Hq * nsplit * 128, dtype=torch.float32, device=dev)
    pm = torch.zeros(B * Hq * nsplit * 2, dtype=torch.float32, device=dev)
    rows = qkv.view(B, R, -1)
    for r in range(R):
        st = torch.tensor([s + r for s in steps], dtype=torch.int32, device=dev)
        out = torch.zeros((B, Hq * 128), dtype=torch.bfloat16, device=dev)
        k0, v0 = kw.clone(), vw.clone()
        hip.decode_attn(rows[:, r], cos, sin, kw, vw, st, po, pm, out, Hq, Hkv, 128, nsplit, 128 ** -0.5)
        for b, s in enumerate(steps):
            if s + r < T:
                want[b * R + r] = out[b]
            else:
                kw[b], vw[b] = k0[b], v0[b]
    return want, kw, vw


STEPS = {2: [254, 62], 3: [0, 62, 126], 5: [0, 62, 126, 253, 17]}      # 62: rows straddle a split boundary; 253, 254: rows past the cache


@pytest.mark.parametrize("heads", [(2, 1), (28, 4)])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_decode_attn_draft_batch_equals_successive_batched_launches(device, heads, B, R):
    from vision_inspection_system_amd import hip
    Hq, Hkv = heads
    T, steps = 256, STEPS[B]
    assert hip.DECODE_KEYS_PER_SPLIT == 64 and not hip.decode_attn_streams(Hkv, B)
    nsplit = T // hip.DECODE_KEYS_PER_SPLIT
    qkv, cos, sin, kc, vc, buf, guard, n = _attn_case(device, Hq, Hkv, T, B, R, 1000 * B + R)
    want, kw, vw = _successive_batch(hip, qkv, cos, sin, kc, vc, steps, R, Hq, Hkv, nsplit)
    before = buf.clone()
    st = torch.tensor(steps, dtype=torch.int32, device=device)
    out = torch.full((B * R, Hq * 128), POISON, dtype=torch.int16, device=device).view(torch.bfloat16)
    po = torch.zeros(B * R * Hq * nsplit * 128, dtype=torch.float32, device=device)
    pm = torch.zeros(B * R * Hq * nsplit * 2, dtype=torch.float32, device=device)
    hip.decode_attn_draft_batch(qkv, cos, sin, kc, vc, st, po, pm, out, Hq, Hkv, 128, nsplit, 128 ** -0.5)
    assert st.cpu().tolist() == steps
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))      # rows past the cache: the poison on both sides
    assert torch.equal(kc, kw) and torch.equal(vc, vw)
    past = [(b, r) for b, s in enumerate(steps) for r in range(R) if s + r >= T]
    assert bool(past) == ((B == 2 and R > 2) or (B == 5 and R > 3))
    a, b0 = buf.view(torch.int16), before.view(torch.int16)
    assert torch.equal(a[:, :guard], b0[:, :guard]) and torch.equal(a[:, guard + n:], b0[:, guard + n:])


@pytest.mark.parametrize("how", ["head count", "environment"])
def test_decode_attn_draft_batch_refuses_where_the_plain_step_streams(device, how, monkeypatch):
    """Hkv * B >= 128 (4 kv heads, 32 sequences), or the tiny head count with the streaming form forced: UNSUPPORTED, nothing
    launched - caches, output and workspace untouched."""
    from vision_inspection_system_amd import hip
    Hq, Hkv, B = (28, 4, 32) if how == "head count" else (2, 1, 2)
    if how == "environment":
        assert not hip.decode_attn_streams(Hkv, B)
        monkeypatch.setenv("VIS_DECODE_ATTN_STREAM", "2")
    else:
        assert not hip.decode_attn_streams(Hkv, B - 1)
    assert hip.decode_attn_streams(Hkv, B)
    T, R = 128, 2
    qkv, cos, sin, kc, vc, buf, guard, n = _attn_case(device, Hq, Hkv, T, B, R, 5)
    before = buf.clone()
    st = torch.full((B,), 70, dtype=torch.int32, device=device)
    out = torch.full((B * R, Hq * 128), POISON, dtype=torch.int16, device=device).view(torch.bfloat16)
    po = torch.zeros(B * R * Hq * 2 * 128, dtype=torch.float32, device=device)
    pm = torch.zeros(B * R * Hq * 2 * 2, dtype=torch.float32, device=device)
    with pytest.raises(hip.AttnStreams):
        hip.decode_attn_draft_batch(qkv, cos, sin, kc, vc, st, po, pm, out, Hq, Hkv, 128, 2, 128 ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))
    assert bool((out.view(torch.int16) == POISON).all()) and not bool(po.any()) and not bool(pm.any())


def test_batch_entries_refuse_bad_arguments(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    P, big = 4096, 4 * 256 * 128
    attn = lambda rows, batch, ld=4608, cbs=big: lib.vis_decode_attn_draft_batch(      # noqa: E731
        P, P, P, P, P, P, P, P, P, 28, 4, 128, 256, 4, 0.1, rows, batch, ld, cbs, 256 * 128, None)
    assert attn(5, 2) == 1 and attn(4, 17) == 1 and attn(2, 0) == 1      # rows, batch * rows > 64, batch
    assert attn(2, 2, ld=4600) == 1 and attn(2, 2, cbs=big - 8) == 1     # row stride, caches that overlap
    assert attn(2, 32) == 3                                              # the plain step would stream: before any launch
    assert lib.vis_spec_accept_batch(P, 1000, 1000, 4, 17, P, P, P, P, P, P, 64, P, P, P, None, None) == 1
    assert lib.vis_spec_accept_batch(P, 1000, 999, 2, 2, P, P, P, P, P, P, 64, P, P, P, None, None) == 1
    assert lib.vis_spec_draft_batch(P, 8, P, P, 64, P, P, 4, 4, 2, 512, 2, P, P, None) == 1
    assert lib.vis_spec_draft_batch(P, 8, P, P, 64, P, P, 3, 4, 2, 512, 65, P, P, None) == 1
    assert lib.vis_spec_gather_batch(P, P, P, P, 2, 2, 100, 512, None) == 1      # D % 8


# ------------------------------------------------------------------------------------------------ vis_spec_accept_batch
V_ACC, T_ROW = 1000, 64


def _dev(device, a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=device)


def _accept_plans(picks):
    """Per sequence (draft, n_draft, step, limit) from its rows' picks: right, first wrong, partly right, the limit inside
    the run, a step behind the limit, a draft count too long, none."""
    w = lambda b, i: (picks[b][i] + 1) % V_ACC      # noqa: E731
    return [(picks[0][:3], 3, 10, 60), ([w(1, 0), picks[1][1], picks[1][2]], 3, 4, 60),
            ([picks[2][0], picks[2][1], w(2, 2)], 3, 20, 60), (picks[3][:3], 3, 30, 31), (picks[4][:3], 3, 12, 11),
            (picks[5][:3], 9, 0, 60), (picks[6][:3], 0, 7, 60)]


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("sampled", [False, True])
def test_spec_accept_batch_equals_the_single_entry_and_the_reference(device, R, sampled):
    from vision_inspection_system_amd import hip, spec
    B = 7
    rng = np.random.default_rng(10 * R + sampled)
    logits = rng.standard_normal((B * R, V_ACC)).astype(np.float32)
    lg = torch.from_numpy(logits).to(device)
    temps = 0.7
    seeds = [11 + 1000003 * b for b in range(B)]
    steps0 = [10, 4, 20, 30, 12, 0, 7]
    # every row's pick from the plain pick launch on that row alone, at its hash counter step + r and its sequence's seed
    picks = []
    for b in range(B):
        row = []
        for r in range(R):
            tok, cur, st = _dev(device, [0] * T_ROW), _dev(device, [-1]), _dev(device, [steps0[b] + r])
            hip.argmax(lg[b * R + r], torch.empty(256, device=device), torch.empty(256, dtype=torch.int32, device=device), tok, cur,
                       st, temps if sampled else 0.0, seeds[b])
            row.append(int(cur.item()))
        picks.append(row + [0] * (3 - len(row)))
    plans = _accept_plans(picks)
    tokens0 = np.arange(1000, 1000 + B * T_ROW, dtype=np.int32).reshape(B, T_ROW)
    cnt0 = [[5 + b, 7, 3] for b in range(B)]
    par = np.zeros((B, 2), dtype=np.uint32)
    par[:, 0], par[:, 1] = np.float32(1.0 / temps).view(np.uint32), seeds
    params = torch.from_numpy(par.view(np.int32)).to(device) if sampled else None
    draft = _dev(device, [list(p[0]) for p in plans])
    nd, lim, st = (_dev(device, [p[i] for p in plans]) for i in (1, 3, 2))
    tok, cur, cnt = _dev(device, tokens0), _dev(device, [-1] * B), _dev(device, cnt0)
    hip.spec_accept_batch(lg, draft, nd, lim, torch.empty(256 * B * R, device=device),
                          torch.empty(256 * B * R, dtype=torch.int32, device=device), tok, cur, st, cnt, params)
    got = (tok.cpu().numpy(), cur.cpu().tolist(), st.cpu().tolist(), cnt.cpu().tolist())
    moved = 0
    for b, (dr, d, s, limit) in enumerate(plans):
        # the single-sequence entry on b's rows and state alone
        t1, c1, s1, n1 = _dev(device, tokens0[b]), _dev(device, [-1]), _dev(device, [s]), _dev(device, cnt0[b])
        args = (lg[b * R:(b + 1) * R], _dev(device, dr), _dev(device, [d]), _dev(device, [limit]),
                torch.empty(256 * R, device=device), torch.empty(256 * R, dtype=torch.int32, device=device), t1, c1, s1, n1)
        if sampled:
            hip.spec_accept_sampled(*args, params[b])
        else:
            hip.spec_accept(*args)
        one = (t1.cpu().numpy(), int(c1.item()), int(s1.item()), n1.cpu().tolist())
        assert np.array_equal(got[0][b], one[0]) and (got[1][b], got[2][b], got[3][b]) == one[1:], (b, R, sampled)
        if sampled:
            want = spec.accept_ref_sampled(picks[b][:R], dr, d, s, limit, tokens0[b], cnt0[b])
        else:
            want = spec.accept_ref(logits[b * R:(b + 1) * R], dr, d, s, limit, tokens0[b], cnt0[b])
        assert np.array_equal(got[0][b], want[0])
        assert (got[1][b], got[2][b], got[3][b]) == (-1 if want[1] is None else want[1], want[2], want[3])
        moved += got[2][b] - s
    if R == 4:      # 4 + 1 + 3 + 2 + 0 + 4 + 1: every kind of run happened
        assert moved == 15
    if sampled and R == 4:
        greedy = [int(np.argmax(logits[b * R])) for b in range(B)]
        assert [p[0] for p in picks] != greedy      # the sampled picks are not the greedy ones: the seeds and 1 / T were read


# ------------------------------------------------------------------------------------------------- vis_spec_draft_batch
def test_spec_draft_batch_equals_propose_per_sequence(device):
    from vision_inspection_system_amd import hip, spec
    rng = np.random.default_rng(3)
    hists = [[5, 6, 7, 8, 9, 5, 6, 7],                  # a match with ids behind it
             [1, 2, 3, 4, 5, 6, 7, 8, 9],               # no match
             [9, 1, 2, 1, 2],                           # the match ends at the history's end: two ids where k asks for three
             rng.integers(0, 4, 200).tolist(), rng.integers(0, 3, 77).tolist(), [3]]
    B, P, T, gen0 = len(hists), 256, 300, 3
    for k, hi, lo in ((3, 4, 2), (1, 3, 1), (2, 8, 3)):
        prompt, plen, rows, steps = np.full((B, P), -3, np.int32), [], np.full((B, T), -9, np.int32), []
        for b, h in enumerate(hists):
            split = (len(h) * (b + 1)) // (B + 1) if len(h) > 1 else 1      # where the prompt ends and the reply starts
            prompt[b, :split] = h[:split]
            rows[b, gen0 + b:gen0 + b + len(h) - split] = h[split:]
            plen.append(split)
            steps.append(gen0 + b + len(h) - split)
        draft, nd = _dev(device, [[-1, -1, -1]] * B), _dev(device, [-5] * B)
        hip.spec_draft_batch(_dev(device, prompt), _dev(device, plen), _dev(device, rows), _dev(device, [gen0 + b for b in range(B)]),
                             _dev(device, steps), k, hi, lo, 1 << 20, draft, nd)
        got, n = draft.cpu().tolist(), nd.cpu().tolist()
        want = [spec.propose(h, k, hi, lo) for h in hists]
        assert [g[:d] for g, d in zip(got, n)] == want, (k, hi, lo)
        assert all(g[d:] == [-1] * (3 - d) for g, d in zip(got, n))      # nothing past the count is written
        if (k, hi, lo) == (3, 4, 2):
            assert want[0] == [8, 9, 5] and want[1] == [] and want[2] == [1, 2] and want[5] == []


# --------------------------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def weights(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    return cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)


@pytest.fixture(scope="module", params=["bf16", "fp8"])
def engines(request, weights, device):
    """(plain engine, {k: engine with batch_speculative}) of one weight format, 64 slots."""
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, w = weights
    mk = lambda **kw: Qwen2VLEngine(cfg, w, device, max_ctx=128, max_batch=64, decode_weights=request.param, **kw)      # noqa: E731
    return mk(), {1: mk(batch_speculative=1), 3: mk(batch_speculative={"num_speculative_tokens": 3, "sampled": True})}


ACCEPTED = {}      # id(plain engine of a format) -> accepted drafts of every batch size's greedy runs


def _reqs(B):
    return [(ids, []) for ids in C.prompts(B)]


@pytest.mark.parametrize("B", [2, 3, 5, 16])
def test_generate_batch_speculative_equals_plain(engines, B):
    """Greedy: the plain replies, token for token and with the same finish reasons - run to the full length and with EOS
    handling, eager and replayed, k = 1 and k = 3 (16 sequences at k = 3: 64 rows) - and per sequence the counters of a
    model-free walk of the drafter over its plain reply."""
    from vision_inspection_system_amd import spec_batch
    plain_eng, spec_engs = engines
    reqs = _reqs(B)
    plain = {ig: plain_eng.generate_batch(reqs, max_new_tokens=C.N_NEW, ignore_eos=ig) for ig in (True, False)}
    fin = plain_eng.last_finish
    assert "spec_steps" not in plain_eng.last_timing
    accepted = 0
    for k, eng in spec_engs.items():
        for graph in ((True, False) if B != 16 else (True,)):
            got = eng.generate_batch(reqs, max_new_tokens=C.N_NEW, ignore_eos=True, use_graph=graph, check_every=4)
            assert got == plain[True], (k, graph)
            t = eng.last_timing
            walks = [spec_batch.simulate(plain[True][b], reqs[b][0], k, vocab=eng.cfg.vocab) for b in range(B)]
            assert [w["reply"] for w in walks] == plain[True]
            assert t["spec_sequences"] == [[w["spec_steps"], w["spec_proposed"], w["spec_accepted"]] for w in walks], (k, graph)
            assert (t["spec_steps"], t["spec_proposed"], t["spec_accepted"]) == tuple(
                sum(w[n] for w in walks) for n in ("spec_steps", "spec_proposed", "spec_accepted"))
            assert t["sequences"] == B and max(w["spec_steps"] for w in walks) <= t["decode_steps"] < C.N_NEW + 4
            accepted += t["spec_accepted"]
        got = eng.generate_batch(reqs, max_new_tokens=C.N_NEW, ignore_eos=False)
        assert got == plain[False] and eng.last_finish == fin, k
        assert "spec_steps" in eng.last_timing
    ACCEPTED.setdefault(id(plain_eng), []).append(accepted)


def test_some_batch_accepted_drafts(engines):
    """The comparison above is not vacuous: over the batch sizes of this weight format drafts were accepted (seeded noise for
    weights follows a prompt's repetition only now and then; a single batch may accept none)."""
    got = ACCEPTED.get(id(engines[0]), [])
    assert len(got) == 4 and sum(got) > 0, got


@pytest.mark.parametrize("B", [2, 5])
def test_generate_batch_speculative_sampled_equals_plain_sampled(engines, B):
    """T = 0.7 with one seed per request, on the engine whose configuration says ``sampled``: the plain sampled replies."""
    plain_eng, spec_engs = engines
    reqs, seeds = _reqs(B), [7 + 13 * b for b in range(B)]
    kw = dict(max_new_tokens=C.N_NEW, ignore_eos=True, temperature=0.7, seeds=seeds)
    plain = plain_eng.generate_batch(reqs, **kw)
    assert plain != plain_eng.generate_batch(reqs, max_new_tokens=C.N_NEW, ignore_eos=True)      # it does sample
    for graph in (True, False):
        assert spec_engs[3].generate_batch(reqs, use_graph=graph, **kw) == plain
        assert spec_engs[3].last_timing["spec_steps"] >= B
    # without seeds: the slot-derived seeds of the plain pick
    kw.pop("seeds")
    assert spec_engs[3].generate_batch(reqs, seed=5, **kw) == plain_eng.generate_batch(reqs, seed=5, **kw)
    assert "spec_steps" in spec_engs[3].last_timing


def test_batches_that_cannot_speculate_run_the_plain_step(engines):
    """17 sequences at k = 3 (68 rows), a group with top_p, a temperature without ``sampled``, a failed lazy request: the plain
    reply and no spec_* keys.  And the setting leaves a single request alone."""
    plain_eng, spec_engs = engines

    def boom():
        raise RuntimeError("no image")

    reqs = _reqs(3)
    cases = [(spec_engs[3], _reqs(17), {}), (spec_engs[3], reqs, dict(top_p=0.9, temperature=0.7, seeds=[1, 2, 3])),
             (spec_engs[1], reqs, dict(temperature=0.7)), (spec_engs[3], [reqs[0], boom, reqs[2]], {})]
    for eng, rq, kw in cases:
        got = eng.generate_batch(rq, max_new_tokens=8, ignore_eos=True, **kw)
        want = plain_eng.generate_batch(rq, max_new_tokens=8, ignore_eos=True, **kw)
        assert not any(k.startswith("spec_") for k in eng.last_timing), kw
        assert [g if not isinstance(g, Exception) else str(g) for g in got] == \
            [w if not isinstance(w, Exception) else str(w) for w in want]
    assert isinstance(got[1], RuntimeError)
    assert spec_engs[3].generate_batch(_reqs(16), max_new_tokens=4, ignore_eos=True) == \
        plain_eng.generate_batch(_reqs(16), max_new_tokens=4, ignore_eos=True)
    assert "spec_steps" in spec_engs[3].last_timing      # 16 x 4 = 64 rows still speculate
    one = spec_engs[3].generate_batch(reqs[:1], max_new_tokens=8, ignore_eos=True)
    assert one == plain_eng.generate_batch(reqs[:1], max_new_tokens=8, ignore_eos=True)
    assert "spec_steps" not in spec_engs[3].last_timing
