"""Predicted outputs on the GPU: vis_spec_draft_pred against its definition spec.propose_pred (every draft and every state
int, over chains of launches), vis_spec_draft unchanged by the refactor it shares its lookup with, and the engine and the
client with a prediction against the plain request - the same reply, and the step and acceptance counters that
spec.simulate_prediction derives from the plain reply alone."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 7777          # stands behind the valid prediction ids and behind the draft row: never proposed, never overwritten
LD = 384               # the bare kernel's prediction buffer
N_NEW = 24


# ------------------------------------------------------------------------------------------- kernel against propose_pred
class _Dev:
    """The device side of one chain: [step, gen0, prompt_len, pred_len] / the token row / prompt / prediction (+ guard) /
    [7 state ints, n_draft, 3 draft ids, guard]."""

    def __init__(self, device, prompt, pred, pred_len_dev):
        i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=device)      # noqa: E731
        self.gen0 = 3
        self.ints = i32([self.gen0, self.gen0, len(prompt), pred_len_dev])
        self.tokens = i32([-7] * 160)
        self.prompt = i32(list(prompt) + [-3, -3])
        self.pred_buf = i32(list(pred) + [POISON] * (LD + 64 - len(pred)))
        self.out = i32([0] * 7 + [-5] + [-1] * 3 + [POISON] * 16)

    def launch(self, hip, reply, k, hi, lo, vocab):
        n = len(reply)
        self.tokens[self.gen0:self.gen0 + n].copy_(torch.tensor(reply, dtype=torch.int32))
        self.ints[0:1].fill_(self.gen0 + n)
        o = self.out
        hip.spec_draft_pred(self.prompt, self.ints[2:3], self.tokens, self.ints[1:2], self.ints[0:1], k, hi, lo, vocab,
                            self.pred_buf[:LD], self.ints[3:4], o[0:7], o[8:8 + k], o[7:8])
        got = o.cpu().tolist()
        assert got[11:] == [POISON] * 16                           # nothing behind the draft row moved
        return got[0:7], got[7], got[8:11]


@pytest.mark.parametrize("P", [1, 2, 3, 64, 257, LD])
def test_kernel_equals_propose_pred_over_chains(device, P):
    from vision_inspection_system_amd import hip
    from vision_inspection_system_amd.spec import PredState, propose_pred
    rng = np.random.default_rng(1000 + P)
    vocab = 1 << 20
    held = lost = 0
    for chain in range(12):
        k = chain % 3 + 1
        hi = int(rng.integers(1, 9))
        lo = int(rng.integers(1, hi + 1))
        pred = rng.integers(0, 5, P).tolist()
        prompt = rng.integers(0, 5, int(rng.integers(1, 40))).tolist()
        # P == LD: the device length says more than the buffer holds and is clamped to it
        dev = _Dev(device, prompt, pred, P + 50 if P == LD else P)
        state, shown = PredState(), [-1, -1, -1]
        reply = [pred[0] if chain % 2 == 0 else int(rng.integers(0, 5))]
        for _ in range(12 + chain % 3):
            draft, state = propose_pred(state, prompt, reply, pred, k, hi, lo, vocab)
            got_state, got_n, got_draft = dev.launch(hip, reply, k, hi, lo, vocab)
            shown[:len(draft)] = draft                             # ids past the count stay what they were
            ctx = (P, chain, k, hi, lo, len(reply))
            assert got_n == len(draft) and got_draft == shown, ctx
            assert got_state == list(state), ctx
            assert POISON not in got_draft
            held += state.src == 2
            lost += state.cursor < 0
            # the accept step's part, on the host: some of the outstanding drafts, then the step's own token
            d = len(draft)
            if rng.random() < 0.6:
                nxt = state.cursor + d
                own = pred[nxt] if state.src == 2 and nxt < P and rng.random() < 0.8 else int(rng.integers(0, 5))
                reply = reply + draft + [own]
            else:
                a = int(rng.integers(0, d + 1))
                own = int(rng.integers(0, 5))
                if a < d and own == draft[a]:
                    own = (own + 1) % 5                            # the id that refused draft a
                reply = reply + draft[:a] + [own]
    if P >= 3:
        assert held > 20 and lost > 5                              # both paths were walked


def test_kernel_entry_refuses_bad_arguments(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    A = 4096
    ok = [A, 8, A, A, 64, A, A, 3, 4, 2, 512, A, 16, A, A, A, A, None]
    for pos, bad in ((7, 4), (8, 9), (9, 5), (12, 0), (11, None), (14, None), (14, A + 2), (10, 0)):
        args = list(ok)
        args[pos] = bad
        assert lib.vis_spec_draft_pred(*args) == 1, pos


# ----------------------------------------------------------------------------------------------- vis_spec_draft unchanged
def test_spec_draft_still_equals_propose(device):
    """The lookup moved into a function both drafters call: vis_spec_draft's drafts and count on 50 seeded histories are
    those of spec.propose, its pinned definition, and nothing past the count is written."""
    from vision_inspection_system_amd import hip, spec
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=device)      # noqa: E731
    rng = np.random.default_rng(77)
    matched = 0
    for i in range(50):
        L = int(rng.integers(1, 301)) if i else 300
        hist = rng.integers(0, 4, L).tolist()
        split = int(rng.integers(1, L + 1))
        k, hi = int(rng.integers(1, 4)), int(rng.integers(1, 9))
        lo = int(rng.integers(1, hi + 1))
        prompt, gen = hist[:split], hist[split:]
        out = i32([-5, -1, -1, -1, POISON])
        hip.spec_draft(i32(prompt + [-3] * 2), i32([len(prompt)]), i32([-7] * 3 + gen + [-9] * 5), i32([3]), i32([3 + len(gen)]),
                       k, hi, lo, 1 << 20, out[1:4], out[0:1])
        want = spec.propose(hist, k, hi, lo)
        matched += bool(want)
        assert out.cpu().tolist() == [len(want)] + want + [-1] * (3 - len(want)) + [POISON], (hist, split, k, hi, lo)
    assert matched > 25


# --------------------------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def model(device):
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.weights import pack_device_weights, synth_state_dict
    cfg = Qwen2VLConfig.tiny()
    return cfg, pack_device_weights(cfg, synth_state_dict(cfg, seed=0), device)


def _engine(model, device, fmt):
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    cfg, w = model
    return Qwen2VLEngine(cfg, w, device, max_ctx=256, decode_weights=fmt)


@pytest.fixture(scope="module", params=["bf16", "fp8", "mxfp4"])
def eng(request, model, device):
    return _engine(model, device, request.param)


IDS = [256] + np.random.default_rng(11).integers(1, 490, 41).tolist()


def _predictions(plain):
    rng = np.random.default_rng(5)
    mid = len(plain) // 2
    return {
        "plain": list(plain),
        "one id replaced": plain[:mid] + [(plain[mid] + 1) % 490] + plain[mid + 1:],
        "segment removed": plain[:8] + plain[13:],
        "segment duplicated": plain[:13] + plain[8:13] + plain[13:],
        "unrelated": rng.integers(1, 490, 30).tolist(),
        "one id": plain[:1],
        "longer than max_new_tokens": list(plain) + rng.integers(1, 490, 40).tolist(),
    }


COUNTERS = ("spec_steps", "spec_proposed", "spec_accepted", "pred_accepted", "pred_rejected")


def test_engine_prediction_equals_plain_and_counts_as_simulated(eng):
    from vision_inspection_system_amd.spec import simulate_prediction
    plain = eng.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True)
    assert len(plain) == N_NEW
    plain_steps = eng.last_timing["decode_steps"]
    fin = eng.last_finish
    for name, p in _predictions(plain).items():
        want = simulate_prediction(plain, IDS, p, 3, 4, 2, N_NEW, vocab=eng.cfg.vocab)
        assert want["reply"] == plain
        for graph in (False, True):
            got = eng.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, use_graph=graph, prediction=p)
            t = eng.last_timing
            print(name, "graph" if graph else "eager", {c: t[c] for c in COUNTERS})
            assert got == plain, (name, graph)
            assert eng.last_finish == fin
            assert {c: t[c] for c in COUNTERS} == {c: want[c] for c in COUNTERS}, (name, graph)
        if name == "plain":      # the test that fails without the feature: a prediction that holds saves weight passes
            assert t["spec_steps"] == -(-(N_NEW - 1) // 4) < plain_steps
            assert t["pred_accepted"] == N_NEW - 1 - t["spec_steps"]
    # speculative= next to the prediction sets k and the window
    p = _predictions(plain)["one id replaced"]
    sp = {"method": "ngram", "num_speculative_tokens": 1, "prompt_lookup_max": 3, "prompt_lookup_min": 1}
    want = simulate_prediction(plain, IDS, p, 1, 3, 1, N_NEW, vocab=eng.cfg.vocab)
    assert eng.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, prediction=p, speculative=sp) == plain
    assert {c: eng.last_timing[c] for c in COUNTERS} == {c: want[c] for c in COUNTERS}
    # an empty prediction is no prediction, and nothing is left behind
    assert eng.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, prediction=[]) == plain
    assert "spec_steps" not in eng.last_timing and "pred_accepted" not in eng.last_timing
    assert eng.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, speculative=3) == plain
    assert "spec_steps" in eng.last_timing and "pred_accepted" not in eng.last_timing


def test_two_predictions_share_one_captured_graph(model, device):
    from vision_inspection_system_amd.spec import simulate_prediction
    e = _engine(model, device, "bf16")
    plain = e.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True)
    ps = _predictions(plain)
    first, second = ps["longer than max_new_tokens"], ps["segment removed"]
    assert len(first) != len(second)
    assert e.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, prediction=first) == plain
    graphs = dict(e._spec_graphs)
    assert len(graphs) == 1 and list(graphs)[0][-1] == "pred"
    assert e.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, prediction=second) == plain
    after = {c: e.last_timing[c] for c in COUNTERS}
    assert len(e._spec_graphs) == 1 and list(e._spec_graphs.values())[0] is list(graphs.values())[0]
    fresh = _engine(model, device, "bf16")
    assert fresh.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, prediction=second) == plain
    assert {c: fresh.last_timing[c] for c in COUNTERS} == after
    want = simulate_prediction(plain, IDS, second, 3, 4, 2, N_NEW, vocab=e.cfg.vocab)
    assert after == {c: want[c] for c in COUNTERS}
    # a speculative request without a prediction keeps its own graph key, the one of before
    assert e.generate(IDS, [], max_new_tokens=N_NEW, ignore_eos=True, speculative=3) == plain
    assert ("spec", 4, "bf16", 4, 2) in e._spec_graphs and len(e._spec_graphs) == 2


# --------------------------------------------------------------------------------------------------------------- client
def test_client_create_with_prediction(device):
    from vision_inspection_system_amd.client import LocalVLMClient, get_model
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": "list: alpha beta gamma; list: alpha beta gamma; list: alpha beta"}]
    plain = c.chat.completions.create(model="synthetic:tiny", messages=msgs, max_tokens=20)
    assert "completion_tokens_details" not in plain.usage
    text = plain.choices[0].message.content
    assert len(text) > 3
    for prediction in ({"type": "content", "content": text},
                       {"type": "content", "content": [{"type": "text", "text": text[:3]}, {"type": "text", "text": text[3:]}]}):
        got = c.chat.completions.create(model="synthetic:tiny", messages=msgs, max_tokens=20, prediction=prediction)
        assert got.choices[0].message.content == text
        assert got.choices[0].finish_reason == plain.choices[0].finish_reason
        t = get_model("synthetic:tiny").engine.last_timing
        assert got.usage["completion_tokens_details"] == {"accepted_prediction_tokens": t["pred_accepted"],
                                                          "rejected_prediction_tokens": t["pred_rejected"]}
        assert {k: v for k, v in got.usage.items() if k != "completion_tokens_details"} == plain.usage
    empty = c.chat.completions.create(model="synthetic:tiny", messages=msgs, max_tokens=20,
                                      prediction={"type": "content", "content": ""})
    assert empty.usage == plain.usage and empty.choices[0].message.content == text
    sp = c.chat.completions.create(model="synthetic:tiny", messages=msgs, max_tokens=20,
                                   speculative={"method": "ngram", "num_speculative_tokens": 3})
    assert sp.usage == plain.usage
    with pytest.raises(ValueError, match="Qwen2-VL"):
        c.chat.completions.create(model="synthetic:mllama-tiny", messages=msgs, max_tokens=4,
                                  prediction={"type": "content", "content": "x"})


# ------------------------------------------------------------------------------------------------------------ off state
def _step_names(device, prediction):
    """The library entries one eager speculative step calls, in order (the recorder of the decode transcript)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_decode_transcript as T
    from vision_inspection_system_amd.spec import SpecConfig
    with T.recording() as rec:
        _, e = T._qwen(device)
        e.prefill(IDS, [], max_new_tokens=N_NEW + 4)
        e._spec_begin(SpecConfig(3, 4, 2), N_NEW, prediction)
        with rec.armed(e):
            e._decode_step_spec(4)
        torch.cuda.synchronize(device)
        return [c.split("(")[0] for c in rec.calls], len(e.dec_layers)


def test_speculative_step_without_prediction_is_the_step_of_before(device):
    names, layers = _step_names(device, None)
    rows = "vis_gemv_bf16_rows"
    assert names == ["vis_gather_rows"] + [rows, "vis_decode_attn_draft", rows, rows, rows] * layers + \
        [rows, "vis_spec_accept", "vis_spec_draft"]
    with_pred, _ = _step_names(device, [5, 6, 7])
    assert with_pred == names[:-1] + ["vis_spec_draft_pred"]
