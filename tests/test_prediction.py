"""Predicted outputs without a GPU: the drafter's definition (spec.propose_pred) on hand-worked cases, the model-free walk
that gives a run's counters (spec.simulate_prediction), the request's argument and every refusal - through ``create``,
``client.check_speculative_request`` and the engines' ``generate`` - before any GPU work."""
import math

import pytest

from test_speculative import MSGS, REFUSED

PRED = {"type": "content", "content": "the reply, probably"}


def _walk(pred, chunks, k=3, hi=4, lo=2, prompt=()):
    """propose_pred over a reply that grows by ``chunks``: [(draft, state)] after every call."""
    from vision_inspection_system_amd.spec import PredState, propose_pred
    state, reply, out = PredState(), [], []
    for c in chunks:
        reply = reply + list(c)
        draft, state = propose_pred(state, prompt, reply, pred, k, hi, lo)
        out.append((draft, tuple(state)))
    return out


# ------------------------------------------------------------------------------------------------------- propose_pred
def test_cursor_advances_through_a_full_match():
    pred = [10, 11, 12, 13, 14, 15, 16]
    got = _walk(pred, [[10], [11, 12, 13, 14], [15, 16, 99]])
    #               draft          cursor last seen src n_out acc rej
    assert got[0] == ([11, 12, 13], (1, 0, 1, 2, 3, 0, 0))       # behind the prompt pass's pick: pred[1:1+k]
    assert got[1] == ([15, 16], (5, 0, 5, 2, 2, 3, 0))           # three drafts kept and the step's own token; d = P - cursor
    assert got[2] == ([], (-1, 7, 8, 0, 0, 5, 0))                # the cursor stood at P when 99 came: lost there, nothing to draft


def test_substituted_id_loses_the_cursor_and_re_anchors_forward():
    pred = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    got = _walk(pred, [[1], [2, 3, 40], [5], [6]])               # the reply has 40 where the prediction has 4
    assert got[0] == ([2, 3, 4], (1, 0, 1, 2, 3, 0, 0))
    assert got[1] == ([], (-1, 3, 4, 0, 0, 2, 1))                # 2 kept, 1 not; lost at 3; [3, 40] stands nowhere
    assert got[2] == ([], (-1, 3, 5, 0, 0, 2, 1))                # [40, 5] neither: one id is below lookup_min = 2
    assert got[3] == ([7, 8, 9], (6, 3, 6, 2, 3, 2, 1))          # [5, 6] ends at e = 6 >= last
    # with lookup_min = 1 the first id behind the substitution already finds the place
    got = _walk(pred, [[1], [2, 3, 40], [5]], lo=1)
    assert got[2] == ([6, 7, 8], (5, 3, 5, 2, 3, 2, 1))


def test_deleted_and_inserted_segment():
    pred = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    got = _walk(pred, [[1], [2, 3, 7], [8], [9, 10]])            # 4 5 6 are missing from the reply
    assert got[1] == ([], (-1, 3, 4, 0, 0, 2, 1))
    assert got[2] == ([9, 10], (8, 3, 5, 2, 2, 2, 1))            # [7, 8] ends at e = 8; two ids are left
    assert got[3] == ([], (10, 3, 7, 0, 0, 3, 2))                # 9 kept, 10 was the step's own token: counted as not kept
    pred = [1, 2, 3, 4, 5, 6]
    got = _walk(pred, [[1], [2, 50], [51], [3], [4]])            # 50 51 stand in the reply only
    assert got[1] == ([], (-1, 2, 3, 0, 0, 1, 2))
    assert got[2][0] == [] and got[3][0] == []
    assert got[4] == ([5, 6], (4, 2, 6, 2, 2, 1, 2))             # [3, 4] ends at e = 4 >= last = 2


def test_repeated_template_takes_the_backward_candidate():
    pred = [20, 21, 22, 30, 31, 40]
    got = _walk(pred, [[20], [21, 22, 30, 31], [20], [21]])      # the reply starts the entry again instead of closing (40)
    assert got[1] == ([40], (5, 0, 5, 2, 1, 3, 0))
    assert got[2] == ([], (-1, 5, 6, 0, 0, 3, 1))
    assert got[3] == ([22, 30, 31], (2, 5, 7, 2, 3, 3, 1))       # [20, 21] ends at e = 2 only: behind last = 5, taken


def test_forward_candidate_first_then_the_nearest_behind():
    from vision_inspection_system_amd.spec import PredState, propose_pred
    pred = [1, 2, 3, 9, 1, 2, 4, 9, 1, 2, 5]                     # [1, 2] ends at e = 2, 6 and 10
    for last, cursor, draft in ((0, 2, [3, 9, 1]), (5, 6, [4, 9, 1]), (6, 6, [4, 9, 1]), (7, 10, [5]), (11, 10, [5])):
        d, st = propose_pred(PredState(cursor=-1, last=last, seen=2), [], [1, 2], pred, 3, 4, 2)
        assert (d, st.cursor, st.last, st.src) == (draft, cursor, last, 2), last
    # the longer window decides before the place does: [9, 1, 2] ends at 6 and 10, and last = 0 would prefer e = 2
    d, st = propose_pred(PredState(cursor=-1, last=0, seen=3), [], [9, 1, 2], pred, 2, 4, 2)
    assert (d, st.cursor) == ([4, 9], 6)
    # a candidate needs an id behind it: [2, 5] ends at P
    d, st = propose_pred(PredState(cursor=-1, last=0, seen=2), [], [2, 5], pred, 3, 4, 2)
    assert (d, st.cursor, st.src) == ([], -1, 0)


def test_short_predictions_and_the_end_of_the_prediction():
    from vision_inspection_system_amd.spec import PredState, propose, propose_pred
    prompt = [6, 7, 8, 9]
    # P = 0: the prompt lookup, always
    hist = prompt + [5, 6, 7]
    assert propose(hist, 3) == [8, 9, 5]
    assert propose_pred(PredState(), prompt, [5, 6, 7], [], 3) == ([8, 9, 5], PredState(-1, 0, 3, 1, 3, 0, 0))
    # P = 1: the one id can only be confirmed, never drafted
    assert propose_pred(PredState(), prompt, [5], [5], 3) == ([], PredState(1, 0, 1, 0, 0, 0, 0))
    assert propose_pred(PredState(), prompt, [4], [5], 3) == ([], PredState(-1, 0, 1, 0, 0, 0, 0))
    # P = k
    assert propose_pred(PredState(), prompt, [5], [5, 6, 7], 3) == ([6, 7], PredState(1, 0, 1, 2, 2, 0, 0))
    # the cursor reaches P: the prompt lookup drafts, and what becomes of ITS drafts is not counted
    d, st = propose_pred(PredState(), prompt, [5, 6, 7], [5, 6, 7], 3)
    assert (d, st) == ([8, 9, 5], PredState(3, 0, 3, 1, 3, 0, 0))
    d, st = propose_pred(st, prompt, [5, 6, 7, 8, 1], [5, 6, 7], 3)
    assert (st.accepted, st.rejected, st.cursor, st.last) == (0, 0, -1, 3)
    # ids are clamped into the vocabulary like vis_spec_draft's
    assert propose_pred(PredState(), [], [5], [5, 600, 7], 3, vocab=512)[0] == [511, 7]
    # a call without a new token (a step issued behind the request's limit) counts nothing and drafts the same
    d, st = propose_pred(PredState(), [], [5], [5, 6, 7, 8], 3)
    assert propose_pred(st, [], [5], [5, 6, 7, 8], 3) == (d, st)


def test_rejected_counts_only_prediction_sourced_drafts():
    prompt = [1, 2, 3, 4, 1, 2]
    got = _walk([50, 51, 52, 53], [[3], [9], [50, 51], [52, 7]], prompt=prompt)
    assert got[0] == ([4, 1, 2], (-1, 0, 1, 1, 3, 0, 0))         # the prediction does not start the reply: prompt lookup
    assert got[1] == ([], (-1, 0, 2, 0, 0, 0, 0))                # all three refused - not the prediction's
    assert got[2] == ([52, 53], (2, 0, 4, 2, 2, 0, 0))
    assert got[3] == ([], (-1, 3, 6, 0, 0, 1, 1))                # 52 kept, 53 not


# ------------------------------------------------------------------------------------------------ simulate_prediction
@pytest.mark.parametrize("N", [5, 13, 25, 24, 22])
def test_simulate_prediction_that_holds(N):
    """pred = the plain reply, k = 3: ceil((N - 1) / 4) steps, accepted = N - 1 - steps.  Nothing is rejected when the last
    step has room for its four tokens ((N - 1) % 4 == 0); otherwise the last step proposes min(3, N - n) drafts behind n
    tokens and the request's limit keeps one fewer (a step's last token is its own), which the definition counts as not
    kept: rejected = 1."""
    from vision_inspection_system_amd.spec import simulate_prediction
    plain = list(range(100, 100 + N))
    r = simulate_prediction(plain, [1, 2, 3], plain, 3, 4, 2, N)
    steps = math.ceil((N - 1) / 4)
    assert r["reply"] == plain and r["spec_steps"] == steps
    assert r["spec_accepted"] == r["pred_accepted"] == N - 1 - steps
    assert r["pred_rejected"] == (0 if (N - 1) % 4 == 0 else 1)
    assert r["spec_proposed"] == r["pred_accepted"] + r["pred_rejected"]


def test_simulate_unrelated_shorter_and_longer_predictions():
    from vision_inspection_system_amd.spec import simulate_prediction
    N = 25
    plain = list(range(100, 100 + N))
    r = simulate_prediction(plain, [1, 2, 3], list(range(300, 340)), 3, 4, 2, N)      # a disjoint id range
    assert r == {"reply": plain, "spec_steps": N - 1, "spec_proposed": 0, "spec_accepted": 0, "pred_accepted": 0,
                 "pred_rejected": 0}
    r = simulate_prediction(plain, [1, 2, 3], plain[:9], 3, 4, 2, N)                   # shorter than the reply
    assert r["reply"] == plain and r["spec_steps"] == 2 + 16 and (r["pred_accepted"], r["pred_rejected"]) == (6, 0)
    r = simulate_prediction(plain, [1, 2, 3], plain + [7] * 30, 3, 4, 2, N)            # longer
    assert r["reply"] == plain and r["spec_steps"] == 6 and (r["pred_accepted"], r["pred_rejected"]) == (18, 0)
    r = simulate_prediction(plain, [1, 2, 3], plain, 1, 4, 2, N)                       # k = 1
    assert r["spec_steps"] == 12 and (r["pred_accepted"], r["pred_rejected"]) == (12, 0)
    # max_new_tokens below the plain reply's length cuts the walk there
    r = simulate_prediction(plain, [1, 2, 3], plain, 3, 4, 2, 9)
    assert r["reply"] == plain[:9] and r["spec_steps"] == 2


# --------------------------------------------------------------------------------------------------------- validation
MALFORMED = [7, "text", ["text"], {}, {"type": "content"}, {"type": "text", "content": "x"}, {"content": "x"},
             {"type": "content", "content": 5}, {"type": "content", "content": None},
             {"type": "content", "content": ["x"]}, {"type": "content", "content": [{"type": "text", "text": 5}]},
             {"type": "content", "content": [{"type": "image_url", "text": "x"}]},
             {"type": "content", "content": [{"type": "text"}]}, {"type": "content", "content": "x", "extra": 1}]


def test_check_prediction():
    from vision_inspection_system_amd.spec import PRED_DEFAULT, SpecConfig, check_prediction, check_prediction_ids, with_prediction
    assert check_prediction(None) is None
    assert check_prediction({"type": "content", "content": "abc"}) == "abc"
    assert check_prediction({"type": "content", "content": [{"type": "text", "text": "ab"}, {"type": "text", "text": "c"}]}) == "abc"
    assert check_prediction({"type": "content", "content": ""}) is None          # empty = no prediction
    assert check_prediction({"type": "content", "content": []}) is None
    for bad in MALFORMED:
        with pytest.raises(ValueError, match="prediction"):
            check_prediction(bad)
    assert check_prediction_ids(None) is None and check_prediction_ids([]) is None
    assert check_prediction_ids(range(10), 4) == [0, 1, 2, 3]                     # at most max_ctx ids are kept
    for bad in ("abc", {"type": "content"}, [1.5], [True], [-1], 7):
        with pytest.raises(ValueError, match="prediction"):
            check_prediction_ids(bad)
    # a prediction alone implies k = 3, window 4..2; speculative= next to it sets k and the window
    assert PRED_DEFAULT == SpecConfig(3, 4, 2)
    assert with_prediction(None, True) == SpecConfig(3, 4, 2) and with_prediction(None, False) is None
    assert with_prediction({"method": "ngram", "num_speculative_tokens": 1, "prompt_lookup_max": 6}, True) == SpecConfig(1, 6, 2)
    assert with_prediction(2, False) == SpecConfig(2, 4, 2)


def test_check_speculative_request_with_prediction():
    from vision_inspection_system_amd.client import check_speculative_request
    from vision_inspection_system_amd.spec import SpecConfig
    assert check_speculative_request(None, prediction=PRED) == SpecConfig(3, 4, 2)
    assert check_speculative_request({"method": "ngram", "num_speculative_tokens": 1}, prediction=PRED) == SpecConfig(1, 4, 2)
    assert check_speculative_request(None, prediction=None) is None
    assert check_speculative_request(None, 0.7, 3, prediction={"type": "content", "content": ""}, top_p=0.5) is None
    for bad in MALFORMED:
        with pytest.raises(ValueError, match="prediction"):
            check_speculative_request(None, prediction=bad)


@pytest.mark.parametrize("case", REFUSED, ids=[f"{c[0]}-{i}" for i, c in enumerate(REFUSED)])
def test_create_refuses_excluded_switches(case):
    from vision_inspection_system_amd.client import CannedResponseClient, LocalVLMClient, check_speculative_request
    name, value = case[0], case[1]
    with pytest.raises(ValueError, match="prediction"):
        check_speculative_request(None, prediction=PRED, **{name: value})
    for client in (LocalVLMClient(), CannedResponseClient()):
        with pytest.raises(ValueError, match="prediction"):
            client.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8, prediction=PRED, **{name: value})


def test_create_refuses_malformed_mllama_and_batches():
    from vision_inspection_system_amd.client import CannedResponseClient, LocalVLMClient
    local, canned = LocalVLMClient(), CannedResponseClient()
    for client in (local, canned):
        for bad in MALFORMED:
            with pytest.raises(ValueError, match="prediction"):
                client.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8, prediction=bad)
        with pytest.raises(ValueError, match="Qwen2-VL"):
            client.chat.completions.create(model="synthetic:mllama-tiny", messages=MSGS, max_tokens=8, prediction=PRED)
    with pytest.raises(ValueError, match="prediction"):
        local.complete_many("synthetic:tiny", [MSGS], prediction=PRED)
    # the canned client records the argument and otherwise ignores it; neutral values next to it are no conflict
    canned.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8, prediction=PRED, temperature=0.0, n=1)
    assert canned.calls[-1]["prediction"] == PRED and "speculative" not in canned.calls[-1]
    canned.chat.completions.create(model="synthetic:tiny", messages=MSGS, max_tokens=8)
    assert "prediction" not in canned.calls[-1]


@pytest.mark.parametrize("case", [c for c in REFUSED if c[2]], ids=[c[2] for c in REFUSED if c[2]])
def test_generate_refuses_excluded_switches(case):
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    eng = Qwen2VLEngine.__new__(Qwen2VLEngine)
    with pytest.raises(ValueError, match="prediction"):
        eng.generate([1, 2, 3], prediction=[4, 5, 6], **{case[2]: case[3]})


def test_generate_refuses_mllama_batches_and_malformed():
    from vision_inspection_system_amd.engine import Qwen2VLEngine
    from vision_inspection_system_amd.mllama_engine import MllamaEngine
    with pytest.raises(ValueError, match="Qwen2-VL"):
        MllamaEngine.__new__(MllamaEngine).generate([1, 2, 3], prediction=[4, 5])
    for E in (Qwen2VLEngine, MllamaEngine):
        with pytest.raises(ValueError, match="prediction"):
            E.__new__(E).generate_batch([([1, 2, 3], [])], prediction=[4, 5])
    with pytest.raises(ValueError, match="prediction"):
        Qwen2VLEngine.__new__(Qwen2VLEngine).generate([1, 2, 3], prediction="abc")


def test_off_state_names_no_new_launch():
    """Without a prediction the speculative step ends with vis_spec_draft: the new drafter is reached through one flag that
    only _spec_begin sets, and the plain steps name neither."""
    import inspect
    from vision_inspection_system_amd.decode_stage import DecodeStage
    for fn in (DecodeStage._decode_step_rows, DecodeStage._decode_step_streamk, DecodeStage._decode_step_fused):
        assert "spec" not in inspect.getsource(fn)
    src = inspect.getsource(DecodeStage._decode_step_spec)
    assert "self._spec_pred" in src and "hip.spec_draft(" in src
