"""generation.Generation without a GPU: stub engines on the CPU.  Each stub derives from one of the real engine classes, so a
case runs through that engine's public ``generate`` / ``generate_batch`` - its spelling (``ignore_eos`` / ``check_every`` or
``stop_on_eos`` / ``chunk``), its class flags and its small hooks - while everything that would launch is a recorder on small
CPU tensors: the prompt passes, ``decode`` / the graph replay / the eager batched step (they advance a scripted reply), the
request scope, the polls, the fork, and what runs after the loop.  Asserted is the sequence of those calls."""
import contextlib

import pytest
import torch

from vision_inspection_system_amd import hip
from vision_inspection_system_amd.engine import Qwen2VLEngine
from vision_inspection_system_amd.generation import Generation
from vision_inspection_system_amd.json_mode import JsonModeError
from vision_inspection_system_amd.mllama_engine import MllamaEngine

V, T, SLOTS, EVERY = 100, 64, 4, 4
EOS = V - 1
IDS = list(range(1, 11))          # a prompt of 10 tokens: room for 53 new ones in the context of 64


class _Cfg:
    vocab, eos_ids = V, (EOS,)


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass

    def elapsed_time(self, other):
        return 0.0


@pytest.fixture(autouse=True)
def no_device_events(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", _Event)


class _Graph:
    def __init__(self, eng, B):
        self.eng, self.B = eng, B

    def replay(self):
        self.eng.log.append(("replay", self.B))
        self.eng._advance(range(self.B), 1)


class Recorders:
    """What the loops call, recorded in ``log``; the "model" writes ``script[slot]`` token by token into the slot's row."""

    def __init__(self):
        self.cfg, self.max_batch, self.max_ctx, self.device = _Cfg(), SLOTS, T, torch.device("cpu")
        self._tok = torch.zeros((SLOTS, T), dtype=torch.int32)
        self.tokens = self._tok[0]
        self.chain_sync, self.batch_shared_len = None, 64
        self.slot_prompt_len = [0] * SLOTS
        self.count = [0] * SLOTS
        self.script = [[(7 * s + i) % 90 + 1 for i in range(T)] for s in range(SLOTS)]      # no EOS unless a case plants one
        self.log = []
        self.stop_at = None              # with stop strings on: the rows have all ended once each has this many tokens
        self.cancel_at = None            # the reader's owner gives up once row 0 has this many tokens
        self.prefill_result = None       # (slots, errors) of prefill_many; None: every request gets its slot
        self.children = 0                # further choices _fork_choices gives request 0
        self.stall = 0                   # decode() calls that still raise ChainStalled
        self.mask_failed = []
        self._init_decode_stage([], None, None)

    # the model
    def _advance(self, slots, n):
        for s in slots:
            for _ in range(n):
                self._tok[s, self.slot_prompt_len[s] - 1 + self.count[s]] = self.script[s][self.count[s]]
                self.count[s] += 1

    def _start(self, slot, n_ids):
        self.slot_prompt_len[slot], self.count[slot] = n_ids, 0
        self._advance([slot], 1)

    @property
    def tokens_b(self):
        self.log.append(("read_rows",))
        return self._tok

    # hooks of the engines
    def _prompt_pass(self, input_ids, frames, max_new_tokens, temperature, seed):
        self.log.append(("prompt_pass", max_new_tokens))
        self.prompt_len = len(input_ids)
        self._start(0, len(input_ids))

    def prefill_many(self, requests, temperature=0.0, seed=0, max_new_tokens=None, seeds=None, penalties=None, shaping=None):
        self.log.append(("prefill_many", len(requests)))
        if self.prefill_result is not None:
            slots, errors = self.prefill_result
        else:
            slots, errors = list(range(len(requests))), [None] * len(requests)
        for r, s in zip(requests, slots):
            if s is not None:
                self._start(s, len(r[0]))
        return slots, errors

    def _batch_graph(self, B):
        self.log.append(("graph", B))
        return _Graph(self, B)

    def _decode_step_batched(self, B):
        self.log.append(("step", B))
        self._advance(range(B), 1)

    def decode(self, n_steps, use_graph=True):
        self.log.append(("decode", n_steps))
        if self.stall:
            self.stall -= 1
            raise hip.ChainStalled("stalled")
        self._advance([0], n_steps)

    def disable_chain(self):
        self.log.append(("stall_hook",))

    def _maybe_reenable_chain(self):
        self.log.append(("clean",))

    # PickStage / DecodeStage
    @contextlib.contextmanager
    def _pick_request(self, logprobs, json_mode, json_schema, top_p, seeded, penalties, stop=None, *, shaping=None,
                      on_stream=None):
        self.log.append(("scope", seeded))
        self.stop_on = stop is not None or on_stream is not None
        self.stream_on = on_stream is not None
        self.last_logprobs = self.last_finish = None
        try:
            yield
        finally:
            self.stop_on = self.stream_on = False
            self.log.append(("scope_end",))

    def generated(self, n):
        self.log.append(("read_row", n))
        return Generation.generated(self, n)

    def _stop_done(self, slots):
        slots = list(slots)
        self.log.append(("stop_done", slots))
        return all(self.count[s] >= self.stop_at for s in slots)

    def _stream_cancelled(self):
        return self.stream_on and self.cancel_at is not None and self.count[0] >= self.cancel_at

    def _stream_bind(self, choice_slots):
        self.log.append(("bind", choice_slots))

    def _fork_choices(self, roots, n, prefix_len, seeds, penalties, shaping):
        self.log.append(("fork", list(roots), list(n), prefix_len))
        live = [s for s in roots if s is not None]
        out = [None if s is None else [s] for s in roots]
        for c in range(self.children):
            child = len(live) + c
            self.slot_prompt_len[child], self.count[child] = self.slot_prompt_len[0], 0
            self._advance([child], 1)
            out[roots.index(0)].append(child)
            self.fork_on = True
        return out

    def _finish(self, rows, eos_ids, ignore_eos, keep_eos=False):
        self.log.append(("finish", ignore_eos, keep_eos))
        if self.stop_on:                 # the device records are not modelled: uncut
            self.last_finish = [("stop", 0) for _ in rows]
            return [r[1] for r in rows]
        return Generation._finish(self, rows, eos_ids, ignore_eos, keep_eos=keep_eos)

    def _record_logprobs(self, rows):
        self.log.append(("logprobs", list(rows)))

    def _mask_failed(self, slots):
        self.log.append(("mask_failed", list(slots)))
        return [s for s in slots if s in self.mask_failed]


ENGINES = {"ignore_eos": Qwen2VLEngine, "stop_on_eos": MllamaEngine}


@pytest.fixture(params=[(sp, k) for sp in ENGINES for k in (False, True)], ids=lambda p: f"{p[0]}-keep_eos={p[1]}")
def eng(request):
    spelling, keep = request.param
    cls = type("Stub", (Recorders, ENGINES[spelling]), {"keep_eos": keep, "spelling": spelling})
    return cls()


def generate(eng, max_new, ignore_eos=False, every=EVERY, ids=IDS, **kw):
    if eng.spelling == "ignore_eos":
        return eng.generate(ids, ["frame"], max_new_tokens=max_new, ignore_eos=ignore_eos, check_every=every, **kw)
    return eng.generate(ids, "frame", max_new_tokens=max_new, stop_on_eos=not ignore_eos, chunk=every, **kw)


def generate_batch(eng, n_req, max_new, ignore_eos=False, every=EVERY, requests=None, **kw):
    requests = requests or [(IDS, "frame")] * n_req
    if eng.spelling == "ignore_eos":
        return eng.generate_batch(requests, max_new_tokens=max_new, ignore_eos=ignore_eos, check_every=every, **kw)
    return eng.generate_batch(requests, max_new_tokens=max_new, stop_on_eos=not ignore_eos, chunk=every, **kw)


def names(eng, *which):
    return [c[0] for c in eng.log if not which or c[0] in which]


def chunks(eng):
    """The decode work between two polls: the sizes of the decode() calls, or the runs of replays / eager steps."""
    out, run = [], 0
    for c in eng.log:
        if c[0] == "decode":
            out.append(c[1])
        elif c[0] in ("replay", "step"):
            run += 1
        elif run:
            out.append(run)
            run = 0
    return out + ([run] if run else [])


def want_chunks(steps, every):
    return [every] * (steps // every) + ([steps % every] if steps % every else [])


def cut(eng, toks):
    """Through the first EOS: without it, or with it for an engine that keeps it."""
    return toks[:toks.index(EOS) + (1 if eng.keep_eos else 0)] if EOS in toks else toks


# ----------------------------------------------------------------------------- polling
def test_single_with_stop_polls_the_records_and_never_the_row(eng):
    eng.stop_at = 7
    for ignore_eos in (False, True):
        del eng.log[:]
        out = generate(eng, 12, ignore_eos=ignore_eos, stop="x")
        assert out == eng.script[0][:9] and eng.last_timing["decode_steps"] == 8 and eng.last_timing["sequences"] == 1
        assert names(eng, "prompt_pass", "stop_done", "decode", "read_row") == \
            ["prompt_pass", "stop_done", "decode", "stop_done", "decode", "stop_done", "read_row"]
        assert chunks(eng) == [4, 4] and eng.log[-1] == ("scope_end",)
        assert ("finish", ignore_eos, eng.keep_eos) in eng.log and eng.stop_eos is (not ignore_eos)


def test_batch_with_stop_polls_the_records_and_reads_the_rows_once(eng):
    eng.stop_at = 3
    out = generate_batch(eng, 2, 12, stop="x")
    assert out == [eng.script[0][:5], eng.script[1][:5]]
    assert names(eng, "stop_done", "read_rows") == ["stop_done", "stop_done", "read_rows"]
    assert [c[1] for c in eng.log if c[0] == "stop_done"] == [[0, 1], [0, 1]] and chunks(eng) == [4]


def test_single_eos_ends_at_the_poll_that_sees_it(eng):
    eng.script[0][5] = EOS
    out = generate(eng, 12)
    assert out == cut(eng, eng.script[0][:9]) and len(out) == 5 + eng.keep_eos and eng.last_finish == [("eos", None)]
    assert names(eng, "read_row", "decode") == ["read_row", "decode", "read_row", "decode", "read_row", "read_row"]
    assert eng.last_timing["decode_steps"] == 8 and ("clean",) in eng.log


def test_batch_ends_only_when_every_row_has_an_eos(eng):
    eng.script[0][2], eng.script[1][6] = EOS, EOS
    out = generate_batch(eng, 2, 12)
    assert out == [cut(eng, eng.script[0][:9]), cut(eng, eng.script[1][:9])]
    assert [len(o) for o in out] == [2 + eng.keep_eos, 6 + eng.keep_eos]
    assert chunks(eng) == [4, 4] and eng.last_timing["decode_steps"] == 8 and eng.last_timing["sequences"] == 2
    assert eng.last_finish == [("eos", None)] * 2
    # the graph is asked for once, for both rows; then one read of the rows per poll (three) and the final one
    assert names(eng, "read_rows", "graph") == ["graph"] + ["read_rows"] * 4 and ("graph", 2) in eng.log


def test_ignore_eos_is_issued_in_one_go(eng):
    eng.script[0][1] = eng.script[1][1] = EOS
    out = generate(eng, 12, ignore_eos=True)
    assert out == eng.script[0][:12] and eng.last_finish == [("length", None)]
    assert names(eng, "decode", "read_row") == ["decode", "read_row"] and chunks(eng) == [11]
    del eng.log[:]
    out = generate_batch(eng, 2, 12, ignore_eos=True, use_graph=False)
    assert out == [eng.script[0][:12], eng.script[1][:12]]
    assert names(eng, "step", "read_rows", "graph") == ["step"] * 11 + ["read_rows"]


# ----------------------------------------------------------------------------- step counts
@pytest.mark.parametrize("max_new", [1, 2, EVERY, EVERY + 1, 11, 60])
@pytest.mark.parametrize("n_ids", [10, 57])
def test_step_counts_and_chunks(eng, max_new, n_ids):
    """min(max_new, room) - 1 steps in chunks of ``check_every``; room = context - prompt - 1 (53, or 6 behind 57 tokens)."""
    ids = list(range(1, n_ids + 1))
    room = T - n_ids - 1
    steps = min(max_new, room) - 1
    out = generate(eng, max_new, ids=ids)
    assert len(out) == steps + 1 and eng.last_timing["decode_steps"] == steps and chunks(eng) == want_chunks(steps, EVERY)
    # Qwen2-VL's prompt pass prepares rope rows for the clamped reply; Mllama's is handed the request's figure and ignores it
    assert ("prompt_pass", min(max_new, room) if eng.spelling == "ignore_eos" else max_new) in eng.log
    del eng.log[:]
    out = generate_batch(eng, 2, max_new, requests=[(ids, "frame"), (IDS, "frame")])
    assert [len(o) for o in out] == [steps + 1] * 2 and eng.last_timing["decode_steps"] == steps
    assert chunks(eng) == want_chunks(steps, EVERY) and eng.last_timing["prompt_tokens"] == max(n_ids, len(IDS))


def test_the_context_clamp_warns_once_per_engine_and_only_for_qwen(eng, caplog):
    with caplog.at_level("WARNING", logger="vision_inspection_system_amd.engine"):
        generate(eng, 60)
        generate(eng, 60)
    said = [r for r in caplog.records if "does not fit the context" in r.getMessage()]
    assert len(said) == (1 if eng.spelling == "ignore_eos" else 0)


# ----------------------------------------------------------------------------- streaming
def test_a_cancelled_stream_ends_at_the_next_chunk_boundary(eng):
    eng.stop_at, eng.cancel_at = 99, 3
    reader = object()
    out = generate(eng, 12, on_stream=reader)
    assert out == eng.script[0][:5] and chunks(eng) == [4] and eng.last_timing["decode_steps"] == 4
    assert ("bind", [[0]]) in eng.log
    del eng.log[:]
    out = generate_batch(eng, 2, 12, on_stream=reader)
    assert out == [eng.script[0][:5], eng.script[1][:5]] and chunks(eng) == [4]
    assert ("bind", [[0], [1]]) in eng.log


# ----------------------------------------------------------------------------- the front end of a batch
def test_all_requests_failed(eng):
    e1, e2 = ValueError("a"), OSError("b")
    eng.prefill_result = ([None, None], [e1, e2])
    out = generate_batch(eng, 2, 12, requests=[lambda: None, lambda: None], logprobs=2)
    assert out == [e1, e2] and eng.last_finish == [None, None]
    assert names(eng) == ["scope", "prefill_many", "logprobs", "scope_end"] and ("logprobs", [None, None]) in eng.log


def test_a_failed_request_keeps_its_exception_and_the_others_run(eng):
    err = ValueError("no image")
    eng.prefill_result = ([0, None, 1], [None, err, None])
    out = generate_batch(eng, 3, 6, requests=[(IDS, "frame"), lambda: None, (IDS, "frame")])
    assert out == [eng.script[0][:6], err, eng.script[1][:6]] and eng.last_finish == [("length", None), None, ("length", None)]
    assert ("fork", [0, None, 1], [1, 1, 1], 64 if eng.spelling == "ignore_eos" else 0) in eng.log
    assert ("bind", [[0], None, [1]]) in eng.log and eng.last_timing["sequences"] == 2


def test_one_request_with_one_choice_is_the_single_route_nested(eng):
    plain = generate_batch(eng, 1, 12)
    assert plain == [eng.script[0][:12]] and eng.last_finish == [("length", None)]
    # the single-sequence loop, polled at the call's interval (Qwen2-VL) or at the default chunk of Mllama's generate
    every = eng.single_route_check_every or EVERY
    assert every == (EVERY if eng.spelling == "ignore_eos" else 32)
    assert "prefill_many" not in names(eng) and chunks(eng) == want_chunks(11, every)
    del eng.log[:]
    out = generate_batch(eng, 1, 12, n=1)
    assert out == [plain] and eng.last_finish == [[("length", None)]] and eng.last_logprobs is None
    assert "prefill_many" not in names(eng) and chunks(eng) == want_chunks(11, every)


def test_one_lazy_request_fails_on_its_own(eng):
    def boom():
        raise OSError("decode failed")
    out = generate_batch(eng, 1, 12, requests=[boom], logprobs=1)
    assert isinstance(out[0], OSError) and eng.last_finish == [None] and eng.last_logprobs == [None]
    assert names(eng) == []
    # the grammar mask could not continue the reply: the error is the request's entry, lazy or not
    eng.mask_failed = [0]
    for requests in ([(IDS, "frame")], [lambda: (IDS, "frame")]):
        out = generate_batch(eng, 1, 12, requests=requests, json_mode=True)
        assert isinstance(out[0], JsonModeError) and eng.last_finish == [None]
    with pytest.raises(JsonModeError):
        generate(eng, 12, json_mode=True)


def test_n_choices_fork_behind_the_roots_and_nest(eng):
    eng.children = 1
    eng.script[2] = list(eng.script[0])
    out = generate_batch(eng, 2, 6, ignore_eos=True, n=[2, 1], temperature=0.7, seeds=[3, 4])
    assert out == [[eng.script[0][:6]] * 2, [eng.script[1][:6]]]
    assert eng.last_finish == [[("length", None)] * 2, [("length", None)]] and eng.last_timing["sequences"] == 3
    assert ("scope", True) in eng.log and ("graph", 3) in eng.log and ("bind", [[0, 2], [1]]) in eng.log
    assert eng.fork_on is False


def test_fork_on_is_off_again_after_an_exception_in_the_loop(eng, monkeypatch):
    eng.children = 1

    def broken(B):
        assert eng.fork_on
        raise RuntimeError("boom")
    monkeypatch.setattr(eng, "_batch_graph", broken)
    with pytest.raises(RuntimeError, match="boom"):
        generate_batch(eng, 2, 6, n=[2, 1])
    assert eng.fork_on is False and eng.log[-1] == ("scope_end",)


def test_the_checks_come_in_order_and_before_anything_runs(eng):
    for kw, message in ((dict(logprobs=21, json_mode=1), "logprobs"), (dict(json_mode=1, top_p=2.0), "json_mode"),
                        (dict(top_p=2.0, seeds=[1]), "top_p"), (dict(seeds=[1], n=9), "seeds"), (dict(n=9), "n")):
        with pytest.raises(ValueError, match=message):
            generate_batch(eng, 2, 6, **kw)
    with pytest.raises(ValueError, match="does not fit max_batch"):
        generate_batch(eng, 5, 6, logprobs=21)
    assert eng.log == []


def test_mllama_wants_an_image_in_every_request_of_a_batch(eng):
    requests = [(IDS, "frame"), (IDS, None)]
    if eng.spelling == "stop_on_eos":
        with pytest.raises(ValueError, match="needs an image in every request"):
            generate_batch(eng, 2, 6, requests=requests)
        assert eng.log == []
    else:
        assert len(generate_batch(eng, 2, 6, requests=requests)) == 2


# ----------------------------------------------------------------------------- a stalled chained launch
def test_chain_stalled_is_served_again_once_through_the_stall_hook(eng):
    eng.stall = 1
    out = generate(eng, 12)
    assert out == eng.script[0][:12]
    assert names(eng, "prompt_pass", "stall_hook", "clean") == ["prompt_pass", "stall_hook", "prompt_pass"]
    assert names(eng, "scope", "scope_end") == ["scope", "scope_end"]          # the same request scope serves the retry
    eng.stall = 2                                                               # a second stall is not caught
    with pytest.raises(hip.ChainStalled):
        generate(eng, 12)
    assert names(eng, "stall_hook").count("stall_hook") == 2
