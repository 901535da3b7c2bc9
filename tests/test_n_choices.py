"""``n`` choices per request, host side: the check of ``n``, the slot layout and fork tables (fork.py) and their contract, the
mock client's n choices, and the client's chunking by choices through a host-only engine stand-in.  No GPU."""
import threading

import pytest

from vision_inspection_system_amd import client as CL
from vision_inspection_system_amd.fork import check_fork_tables, check_n_list, fork_layout


def test_check_n():
    assert CL.check_n(None, 8) is None
    assert CL.check_n(1, 8) == 1 and CL.check_n(8, 8) == 8
    for bad in (0, -1, True, 2.0, "2", 9):
        with pytest.raises(ValueError):
            CL.check_n(bad, 8)
    assert check_n_list(None, 3, 8) is None
    assert check_n_list(2, 3, 8) == [2, 2, 2]
    assert check_n_list([2, 1, 5], 3, 8) == [2, 1, 5]
    for bad in ([2, 1], [2, None, 1], [3, 3, 3], 3, "21", [True, 1, 1]):
        with pytest.raises(ValueError):
            check_n_list(bad, 3, 8)


def test_layout_roots_first_children_behind():
    lay = fork_layout([200, 40, 130], [3, 2, 1], 0, 8)
    assert lay.slots == [[0, 3, 4], [1, 5], [2]]
    # S = 200: the children read [0, 192) from their root and get [192, 200) copied
    assert [lay.parent[s] for s in (3, 4)] == [0, 0] and [lay.fork_len[s] for s in (3, 4)] == [192, 192]
    assert (3, 0, 192, 200) in lay.copies and (4, 0, 192, 200) in lay.copies
    # S = 40: nothing to share below one split - fork_len 0, the whole prompt copied
    assert lay.fork_len[5] == 0 and (5, 1, 0, 40) in lay.copies and len(lay.copies) == 3
    # roots read everything from their own cache
    assert lay.parent[:3] == [0, 1, 2] and lay.fork_len[:3] == [0, 0, 0]
    assert lay.holds == [200, 40, 130, 0, 0, 40]
    check_fork_tables(lay.parent, lay.fork_len, 256, lay.holds)


def test_layout_text_prefix_goes_through_the_tables():
    lay = fork_layout([200, 210], [2, 2], 128, 8)
    assert lay.slots == [[0, 2], [1, 3]]
    assert lay.parent == [0, 0, 0, 1] and lay.fork_len == [0, 128, 192, 192]      # root 1: parent 0, fork_len P
    check_fork_tables(lay.parent, lay.fork_len, 256, lay.holds)       # a child of root 1: the root holds the prefix rows itself
    with pytest.raises(ValueError):
        check_fork_tables(lay.parent, lay.fork_len, 256)               # ... which the tables alone cannot show
    no_children = fork_layout([200, 210, 220], [1, 1, 1], 64, 4)
    assert no_children.copies == [] and no_children.parent == [0, 0, 0] and no_children.fork_len == [0, 64, 64]


def test_layout_refuses_what_does_not_fit():
    with pytest.raises(ValueError):
        fork_layout([100, 100], [3, 2], 0, 4)
    fork_layout([100, 100], [2, 2], 0, 4)
    with pytest.raises(ValueError):
        fork_layout([100, 100], [2], 0, 4)
    with pytest.raises(ValueError):
        fork_layout([100], [0], 0, 4)
    with pytest.raises(ValueError):
        fork_layout([100], [1], 100, 4)        # a prefix is a multiple of 64


@pytest.mark.parametrize("lens,n,P", [([200], [8], 0), ([63, 64, 65], [2, 3, 3], 0), ([255, 129], [4, 4], 128),
                                       ([1], [2], 0), ([2249] * 8, [8] * 8, 960)])
def test_every_layout_passes_the_contract(lens, n, P):
    lay = fork_layout(lens, n, P, 64)
    check_fork_tables(lay.parent, lay.fork_len, 4096, lay.holds)
    assert sorted(s for cs in lay.slots for s in cs) == list(range(sum(n)))
    for child, root, lo, hi in lay.copies:
        assert lo == 64 * (lens[root] // 64) == lay.fork_len[child] and hi == lens[root] and hi - lo < 64
        assert lay.parent[child] == (root if lo else child)


def test_hand_made_tables_that_break_the_contract():
    check_fork_tables([0, 0, 0], [0, 64, 128])
    with pytest.raises(ValueError):
        check_fork_tables([0, 0, 1], [0, 64, 64])          # a child of a child
    with pytest.raises(ValueError):
        check_fork_tables([0, 0], [0, 100])                # not a multiple of 64
    with pytest.raises(ValueError):
        check_fork_tables([0, 2], [0, 64])                 # a parent outside the batch
    with pytest.raises(ValueError):
        check_fork_tables([0, -1], [0, 64])
    with pytest.raises(ValueError):
        check_fork_tables([0, 0], [0, 256], 256)           # a fork length outside the cache
    with pytest.raises(ValueError):
        check_fork_tables([0, 0], [0, 128], 256, [100, 0])     # the parent does not hold that many rows
    with pytest.raises(ValueError):
        check_fork_tables([0, 0], [0])


def test_mock_client_returns_n_choices():
    c = CL.make_client("mock", reply="fine")
    r = c.chat.completions.create(model="m", messages=[{"role": "user", "content": "x"}], n=3)
    assert [ch.index for ch in r.choices] == [0, 1, 2] and all(ch.message.content == "fine" for ch in r.choices)
    assert c.calls[-1]["n"] == 3
    one = c.chat.completions.create(model="m", messages=[{"role": "user", "content": "x"}])
    assert len(one.choices) == 1 and one.choices[0].index == 0 and "n" not in c.calls[-1]
    with pytest.raises(ValueError):
        c.chat.completions.create(model="m", messages=[], n=0)


class _HostOnlyEngine:
    """Stands where the engine stands and consumes the client's requests without a model (as bench.py --dry-ingest does)."""
    host_only = True

    def __init__(self, max_batch):
        self.max_batch, self.device, self.lock = max_batch, "cpu", threading.Lock()
        self.calls, self.last_timing, self.last_logprobs, self.last_finish = [], {}, None, None

    def generate_batch(self, requests, n=None, **kw):
        ids = [r()[0] for r in requests]
        self.calls.append((len(ids), n, kw.get("seeds")))
        reply = [65 + len(self.calls), 66]
        self.last_finish = [[("length", None)] * n if n else ("length", None) for _ in ids]
        return [[reply + [c] for c in range(n)] if n else reply for _ in ids]


def test_client_fills_chunks_by_choices():
    from vision_inspection_system_amd.config import Qwen2VLConfig
    from vision_inspection_system_amd.tokenizer import ByteTokenizer
    cfg = Qwen2VLConfig.tiny()
    tok = ByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.vision_start_id, cfg.vision_end_id, cfg.eos_ids)
    eng = _HostOnlyEngine(4)
    CL.register_model("host-only:n", "cpu", CL.LoadedModel(eng, tok, cfg, "host-only:n"))
    try:
        c = CL.LocalVLMClient(device="cpu")
        msgs = [[{"role": "user", "content": f"request {i}"}] for i in range(5)]
        out = c.complete_many("host-only:n", msgs, max_tokens=4, n=2, seed=3)
        assert [(b, n) for b, n, _ in eng.calls] == [(2, 2), (2, 2), (1, 2)]
        assert eng.calls[0][2] == [3, 3]                      # the request's seed; choice i adds i in the engine
        assert len(out) == 5
        for r in out:
            assert [ch.index for ch in r.choices] == [0, 1] and r.choices[0].finish_reason == "length"
            assert r.usage["completion_tokens"] == 6 and r.usage["total_tokens"] == r.usage["prompt_tokens"] + 6
        assert out[0].choices[0].message.content != out[0].choices[1].message.content
        eng.calls.clear()
        for n in (None, 1):                                   # one choice: the engine is not handed ``n`` at all
            one = c.complete_many("host-only:n", msgs, max_tokens=4, n=n)
            assert len(one) == 5 and all(len(r.choices) == 1 and r.usage["completion_tokens"] == 2 for r in one)
        assert [(b, n) for b, n, _ in eng.calls] == [(4, None), (1, None)] * 2
        with pytest.raises(ValueError):
            c.complete_many("host-only:n", msgs, n=5)         # more choices than the engine has slots
    finally:
        CL.unregister_model("host-only:n", "cpu")
