"""Speculative decoding under a JSON Schema on the GPU (spec.py "grammar").  The kernels: vis_schema_mask_rows against
vis_schema_mask run alone on the history with the drafts appended (word for word), vis_spec_accept_masked against
vis_argmax_masked_f32 (bit for bit) and spec.accept_ref_sampled, vis_spec_draft_schema against schema_draft.propose.  The
engines and the client: generate(json_schema=dfa, speculative={k, grammar}) returns the plain schema-constrained reply token
for token, fails where it fails, and reports the counters of schema_draft.simulate."""
import itertools
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import spec_sampled_cases as C
from schema_cases import Closed, Flat, Nested, distance_to_accept, random_walk
from test_json_mode_gpu import _Vocab, _dev_table
from test_json_schema_gpu import CLOSED_MAX, _Dev
from vision_inspection_system_amd import json_grammar as G
from vision_inspection_system_amd import json_schema as S
from vision_inspection_system_amd import schema_draft as D
from vision_inspection_system_amd.schemas import REPORT_SCHEMA

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMAS = {"flat": Flat.model_json_schema(), "nested": Nested.model_json_schema(), "report": REPORT_SCHEMA,
           "closed": Closed.model_json_schema()}
T = 256
REC = 32


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


@pytest.fixture(scope="module")
def dfas():
    return {k: S.compile_schema(v) for k, v in SCHEMAS.items()}


_VOCABS: dict = {}


def _vocab(V):
    """A synthetic vocabulary of V ids (V = 200: 4 words, the last one ragged; 1000: ragged too, multi-byte tokens), on the device."""
    if V not in _VOCABS:
        table = G.build_token_table(_Vocab(V, seed=11), V, [V - 3, V - 1])
        _VOCABS[V] = (table, _dev_table(table))
    return _VOCABS[V]


@pytest.fixture(params=[200, 1000])
def vocab(request, device):
    return _vocab(request.param)


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64), dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------- rows mask
def _single(histories, table, dt, dev):
    """vis_schema_mask alone: one row per history (token ids), folded from the start state.  Returns int64 [B, nw]."""
    from vision_inspection_system_amd import hip
    B, nw = len(histories), (table.vocab + 63) // 64
    tokens = torch.zeros((B, T), dtype=torch.int32)
    state = torch.zeros((B, S.STATE_INTS), dtype=torch.int32)
    step = torch.zeros(B, dtype=torch.int32)
    for r, h in enumerate(histories):
        tokens[r, :len(h)] = torch.tensor(list(h), dtype=torch.int32)
        step[r] = len(h)
        state[r, (len(h) & 1) * S.SLOT_INTS + S.ANCHOR] = 1
        state[r, (len(h) & 1) * S.SLOT_INTS + S.STATE] = dev.header[2].item()
    allow = torch.zeros((B, nw), dtype=torch.int64, device="cuda")
    hip.schema_mask(state.cuda(), tokens.cuda(), step.cuda(), *dt, allow, *dev.args())
    return allow


class _Rows:
    """One sequence's record and buffers of vis_schema_mask_rows."""

    def __init__(self, table, dt, dev, history, record=None):
        self.table, self.dt, self.dev = table, dt, dev
        self.nw = (table.vocab + 63) // 64
        self.record = _i32(record if record is not None else [0] * REC)
        self.tokens = _i32(list(history) + [0] * (T - len(history)))
        self.step = _i32([len(history)])

    def launch(self, R, draft, n_draft):
        from vision_inspection_system_amd import hip
        allow = torch.full((R, self.nw + 3), -1, dtype=torch.int64, device="cuda")
        d = _i32(list(draft) + [0] * (3 - len(draft)))
        hip.schema_mask_rows(self.record, self.tokens, self.step, d, _i32([n_draft]), *self.dt, allow, *self.dev.args())
        torch.cuda.synchronize()
        assert (allow[:, self.nw:] == -1).all(), "wrote past a row's words"
        rec = self.record.cpu().tolist()
        assert rec[4:] == [0] * (REC - 4), "counters left behind"
        return allow[:, :self.nw].contiguous(), rec[:4]


def _live_rows(dfa, table, history, draft, n_draft, R):
    """How many rows the definition keeps: row r needs r <= n_draft (clamped) and every draft in front of it in range, no EOS
    id, and accepted by the walk from the state in front of it."""
    st = S.initial_state(dfa)
    for t in history:
        S.advance(dfa, st, t, table)
    live, d = 1, min(max(n_draft, 0), R - 1)
    for r in range(1, R):
        t = draft[r - 1] if r - 1 < len(draft) else 0
        if r > d or st[1] or not 0 <= t < table.vocab or table.flags[t] & G.FLAG_EOS:
            break
        S.advance(dfa, st, t, table)
        if st[1]:
            break
        live += 1
    return live


def _check_rows(dfa, table, dt, dev, history, draft, n_draft, R, record=None):
    rows = _Rows(table, dt, dev, history, record)
    got, rec = rows.launch(R, draft, n_draft)
    live = _live_rows(dfa, table, history, draft, n_draft, R)
    want = _single([list(history) + [int(t) for t in draft[:r]] for r in range(live)], table, dt, dev)
    assert torch.equal(got[:live], want), (history, draft, n_draft, R)
    assert (got[live:] == 0).all(), (history, draft, n_draft, R, live)
    again, rec2 = rows.launch(R, draft, n_draft)      # the same launch twice: the same words and record
    assert torch.equal(again, got) and rec2 == rec
    st = S.initial_state(dfa)
    for t in history:
        S.advance(dfa, st, t, table)
    assert rec == [st[0], st[1], len(history), 1]
    return live


def _allowed_draft(dfa, table, state, rng, want_long=True):
    ok, err = S.allowed(dfa, [state, 0], table)
    ids = [int(t) for t in np.flatnonzero(ok) if not table.flags[t] & G.FLAG_EOS]
    if err or not ids:
        return None
    longest = max(len(table.tokens[t]) for t in ids)
    pool = [t for t in ids if len(table.tokens[t]) == longest] if want_long and rng.random() < 0.5 else ids
    return rng.choice(pool)


def _rejected_draft(dfa, table, state):
    ok, _ = S.allowed(dfa, [state, 0], table)
    return next(t for t in range(table.vocab) if not ok[t] and table.tokens[t] and not table.flags[t] & G.FLAG_EOS)


def _histories(dfa, table, rng, n):
    """Token histories (single-byte tokens inside the vocabulary) that reach varied states, the empty one first."""
    out, dist = [[]], distance_to_accept(dfa)
    while len(out) < n:
        doc, _ = random_walk(dfa, rng, dist, wander=0)
        doc = doc[:rng.randint(1, min(len(doc) - 1, 120))]
        if all(b < table.vocab - 3 and table.tokens[b] == bytes([b]) for b in doc):
            out.append(list(doc))
    return out


@pytest.mark.parametrize("V,name", [(200, "closed"), (1000, "closed"), (1000, "report")])
def test_rows_equal_the_single_mask_on_the_drafted_history(device, dfas, V, name):
    """V = 200 has no bytes for the report's strings: 'closed' covers it."""
    table, dt = _vocab(V)
    dfa = dfas[name]
    dev = _Dev().load(dfa)
    rng = random.Random(table.vocab)
    multi = 0
    for history in _histories(dfa, table, rng, 5):
        s = S.walk(dfa, dfa.start, bytes(history))
        good, st = [], s
        for _ in range(3):      # a chain of allowed drafts, multi-byte where the vocabulary has one
            t = _allowed_draft(dfa, table, st, rng)
            if t is None:
                break
            good.append(t)
            st = S.walk(dfa, st, table.tokens[t])
        multi += sum(len(table.tokens[t]) > 1 for t in good)
        for R in (1, 2, 3, 4):
            assert _check_rows(dfa, table, dt, dev, history, good, len(good), R) == min(R, len(good) + 1)
            for n_draft in (0, 1, R - 2, 7, -3):      # none, fewer than R - 1, more than the rows hold, negative
                _check_rows(dfa, table, dt, dev, history, good, n_draft, R)
        for at in range(min(3, len(good))):      # a rejected draft at r = 0 / 1 / 2: all-zero rows behind it
            st = s
            for t in good[:at]:
                st = S.walk(dfa, st, table.tokens[t])
            bad = good[:at] + [_rejected_draft(dfa, table, st)] + good[at + 1:]
            assert _check_rows(dfa, table, dt, dev, history, bad, 3, 4) == at + 1
            for other in (int(table.eos_ids[0]), -1, table.vocab, 2 ** 30):      # an EOS draft, out-of-range drafts
                assert _check_rows(dfa, table, dt, dev, history, good[:at] + [other] + good[at + 1:], 3, 4) == at + 1
    assert multi > 0 or table.vocab == 200
    # the accepting state: row 0 allows the EOS ids only, and an EOS draft ends the chain
    doc, end = random_walk(dfa, rng, distance_to_accept(dfa), wander=0)
    if all(b < table.vocab - 3 for b in doc) and len(doc) < T - 8:
        assert dfa.state_flags[end] & S.STATE_ACCEPT
        assert _check_rows(dfa, table, dt, dev, list(doc), [int(table.eos_ids[0]), 5, 6], 3, 4) == 1


def test_rows_fold_whatever_the_step_advanced_by(vocab, dfas):
    """step advances by every amount 1..4 between launches (and by 0): the record equals json_schema.advance over the tokens in
    front of it, row 0 the single mask's row there; only picked tokens are folded, never a draft."""
    table, dt = vocab
    dfa = dfas["closed"]
    dev = _Dev().load(dfa)
    rng = random.Random(5)
    doc, _ = random_walk(dfa, rng, distance_to_accept(dfa), wander=0)
    ids = list(doc) + [int(table.eos_ids[0])] * 3      # past the document's end: EOS in the accepting state changes nothing
    rows = _Rows(table, dt, dev, ids)
    at, st, folded = 0, S.initial_state(dfa), 0
    incs = itertools.cycle((0, 1, 2, 3, 4, 0, 4, 3, 2, 1))
    while at < len(ids):
        inc = next(incs)
        at = min(at + inc, len(ids))
        rows.step.fill_(at)
        bogus = [rng.randrange(table.vocab - 3) for _ in range(3)]      # drafts of any kind never reach the record
        got, rec = rows.launch(4, bogus, 3)
        for t in ids[folded:at]:
            S.advance(dfa, st, t, table)
        folded = at
        assert rec == [st[0], st[1], at, 1], (at, inc)
        assert torch.equal(got[:1], _single([ids[:at]], table, dt, dev)), at
    assert at == len(ids) and not st[1]
    # an anchored record in the middle: the fold starts at its position, in its state
    mid = len(doc) // 2
    rec = [S.walk(dfa, dfa.start, bytes(doc[:mid])), 0, mid, 1] + [0] * (REC - 4)
    _check_rows(dfa, table, dt, dev, list(doc[:mid + 3]), [], 0, 2, record=rec)
    # a token the DFA rejects sets the error bit only: EOS ids in row 0, nothing behind it
    wrong = list(doc[:4]) + [_rejected_draft(dfa, table, S.walk(dfa, dfa.start, bytes(doc[:4])))]
    got, rec = _Rows(table, dt, dev, wrong).launch(3, [ids[5], ids[6]], 2)
    eos_only = torch.from_numpy(G.mask_words(np.isin(np.arange(table.vocab), table.eos_ids))).cuda()
    assert rec[1] == 1 and torch.equal(got[0], eos_only) and (got[1:] == 0).all()


def test_rows_table_through_l2_and_bad_header(device):
    table, dt = _vocab(1000)
    keys = {f"property_{i:02d}": {"enum": ["alpha", "beta", "gamma"]} for i in range(40)}
    dfa = S.compile_schema({"type": "object", "properties": keys, "required": list(keys)[::3]})
    assert dfa.trans.nbytes > 72 * 1024      # too large for the LDS staging: read through L2
    dev = _Dev().load(dfa)
    rng = random.Random(3)
    for history in _histories(dfa, table, rng, 3):
        st, good = S.walk(dfa, dfa.start, bytes(history)), []
        for _ in range(3):
            good.append(_allowed_draft(dfa, table, st, rng))
            st = S.walk(dfa, st, table.tokens[good[-1]])
        assert _check_rows(dfa, table, dt, dev, history, good, 3, 4) == 4
        assert _check_rows(dfa, table, dt, dev, history, [good[0], _rejected_draft(dfa, table, S.walk(
            dfa, S.walk(dfa, dfa.start, bytes(history)), table.tokens[good[0]])), good[2]], 3, 4) == 2
    # a header outside the capacities: the error state - EOS ids in row 0, nothing behind it, nothing indexed
    small = S.compile_schema(SCHEMAS["flat"])
    dev = _Dev(cap_states=(small.n_states + 7) & ~7, cap_classes=small.n_classes).load(small)
    eos_only = torch.from_numpy(G.mask_words(np.isin(np.arange(table.vocab), table.eos_ids))).cuda()
    for bad in ([small.n_states + 8, small.n_classes, small.start, 0], [small.n_states, small.n_classes + 1, small.start, 0],
                [small.n_states, small.n_classes, small.n_states, 0], [0, 0, 0, 0], [-1, -1, -1, 0]):
        dev.header.copy_(torch.tensor(bad, dtype=torch.int32))
        got, rec = _Rows(table, dt, dev, [ord("{")]).launch(4, [ord('"'), ord("n"), ord("a")], 3)
        assert torch.equal(got[0], eos_only) and (got[1:] == 0).all() and rec[1] == 1, bad
        assert torch.equal(got[:1], _single([[ord("{")]], table, dt, dev))


def test_rows_under_a_captured_graph_follow_the_schema_buffers(vocab, dfas):
    from vision_inspection_system_amd import hip
    table, dt = vocab
    dev = _Dev().load(dfas["closed"])
    history = [ord("{"), ord('"')]
    rows = _Rows(table, dt, dev, history)
    allow = torch.zeros((3, rows.nw), dtype=torch.int64, device="cuda")
    draft, n_draft = _i32([ord("a"), ord('"'), 0]), _i32([2])

    def launch():
        hip.schema_mask_rows(rows.record, rows.tokens, rows.step, draft, n_draft, *dt, allow, *dev.args())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for name, d in (("closed", [ord("a"), ord('"')]), ("flat", [ord("n"), ord("a")]), ("closed", [ord("a"), ord('"')])):
        dev.load(dfas[name])
        rows.record.zero_()
        draft[:2] = _i32(d)
        g.replay()
        torch.cuda.synchronize()
        want = _single([history, history + d[:1], history + d], table, dt, dev)
        assert torch.equal(allow, want), name
        assert (want != 0).any(dim=1).all()


# --------------------------------------------------------------------------------------------------- masked accept
T_ROW = 1100


def _masked_token(hip, row, st, inv_temp, seed, allow_row):
    """What vis_argmax_masked_f32 (batch 1) stores for ``row`` at step ``st`` under ``allow_row``."""
    tokens, cur, step = _i32([-1] * T_ROW), _i32([-1]), _i32([st])
    ws_val, ws_idx = torch.empty(256, dtype=torch.float32, device="cuda"), torch.empty(256, dtype=torch.int32, device="cuda")
    rc = hip.load().vis_argmax_masked_f32(row.data_ptr(), row.numel(), ws_val.data_ptr(), ws_idx.data_ptr(), tokens.data_ptr(),
                                          T_ROW, cur.data_ptr(), step.data_ptr(), float(inv_temp), seed, 1, row.numel(),
                                          allow_row.data_ptr(), allow_row.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return int(tokens[st].item())


def _accept(hip, logits, st, draft, d, limit, allow, params, counters=(5, 7, 3)):
    R = logits.shape[0]
    tokens0 = np.arange(2000, 2000 + T_ROW, dtype=np.int32)
    tokens, cur, step, cnt = _i32(tokens0), _i32([-1]), _i32([st]), _i32(list(counters))
    hip.spec_accept_masked(logits, _i32(list(draft) + [0] * (3 - len(draft))), _i32([len(draft) if d is None else d]),
                           _i32([limit]), torch.empty(256 * R, dtype=torch.float32, device="cuda"),
                           torch.empty(256 * R, dtype=torch.int32, device="cuda"), tokens, cur, step, cnt, allow, params)
    return tokens.cpu().numpy(), int(cur.item()), int(step.item()), cnt.cpu().tolist(), tokens0


@pytest.mark.parametrize("V", [1000, 4099])
def test_masked_picks_equal_vis_argmax_masked_bit_for_bit(device, V):
    """Greedy (params None, and inv_temp 0) and sampled at steps 0 / 5 / 1000 with 1 / T of 0.5 / 10: every row's pick is the
    token vis_argmax_masked_f32 stores for that row at step + r.  Rows: a random tenth of the ids, ONE allowed id, none, all."""
    from vision_inspection_system_amd import hip, spec
    rng = np.random.default_rng(V)
    logits = torch.tensor(C.diff_rows(V)).to(device)      # a planted tie, all NaN, two Gaussians
    nw = (V + 63) // 64
    bits = rng.random((4, nw * 64)) < 0.1
    bits[:, V:] = False
    bits[3] = False
    bits[3, V - 1] = True                                  # one allowed id, in the ragged last word
    bits[2] = False                                        # none: picks 0
    masks = {"mixed": bits.copy()}
    bits[:, :V] = True
    masks["all"] = bits
    for kind, b in masks.items():
        allow = torch.from_numpy(np.stack([G.mask_words(r[:nw * 64]) for r in b])).to(device)
        for inv_temp, seed in ((None, 0), (0.0, 3), (0.5, 0), (0.5, 0xFFFFFFFF), (10.0, 12345)):
            params = None if inv_temp is None else torch.from_numpy(C.params_words(inv_temp, seed)).to(device)
            for st in (0, 5, 1000):
                ref = [_masked_token(hip, logits[r], st + r, inv_temp or 0.0, seed, allow[r]) for r in range(4)]
                if kind == "mixed":
                    assert ref[3] == V - 1 and ref[2] == 0
                for R in (1, 2, 4):
                    tok, cur, step, cnt, _ = _accept(hip, logits[:R], st, ref[:R - 1], None, T_ROW - 1, allow[:R], params)
                    assert tok[st:st + R].tolist() == ref[:R], (V, kind, inv_temp, seed, st, R)
                    assert (cur, step, cnt) == (ref[R - 1], st + R, [6, 7 + R - 1, 3 + R - 1])
    # tokens, cur, step and counters equal spec.accept_ref_sampled on those picks: wrong drafts, counts, the limit
    allow = torch.from_numpy(np.stack([G.mask_words(r[:nw * 64]) for r in masks["mixed"]])).to(device)
    params = torch.from_numpy(C.params_words(0.5, 7)).to(device)
    st = 5
    picks = [_masked_token(hip, logits[r], st + r, 0.5, 7, allow[r]) for r in range(4)]
    wrong = lambda i: (picks[i] + 1) % V      # noqa: E731
    for draft, d, limit in ((picks[:3], None, T_ROW - 1), ([wrong(0), picks[1], picks[2]], None, T_ROW - 1),
                            ([picks[0], wrong(1), picks[2]], None, T_ROW - 1), ([picks[0], picks[1], wrong(2)], None, T_ROW - 1),
                            (picks[:3], 0, T_ROW - 1), (picks[:3], 2, T_ROW - 1), (picks[:3], 9, T_ROW - 1), (picks[:3], -4, T_ROW - 1),
                            (picks[:3], None, st + 1), (picks[:3], None, st), (picks[:3], None, st - 1)):
        tok, cur, step, cnt, tokens0 = _accept(hip, logits, st, draft, d, limit, allow, params)
        want = spec.accept_ref_sampled(picks, draft, len(draft) if d is None else d, st, limit, tokens0, [5, 7, 3])
        assert np.array_equal(tok, want[0]), (draft, d, limit)
        assert (cur, step, cnt) == (-1 if want[1] is None else want[1], want[2], want[3]), (draft, d, limit)


def test_entries_refuse_bad_arguments(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    P = 4096
    ok = [P, 1000, 1000, 2, P, P, P, P, P, P, 64, P, P, P, None, P, 16, None]
    assert lib.vis_spec_accept_masked(*ok[:15], None, 16, None) == 1
    for at, bad in ((15, P + 4), (16, 15), (14, P + 2), (3, 5), (0, None)):
        args = list(ok)
        args[at] = bad
        assert lib.vis_spec_accept_masked(*args) == 1, (at, bad)
    rows = [P, P, 64, P, P, P, 2, P, P, P, P, 2, 1000, P, 16, P, P, P, P, 64, 64, None]
    for at, bad in ((6, 0), (6, 5), (14, 15), (0, None), (4, None), (16, P + 8), (19, 4097), (12, 0)):
        args = list(rows)
        args[at] = bad
        assert lib.vis_schema_mask_rows(*args) == 1, (at, bad)
    dr = [P, P, 64, P, P, P, P, 1000, P, P, P, P, 64, 64, P, P, 3, P, P, None]
    for at, bad in ((16, 0), (16, 4), (14, None), (15, None), (17, None), (12, 0), (7, 0)):
        args = list(dr)
        args[at] = bad
        assert lib.vis_spec_draft_schema(*args) == 1, (at, bad)


# ---------------------------------------------------------------------------------------------------------- drafter
def test_drafter_equals_propose(device, dfas):
    """vis_spec_draft_schema == schema_draft.propose from random reachable states, over a merged vocabulary and the report
    schema; it leaves the draft row alone when it has none; table entries outside their range draft nothing."""
    from vision_inspection_system_amd import hip
    V = 1000
    table = G.build_token_table(_Vocab(V, seed=11), V, [V - 3, V - 1])
    dt = _dev_table(table)
    some = none = 0
    for name in ("report", "closed"):
        dfa = dfas[name]
        dev = _Dev().load(dfa)
        tables = D.build(dfa, table)
        jt, jn = torch.from_numpy(tables.jump_tok).cuda(), torch.from_numpy(tables.jump_next).cuda()
        rng, dist = random.Random(len(name)), distance_to_accept(dfa)
        prefixes = [b"", b"{", b'{"']
        while len(prefixes) < 24:
            doc, _ = random_walk(dfa, rng, dist, wander=rng.choice([0, 100]))
            p = doc[:rng.randint(1, min(len(doc), T - 8))]
            if all(table.tokens[b] == bytes([b]) for b in p):
                prefixes.append(p)
        for p in prefixes:
            s = S.walk(dfa, dfa.start, p)
            for k in (1, 2, 3):
                want = D.propose(dfa, tables, s, k)
                tokens, step = _i32(list(p) + [0] * (T - len(p))), _i32([len(p)])
                draft, n_draft = _i32([7, 8, 9]), _i32([2])
                for record in ([0] * REC, [S.walk(dfa, dfa.start, p[:len(p) // 2]), 0, len(p) // 2, 1] + [0] * (REC - 4)):
                    rec = _i32(record)
                    hip.spec_draft_schema(rec, tokens, step, dt[0], dt[1], dt[2], *dev.args(), jt, jn, k, draft, n_draft)
                    assert rec.cpu().tolist() == record      # it only reads the record
                    if want:
                        assert n_draft.item() == len(want) and draft.cpu().tolist()[:len(want)] == want, (p, k)
                        assert draft.cpu().tolist()[len(want):] == [7, 8, 9][len(want):]
                        some += 1
                    else:      # what the drafter in front of it wrote stands
                        assert n_draft.item() == 2 and draft.cpu().tolist() == [7, 8, 9], (p, k)
                        none += 1
        # the error state drafts nothing; neither do table entries outside their range
        p = b'{"'
        tokens, step = _i32(list(p) + [0] * (T - len(p))), _i32([len(p)])
        assert D.propose(dfa, tables, S.walk(dfa, dfa.start, p), 3)
        for rec, tok, nxt in (([0, 1, 0, 0] + [0] * (REC - 4), jt, jn), ([0] * REC, torch.full_like(jt, V), jn),
                              ([0] * REC, torch.full_like(jt, -7), jn), ([0] * REC, jt, torch.full_like(jn, dfa.n_states)),
                              ([0] * REC, jt, torch.full_like(jn, -1))):
            draft, n_draft = _i32([7, 8, 9]), _i32([2])
            hip.spec_draft_schema(_i32(rec), tokens, step, dt[0], dt[1], dt[2], *dev.args(), tok, nxt, 3, draft, n_draft)
            assert n_draft.item() == 2 and draft.cpu().tolist() == [7, 8, 9]
    assert some > 20 and none > 5


# ---------------------------------------------------------------------------------------------------------- engines
sys.path.insert(0, os.path.join(HERE, "golden"))
N_NEW = CLOSED_MAX + 8


def _spec(k, **kw):
    return {"method": "ngram", "num_speculative_tokens": k, "grammar": True, **kw}


class _Eng:
    """One engine with a byte-level tokenizer behind one spelling: generate(**kw) on a fixed prompt."""

    def __init__(self, family, device, fmt, cross_kv="bf16"):
        import gen_decode_transcript as GT
        self.family = family
        if family == "mllama":
            from vision_inspection_system_amd.tokenizer import LlamaByteTokenizer
            cfg, self.e = GT._mllama(device, decode_weights=fmt, cross_kv=cross_kv, speculative=True)
            self.e.tokenizer = LlamaByteTokenizer(cfg.vocab, cfg.image_token_id, cfg.eos_ids)
            gm = np.load(os.path.join(HERE, "golden", "mllama_tiny.npz"))
            self.ids, self.frames = gm["a_ids"].tolist(), torch.from_numpy(gm["a_image"]).to(device)
            self.eos = lambda on: dict(stop_on_eos=on)
        else:
            cfg, self.e = GT._qwen(device, decode_weights=fmt)
            self.ids, self.frames = [256] + list(b'{"a":"x","b":true,"c":null} {"a":"y","b":false,"c":null}'), []
            self.eos = lambda on: dict(ignore_eos=not on)
        self.cfg = cfg

    def generate(self, n=N_NEW, stop_at_eos=True, **kw):
        return self.e.generate(self.ids, self.frames, max_new_tokens=n, **self.eos(stop_at_eos), **kw)


@pytest.fixture(scope="module", params=[("qwen", "bf16"), ("qwen", "fp8"), ("qwen", "mxfp4"), ("mllama", "bf16"),
                                        ("mllama", "fp8"), ("mllama", "mxfp4")], ids="-".join)
def eng(request, device):
    return _Eng(request.param[0], device, request.param[1])


def test_speculative_under_a_schema_equals_the_plain_reply(eng, dfas):
    """generate(json_schema=dfa, speculative={k, grammar}) == generate(json_schema=dfa): tokens and last_finish; k = 1 and 3,
    eager and replayed, greedy and sampled with a temperature and a seed, the mask alone, a prediction of the plain reply."""
    for name, n in (("closed", N_NEW), ("flat", 40)):
        dfa = dfas[name]
        for how in ({}, {"temperature": 0.8, "seed": 11}):
            plain = eng.generate(n, json_schema=dfa, **how)
            fin = eng.e.last_finish
            assert "spec_steps" not in eng.e.last_timing and plain
            if name == "closed":
                assert fin[0][0] == "eos"
                doc = bytes(t for t in plain if t not in eng.cfg.eos_ids)
                assert S.accepts(dfa, doc) and Closed.model_validate(json.loads(doc))
            for k in (1, 3):
                for graph in (False, True):
                    got = eng.generate(n, json_schema=dfa, use_graph=graph, speculative=_spec(k, sampled=bool(how)), **how)
                    assert got == plain and eng.e.last_finish == fin, (name, how, k, graph)
                    t = eng.e.last_timing
                    assert t["spec_steps"] >= 1 and 0 <= t["spec_accepted"] <= t["spec_proposed"] <= k * t["spec_steps"]
                    assert eng.e.schema_on is False
            mask_only = _spec(3, sampled=bool(how), schema_drafts=False)
            assert eng.generate(n, json_schema=dfa, speculative=mask_only, **how) == plain
            got = eng.generate(n, json_schema=dfa, speculative=mask_only, prediction=list(plain), **how)
            assert got == plain and eng.e.last_finish == fin and "pred_accepted" in eng.e.last_timing
            assert eng.generate(n, json_schema=dfa, **how) == plain      # nothing is left behind
    keys = list(eng.e._spec_graphs)
    assert any("grammar" in k and "schema_drafts" in k for k in keys) and any("grammar" in k and "schema_drafts" not in k for k in keys)
    # without the opt-in the request is refused as before; grammar without a schema, and the schema's drafts next to a prediction
    with pytest.raises(ValueError, match="together with json_schema is not supported"):
        eng.generate(json_schema=dfas["closed"], speculative=2)
    with pytest.raises(ValueError, match="'grammar' needs a JSON Schema"):
        eng.generate(speculative=_spec(2))
    with pytest.raises(ValueError, match="schema_drafts"):
        eng.generate(json_schema=dfas["closed"], speculative=_spec(2), prediction=[1, 2, 3])
    with pytest.raises(ValueError, match="together with json_mode is not supported"):
        eng.generate(json_mode=True, json_schema=dfas["closed"], speculative=_spec(2))
    # a speculative request without the schema is what it was
    plain = eng.generate(24, stop_at_eos=False)
    assert eng.generate(24, stop_at_eos=False, speculative=3) == plain
    assert not any("grammar" in k for k in eng.e._spec_graphs if k not in keys)


def test_counters_equal_the_model_free_walk(eng, dfas):
    """Byte-level vocabulary: spec_steps / spec_proposed / spec_accepted are schema_draft.simulate's on the plain reply, and
    the schema's forced bytes save steps."""
    names = ("spec_steps", "spec_proposed", "spec_accepted")
    for name, n in (("closed", 40), ("report", 60)):
        dfa = dfas[name]
        plain = eng.generate(n, stop_at_eos=False, json_schema=dfa)
        table = eng.e._schema.table
        tables = D.build(dfa, table)
        for k, graph in ((3, True), (1, False), (2, True)):
            for drafts in (True, False):
                sp = _spec(k, schema_drafts=drafts)
                got = eng.generate(n, stop_at_eos=False, json_schema=dfa, use_graph=graph, speculative=sp)
                assert got == plain, (name, k, graph, drafts)
                from vision_inspection_system_amd.spec import check_speculative
                sim = D.simulate(dfa, tables, table, plain, check_speculative(sp), prompt=eng.ids, max_new_tokens=n)
                assert {x: eng.e.last_timing[x] for x in names} == {x: sim[x] for x in names}, (name, k, graph, drafts)
                if drafts:
                    assert sim["spec_steps"] < len(plain) - 1 and sim["schema_proposed"] > 0 and sim["spec_accepted"] > 0


def test_failure_is_the_plain_requests_failure(device, dfas):
    """tests/test_json_schema_gpu.py::test_failure_is_reported's vocabulary (no '"'): JsonModeError, speculating or not."""
    from vision_inspection_system_amd.json_mode import JsonModeError
    e = _Eng("qwen", device, "bf16")

    class NoQuote:
        def token_bytes(self, t):
            return b"" if t == ord('"') or t > 255 else bytes([t])

    e.e.tokenizer = NoQuote()
    with pytest.raises(JsonModeError):
        e.generate(30, json_schema=dfas["flat"])
    for k, graph in ((1, False), (3, True)):
        with pytest.raises(JsonModeError):
            e.generate(30, json_schema=dfas["flat"], use_graph=graph, speculative=_spec(k))
        assert e.e.last_finish == [None]
    with pytest.raises(JsonModeError):      # run to the length limit: the forced EOS stands in the reply itself
        e.generate(12, stop_at_eos=False, json_schema=dfas["flat"], speculative=_spec(3))


def test_mllama_fp8_cross_keys(device, dfas):
    e = _Eng("mllama", device, "bf16", cross_kv="fp8")
    plain = e.generate(json_schema=dfas["closed"])
    for k in (1, 3):
        assert e.generate(json_schema=dfas["closed"], speculative=_spec(k)) == plain


# ----------------------------------------------------------------------------------------------------------- client
@pytest.mark.parametrize("model_id", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_create(device, monkeypatch, model_id):
    from vision_inspection_system_amd.client import LocalVLMClient
    if model_id.startswith("synthetic:mllama"):
        monkeypatch.setenv("VIS_AUDITOR_SPECULATIVE", "2")
    c = LocalVLMClient()
    msgs = [{"role": "user", "content": "Inspect: a x b true c null; a x b true c null"}]
    schema = Closed.model_json_schema()
    rf = {"type": "json_schema", "json_schema": {"name": "r", "schema": schema, "strict": True}}
    for kw, extra in ((dict(temperature=0.0), {}), (dict(temperature=0.7, seed=5), {"sampled": True})):
        plain = c.chat.completions.create(model=model_id, messages=msgs, max_tokens=N_NEW, response_format=rf, **kw)
        for k in (1, 2):
            sp = c.chat.completions.create(model=model_id, messages=msgs, max_tokens=N_NEW, response_format=rf,
                                           speculative=_spec(k, **extra), **kw)
            assert sp.choices[0].message.content == plain.choices[0].message.content
            assert sp.choices[0].finish_reason == plain.choices[0].finish_reason and sp.usage == plain.usage
            assert sp.timings["spec_steps"] >= 1
        obj = json.loads(plain.choices[0].message.content)
        assert S.validate(schema, obj) and Closed.model_validate(obj)
    with pytest.raises(ValueError, match="together with response_format is not supported"):
        c.chat.completions.create(model=model_id, messages=msgs, max_tokens=8, response_format=rf,
                                  speculative={"method": "ngram", "num_speculative_tokens": 2})
    with pytest.raises(ValueError, match="'grammar' needs a JSON Schema"):
        c.chat.completions.create(model=model_id, messages=msgs, max_tokens=8, speculative=_spec(2))


# -------------------------------------------------------------------------------------------------------- off state
def _step_names(device, cfg, dfa=None):
    """The library entries one eager speculative step calls, in order (the recorder of the decode transcript)."""
    import gen_decode_transcript as GT
    ids = [256] + list(b'{"a":"x"} {"a":"x"} {"a":')
    with GT.recording() as rec:
        _, e = GT._qwen(device)
        with e._pick_request(None, False, dfa, None, False, None):
            e.prefill(ids, [], max_new_tokens=20)
            e._spec_begin(cfg, 12)
            with rec.armed(e):
                e._decode_step_spec(cfg.rows)
            torch.cuda.synchronize(device)
        return [c.split("(")[0] for c in rec.calls], len(e.dec_layers)


def test_a_request_without_grammar_issues_the_launches_of_before(device, dfas):
    import gen_decode_transcript as GT
    from vision_inspection_system_amd.spec import SpecConfig
    rows = "vis_gemv_bf16_rows"
    names, layers = _step_names(device, SpecConfig(3, 4, 2))
    body = ["vis_gather_rows"] + [rows, "vis_decode_attn_draft", rows, rows, rows] * layers + [rows]
    assert names == body + ["vis_spec_accept", "vis_spec_draft"]
    assert _step_names(device, SpecConfig(3, 4, 2, True))[0] == body + ["vis_spec_accept_sampled", "vis_spec_draft"]
    tail = ["vis_schema_mask_rows", "vis_spec_accept_masked", "vis_spec_draft"]
    assert _step_names(device, SpecConfig(3, 4, 2, False, True), dfas["closed"])[0] == body + tail + ["vis_spec_draft_schema"]
    assert _step_names(device, SpecConfig(3, 4, 2, True, True, False), dfas["closed"])[0] == body + tail
    # the plain decode step: the recorded transcript, call for call
    with open(os.path.join(HERE, "golden", "decode_transcript.json")) as f:
        golden = json.load(f)["configs"]
    for name in ("qwen_single_bf16", "mllama_single"):
        got = GT.record(name, device)
        assert got["chained"] == golden[name]["chained"]
        assert not GT.first_difference(got["calls"], golden[name]["calls"]), name
