"""top_k / min_p / logit_bias on MI355X: vis_shape_f32 against shaping.reference_shape bit for bit (rank cut with ties,
both zeros, min_p thresholds, bias lists, allow rows, both select paths), its argument errors, repeatability and batch
invariance; then the engines' and the client's keywords on the tiny synthetic models."""
import itertools
import json
import math

import numpy as np
import pytest
import torch

from test_sampling_gpu import _mllama, _msgs, _qwen_engine, _qwen_reqs
from vision_inspection_system_amd import hip
from vision_inspection_system_amd.shaping import MAX_BIAS, ShapeBuffers, min_p_delta, reference_shape

pytestmark = pytest.mark.gpu
POISON = 0x7FC12345            # a NaN pattern no kernel writes


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


# ----------------------------------------------------------------------------- inputs
def _row(kind: int, V: int, rng) -> np.ndarray:
    """0: normal logits; 1: quantised to eight values (the k-th place falls inside a tie run); 2: all equal; 3: both zeros
    among a few other values."""
    if kind == 0:
        return rng.normal(0, 3, V).astype(np.float32)
    if kind == 1:
        return (rng.integers(0, 8, V) * 0.5 - 2.0).astype(np.float32)
    if kind == 2:
        return np.full(V, 1.25, dtype=np.float32)
    return rng.choice(np.array([-0.0, 0.0, 1.0, -1.0, 0.5], dtype=np.float32), V)


def _bias(n: int, V: int, rng) -> list:
    """n (id, value) pairs: ids 0 and V - 1 and the values +-100 among them; past V distinct ids, ids outside the vocabulary
    (the kernel skips them)."""
    if n == 0:
        return []
    if n == 1:
        return [(V - 1, 100.0)]
    base = [0] + ([V - 1] if V > 1 else [])
    ids = (base + [i for i in rng.permutation(V).tolist() if i not in base])[:n]
    ids += [V + 5 * j for j in range(n - len(ids))]
    if ids[-1] >= V:
        ids[-1] = -3
    vals = rng.uniform(-100, 100, n).astype(np.float32).tolist()
    vals[0], vals[1] = 100.0, -100.0
    return list(zip(ids, vals))


def _allow_bits(kind: int, V: int, rng) -> np.ndarray:
    """0: every id; 1: a random half; 2: one id; 3: none; 4: only ids of the last (ragged) 64-bit word."""
    a = np.zeros(V, dtype=bool)
    if kind == 0:
        a[:] = True
    elif kind == 1:
        a[:] = rng.random(V) < 0.5
    elif kind == 2:
        a[int(rng.integers(0, V))] = True
    elif kind == 4:
        a[(V - 1) // 64 * 64:] = True
    return a


def _pack(bits: np.ndarray) -> torch.Tensor:
    B, V = bits.shape
    nw = (V + 63) // 64
    full = np.zeros((B, nw * 64), dtype=bool)
    full[:, :V] = bits
    return torch.from_numpy(np.packbits(full.reshape(B, -1, 8), axis=2, bitorder="little").reshape(B, -1)
                            .view("<u8").view(np.int64).copy()).cuda()


def _launch(x: np.ndarray, ks, deltas, biases, allow=None, out=None):
    """One vis_shape_f32 launch over the rows of x [B, V] -> (out as int32 [B, V], nkept [B], records [B, 4] int32)."""
    B, V = x.shape
    xd = torch.from_numpy(x).cuda()
    bid = np.zeros((B, MAX_BIAS), dtype=np.int32)
    bval = np.zeros((B, MAX_BIAS), dtype=np.float32)
    for b, lst in enumerate(biases):
        for j, (i, v) in enumerate(lst):
            bid[b, j], bval[b, j] = i, v
    out = torch.full((B, V), POISON, dtype=torch.int32, device="cuda").view(torch.float32) if out is None else out
    nkept = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = hip.shape_ws(V, B, "cuda")
    hip.shape_logits(xd if B > 1 else xd[0], torch.tensor(ks, dtype=torch.int32).cuda(),
                     torch.tensor(deltas, dtype=torch.float32).cuda(),
                     torch.tensor([len(b) for b in biases], dtype=torch.int32).cuda(), torch.from_numpy(bid).cuda(),
                     torch.from_numpy(bval).cuda(), out if B > 1 else out[0], nkept, ws,
                     allow=None if allow is None else _pack(allow))
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu().numpy(), nkept.cpu().numpy(), ws.cpu().numpy().view(np.int32).reshape(B, 4)


def _check(x, ks, deltas, biases, allow, what):
    got, nk, rec = _launch(x, ks, deltas, biases, allow)
    for b in range(x.shape[0]):
        ref = reference_shape(x[b], ks[b], deltas[b], biases[b], None if allow is None else allow[b])
        bad = np.flatnonzero(got[b] != ref.out.view(np.int32))
        assert bad.size == 0, (what, b, ks[b], deltas[b], len(biases[b]), bad[:5], got[b][bad[:5]], ref.out.view(np.int32)[bad[:5]])
        assert nk[b] == ref.nkept, (what, b, ks[b], deltas[b], nk[b], ref.nkept)
    return rec


MINP = [(0.0, 1.0), (0.05, 0.5), (0.05, 2.0), (1.0, 0.5), (1.0, 2.0)]     # (min_p, temperature)


@pytest.mark.parametrize("V", [1, 63, 320, 1000, 4097])
def test_kernel_matches_reference_bit_for_bit(V):
    """Every combination of k, min_p / temperature, bias count and allow row, one combination per row (the parameters are
    per row), over the four kinds of rows; launches of 64, 3 and 1 rows."""
    rng = np.random.default_rng(V)
    ks = sorted({0, 1, 2, 40, V - 1, V})
    combos = list(itertools.product(ks, MINP, (0, 1, MAX_BIAS)))
    paths = set()
    for with_allow in (False, True):
        rows = [(k, mp, nb, ak) for (k, mp, nb) in combos for ak in ((0, 1, 2, 3, 4) if with_allow else (0,))]
        sizes = itertools.chain((1, 3), itertools.repeat(64))
        i = 0
        while i < len(rows):
            chunk = rows[i:i + next(sizes)]
            x = np.stack([_row((i + j) % 4, V, rng) for j in range(len(chunk))])
            allow = np.stack([_allow_bits(c[3], V, rng) for c in chunk]) if with_allow else None
            rec = _check(x, [c[0] for c in chunk], [min_p_delta(*c[1]) for c in chunk], [_bias(c[2], V, rng) for c in chunk],
                         allow, (V, with_allow, i))
            paths |= set(rec[:, 3].tolist())
            i += len(chunk)
    if V == 4097:
        assert paths == {0, 1, 2}          # no rank cut, the cut by rank counting in LDS, the radix select (all-equal rows)


def test_kernel_full_vocabulary():
    """V = 152064 at 2 rows: normal logits (the cut is found among a bin's members in LDS) and logits on eight values (the
    k-th place inside a tie run of thousands: the radix select), k = 40, min_p = 0.05, 8 biases."""
    V = 152064
    rng = np.random.default_rng(7)
    x = np.stack([_row(0, V, rng), _row(1, V, rng)])
    bias = [(0, -100.0), (V - 1, 100.0)] + [(int(i), float(v)) for i, v in zip(rng.permutation(V)[:6] + 1, rng.uniform(-5, 5, 6))]
    rec = _check(x, [40, 40], [min_p_delta(0.05, 1.0)] * 2, [bias, bias[2:]], None, "full")
    assert rec[:, 3].tolist() == [1, 2] and rec[:, 2].tolist() == [V, V]
    allow = np.stack([_allow_bits(1, V, rng), _allow_bits(4, V, rng)])
    _check(x, [40, 2], [min_p_delta(0.05, 2.0), -math.inf], [bias, []], allow, "full, masked")


def test_argument_errors_launch_nothing():
    V, B = 320, 2
    lib = hip.load()
    x = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    out = torch.full((B, V), POISON, dtype=torch.int32, device="cuda")
    k = torch.ones(B, dtype=torch.int32, device="cuda")
    d = torch.zeros(B, dtype=torch.float32, device="cuda")
    nb = torch.zeros(B, dtype=torch.int32, device="cuda")
    bi = torch.zeros((B, MAX_BIAS), dtype=torch.int32, device="cuda")
    bv = torch.zeros((B, MAX_BIAS), dtype=torch.float32, device="cuda")
    nk = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = hip.shape_ws(V, B, "cuda")
    allow = torch.full((B, 5), -1, dtype=torch.int64, device="cuda")
    good = dict(logits=x.data_ptr(), V=V, ld=V, allow=allow.data_ptr(), ld_allow=5, k=k.data_ptr(), d=d.data_ptr(),
                nb=nb.data_ptr(), bi=bi.data_ptr(), bv=bv.data_ptr(), out=out.data_ptr(), ld_out=V, nk=nk.data_ptr(),
                ws=ws.data_ptr(), B=B)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vis_shape_f32(a["logits"], a["V"], a["ld"], a["allow"], a["ld_allow"], a["k"], a["d"], a["nb"], a["bi"], a["bv"],
                                 a["out"], a["ld_out"], a["nk"], a["ws"], a["B"], torch.cuda.current_stream().cuda_stream)

    bad = [dict(logits=None), dict(k=None), dict(d=None), dict(nb=None), dict(bi=None), dict(bv=None), dict(out=None),
           dict(nk=None), dict(ws=None), dict(V=0), dict(V=262145), dict(B=0), dict(B=65), dict(ld=V - 1), dict(ld_out=V - 1),
           dict(ld_allow=4), dict(allow=allow.data_ptr() + 4), dict(out=x.data_ptr()), dict(logits=x.data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((nk == -7).all())
    assert lib.vis_shape_ws_bytes(0, 1) == 0 and lib.vis_shape_ws_bytes(V, 65) == 0 and lib.vis_shape_ws_bytes(262145, 1) == 0
    assert call() == 0 and call(allow=None, ld_allow=0) == 0
    torch.cuda.synchronize()
    assert not bool((out == POISON).any())


def test_repeated_launch_and_batch_invariance():
    """A launch repeated on the same inputs rewrites the same bytes; a row's result is the same alone and as row 63 of 64."""
    V = 4097
    rng = np.random.default_rng(3)
    x = np.stack([_row(j % 4, V, rng) for j in range(64)])
    ks = [40] * 64
    deltas = [min_p_delta(0.05, 2.0)] * 64
    biases = [_bias(MAX_BIAS, V, rng) for _ in range(64)]
    allow = np.stack([_allow_bits(1, V, rng) for _ in range(64)])
    out = torch.full((64, V), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    first, nk1, _ = _launch(x, ks, deltas, biases, allow, out=out)
    again, nk2, _ = _launch(x, ks, deltas, biases, allow, out=out)
    assert np.array_equal(first, again) and np.array_equal(nk1, nk2)
    for r in (63, 62, 61, 60):                       # one row of each kind
        alone, nk, _ = _launch(x[r:r + 1], ks[r:r + 1], deltas[r:r + 1], biases[r:r + 1], allow[r:r + 1])
        assert np.array_equal(alone[0], first[r]) and nk[0] == nk1[r]


# ----------------------------------------------------------------------------- engines
def _record_nkept(monkeypatch):
    """ShapeBuffers.apply wrapped to keep the survivor counts of every launch."""
    seen, orig = [], ShapeBuffers.apply

    def apply(self, logits, slot=0, allow=None):
        out = orig(self, logits, slot, allow)
        B = logits.shape[0] if logits.dim() == 2 else 1
        seen.append(self.nkept[slot:slot + B].clone())
        return out
    monkeypatch.setattr(ShapeBuffers, "apply", apply)
    return seen, orig


def _engine_checks(eng, a, b, monkeypatch, kw, single_is_batch_exact: bool, parse):
    greedy = eng.generate(*a, **kw)
    # top_k = 1 at a high temperature is the greedy reply, with one survivor at every step (a tie would keep more and make
    # the comparison vacuous)
    seen, orig = _record_nkept(monkeypatch)
    assert eng.generate(*a, temperature=1.5, seed=3, top_k=1, use_graph=False, **kw) == greedy
    assert len(seen) == len(greedy) and all(int(n) == 1 for t in seen for n in t)
    monkeypatch.setattr(ShapeBuffers, "apply", orig)
    assert eng.generate(*a, temperature=1.5, seed=3, top_k=1, **kw) == greedy          # graph replay
    assert eng.shape_on is False and eng._shape_key() == (False,)
    # logit_bias: -100 bans the greedy first token, +100 forces another
    other = (greedy[0] + 7) % 200
    assert eng.generate(*a, logit_bias={greedy[0]: -100}, **kw)[0] != greedy[0]
    assert eng.generate(*a, logit_bias={str(other): 100}, **kw)[0] == other
    assert eng.generate(*a, **kw) == greedy                                             # off again
    # a seeded request with top_k and min_p: the same tokens alone and in a batch of three whose other members differ
    skw = dict(kw, temperature=1.0)
    for jm in (False, True):
        jkw = dict(skw, json_mode=True) if jm else skw
        if jm:
            jkw.pop("ignore_eos", None), jkw.pop("stop_on_eos", None)
        alone = eng.generate_batch([a], seeds=[5], top_k=40, min_p=0.05, **jkw)[0]
        three = eng.generate_batch([a, b, a], seeds=[5, 9, 11], top_k=[40, 3, None], min_p=[0.05, None, 0.5],
                                   logit_bias=[None, {other: 5.0}, None], **jkw)
        moved = eng.generate_batch([b, b, a], seeds=[1, 2, 5], top_k=[None, 1, 40], min_p=[0.9, None, 0.05], **jkw)
        assert three[0] == moved[2], jm
        print(f"alone vs in a batch of three (json_mode={jm}): {alone == three[0]}; first token {alone[:1] == three[0][:1]}")
        if single_is_batch_exact:
            assert alone == three[0], jm
        else:
            assert alone[:1] == three[0][:1], jm
        if jm:
            for t in (alone, three[0], three[1], three[2]):
                parse(t)


def test_qwen_engine(device, monkeypatch):
    """alone == in a batch of three, token for token: with VIS_ROWS_GEMV=3 the batched step is the single-sequence
    arithmetic (every sequence bit-identical to decoding alone), so nothing but the shaping parameters could differ."""
    from test_json_mode_gpu import _replay
    monkeypatch.setenv("VIS_ROWS_GEMV", "3")
    cfg, eng = _qwen_engine(device, max_batch=4)
    a, b = _qwen_reqs(device)
    _engine_checks(eng, a, b, monkeypatch, dict(max_new_tokens=24, ignore_eos=True), True,
                   lambda t: _replay(eng._json.table, t, set(cfg.eos_ids), "qwen"))


def test_mllama_engine(device, monkeypatch):
    """The batched step of this engine is not the single-sequence arithmetic (the existing sampling tests compare the first
    token only), so alone and in-batch agree on the prompt pass's pick, and the full reply is compared between two batches
    of three that hold the request in different slots next to members with other settings."""
    from test_json_mode_gpu import _replay
    eng, a, b = _mllama(device)
    _engine_checks(eng, a, b, monkeypatch, dict(max_new_tokens=24, stop_on_eos=False), False,
                   lambda t: _replay(eng._json.table, t, set(eng.cfg.eos_ids), "mllama"))


@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_accepts_the_three_parameters(device, tmp_path, model):
    from vision_inspection_system_amd.client import LocalVLMClient
    c = LocalVLMClient()
    m = _msgs(tmp_path, 1)
    greedy = c.chat.completions.create(model=model, messages=m, temperature=0.0, max_tokens=16)
    r = c.chat.completions.create(model=model, messages=m, temperature=1.5, seed=3, max_tokens=16, top_k=1)
    assert r.choices[0].message.content == greedy.choices[0].message.content
    r = c.chat.completions.create(model=model, messages=m, temperature=1.0, seed=3, max_tokens=16, top_k=40, min_p=0.05,
                                  logit_bias={"65": -100, 66: 2.5})
    assert r.usage["completion_tokens"] >= 1
    many = c.complete_many(model, [m, m], temperature=1.0, max_tokens=16, seed=3, top_k=40, min_p=0.05)
    assert many[0].choices[0].message.content == many[1].choices[0].message.content
    with pytest.raises(ValueError):
        c.chat.completions.create(model=model, messages=m, max_tokens=4, top_k=0)
    with pytest.raises(ValueError):
        c.chat.completions.create(model=model, messages=m, max_tokens=4, logit_bias={"1": 101})
    r = c.chat.completions.create(model=model, messages=m, temperature=0.7, seed=3, max_tokens=24, min_p=0.1,
                                  response_format={"type": "json_object"})
    if r.choices[0].finish_reason == "stop":
        assert isinstance(json.loads(r.choices[0].message.content), dict)
