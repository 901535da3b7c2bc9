"""no_repeat_ngram_size / bad_words / min_tokens on the GPU: vis_ban_f32 against ban.ban_ref - the banned set exactly, every
other entry bit for bit, the input and everything outside the batch's rows untouched - the launcher's refusals, and both
engines end to end: every pick of a reply is the argmax of the raw row with ban_ref's ids taken out, min_tokens holds EOS
back for exactly that many tokens, a banned word changes the reply where it stood and never shows again."""
import ctypes

import numpy as np
import pytest
import torch

from test_sampling_gpu import _mllama, _msgs, _qwen_engine, _qwen_reqs
from vision_inspection_system_amd import hip
from vision_inspection_system_amd.ban import BanBuffers, ban_ref

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC0BEEF            # a NaN pattern no copy and no ban writes
V, T, PL = 1031, 320, 16         # odd: no multiple of a wave or of a vector width; token row; prompt row
# ids the histories are drawn from: both ends of the vocabulary, both sides of the seam between the row's two workgroups
# (ids 515 | 516) and of a vector (1027 | 1028), and one id outside the vocabulary (mllama's image token is id V)
ALPHABET = [0, 1, 515, 516, 1027, 1028, V - 1, V]
EOS = [1029, 2, 600]


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


def _rows(vocab=V, alphabet=ALPHABET):
    """64 row specs (n, prompt, generated, min_tokens, gen0): off / n = 1 / 2 / 3, prompts of 0 and 5 ids, L in {0, n-1, n,
    n+1, 300, 40, 12} where the prompt allows it, min_tokens off / one above the generated count / equal to it."""
    rng = np.random.default_rng(11)
    rows = []
    for i in range(64):
        n = i % 4
        P = (0, 5)[(i // 4) % 2]
        L = (0, n - 1, n, n + 1, 300, 40, 12, 300)[i // 8]
        G = max(L - P, 0)
        prompt = [alphabet[j] for j in rng.integers(0, len(alphabet), P)]
        gen = [alphabet[j] for j in rng.integers(0, len(alphabet), G)]
        if G >= 2 * n and n >= 2 and i % 8 >= 4:        # the tail copies an earlier n - 1 ids: an n-gram match for certain
            gen[G - n + 1:] = gen[0:n - 1]
        rows.append([n, prompt, gen, (0, G + 1, G)[i % 3], (i * 3) % 7])
    # the words' rows: a match that starts in the prompt and ends in the reply, one wholly inside the prompt, an empty history
    rows[60] = [0, [7, 11, 12, 13, 14], [21, 22, 23], 0, 2]
    rows[61] = [2, [3, 4, 5, 6, 515], [], 1, 0]
    rows[62] = [3, [], [], 1, 5]
    return rows


WORDS = [(777,), (515, 902), (11, 12, 13, 14, 21, 22, 23, 900), (11, 12, 13, 14, 21, 22, 24, 901), (V - 1, 0), (1, 2, 3, 903)]


def _launch(rows, n_eos, vocab=V, ld_pad=5, words=WORDS, seed=0):
    """One vis_ban_f32 launch over ``rows`` -> (input before, input after, the whole out buffer) as int32 bit patterns."""
    B, ld = len(rows), vocab + ld_pad
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, ld)).astype(np.float32) * 4
    toks = np.asarray(ALPHABET, dtype=np.int32)[rng.integers(0, len(ALPHABET), (B, T))]      # stale ids around the reply
    prompt = np.asarray(ALPHABET, dtype=np.int32)[rng.integers(0, len(ALPHABET), (B, PL))]
    for b, (n, p, g, mt, g0) in enumerate(rows):
        prompt[b, :len(p)] = p
        toks[b, g0:g0 + len(g)] = g
    dev = "cuda"
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    xd = torch.from_numpy(x).to(dev)
    out = torch.full((B + 1, ld), SENTINEL, dtype=torch.int32, device=dev)
    table = np.zeros((16, 8), dtype=np.int32)
    for w, ids in enumerate(words):
        table[w, :len(ids)] = ids
    eos = np.zeros(8, dtype=np.int32)
    eos[:3] = EOS
    hip.ban(xd[:, :vocab], i32(prompt), i32([len(r[1]) for r in rows]), i32(toks), i32([r[4] for r in rows]),
            i32([r[4] + len(r[2]) for r in rows]), i32([r[0] for r in rows]), i32([r[3] for r in rows]), i32(table),
            [len(w) for w in words], i32(eos), n_eos, out.view(torch.float32)[:B, :vocab])
    torch.cuda.synchronize()
    return x.view(np.int32), xd.cpu().numpy().view(np.int32), out.cpu().numpy()


def _check(rows, n_eos, vocab=V, **kw):
    x, x_after, out = _launch(rows, n_eos, vocab, **kw)
    B = len(rows)
    assert np.array_equal(x, x_after)                                    # the input rows are unchanged
    assert (out[B] == SENTINEL).all() and (out[:B, vocab:] == SENTINEL).all()      # rows beyond the batch, the rows' padding
    ninf = np.float32(-np.inf).view(np.int32)
    hits = 0
    for b, (n, p, g, mt, g0) in enumerate(rows):
        want = ban_ref(p, g, n, kw.get("words", WORDS), mt, EOS[:n_eos], vocab=vocab)
        got = set(np.flatnonzero(out[b, :vocab] == ninf).tolist())
        assert got == want, (b, rows[b][0], len(p), len(g), mt, sorted(got ^ want))
        keep = np.ones(vocab, dtype=bool)
        keep[list(want)] = False
        assert np.array_equal(out[b, :vocab][keep], x[b, :vocab][keep]), b           # bit-identical elsewhere
        hits += bool(ban_ref(p, g, n, vocab=vocab))
    return hits


@pytest.mark.parametrize("ld_pad", [5, 6])           # rows 16 bytes apart in whole vectors (dwordx4 copies) and not (scalar)
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("n_eos", [1, 3])
def test_kernel_matches_ban_ref(B, n_eos, ld_pad):
    rows = _rows()
    hits = sum(_check(rows[r:r + B], n_eos, ld_pad=ld_pad) for r in range(0, 64 - B + 1, B))
    assert hits >= 20                                # the n-gram rule had something to ban in many rows
    # the words' rows did what they were written for
    assert ban_ref(*rows[60][1:3], 0, WORDS) == {777, 900} and ban_ref(*rows[61][1:3], 0, WORDS) == {777, 902}
    assert ban_ref(*rows[62][1:3], 3, WORDS, 1, EOS[:n_eos]) == {777, *EOS[:n_eos]}


def test_kernel_no_words_no_eos_and_a_row_with_everything_off():
    rows = _rows()
    _check(rows[:8], 0, words=[])
    x, _, out = _launch([[0, [1, 2], [1, 2], 0, 0]], 3, words=[])       # all three off: still copied
    assert np.array_equal(out[0, :V], x[0, :V])


def test_kernel_where_the_grid_is_capped():
    """64 rows of 40001 ids: 40 workgroups per row would pass the cap, so each of 32 owns a longer run of ids; the ids sit on
    the seams between those runs."""
    vocab = 40001
    per = ((vocab + 3) // 4 + 31) // 32 * 4              # ids per workgroup
    alphabet = [0, per - 1, per, 7 * per - 1, 7 * per, 31 * per, vocab - 1, vocab]
    rng = np.random.default_rng(5)
    rows = []
    for i in range(64):
        gen = [alphabet[j] for j in rng.integers(0, 8, 300)]
        rows.append([1 + i % 3, [alphabet[j] for j in rng.integers(0, 8, 5)], gen, 301 if i % 2 else 0, i % 5])
    assert _check(rows, 3, vocab, words=[(per, 31 * per - 1)]) >= 56


def test_argument_errors_launch_nothing():
    B = 2
    lib = hip.load()
    dev = "cuda"
    x = torch.zeros((B, V), dtype=torch.float32, device=dev)
    out = torch.full((B, V), SENTINEL, dtype=torch.int32, device=dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    prompt, plen, toks, gen0, step, ngram, mt, words, eos = z(B, PL), z(B), z(B, T), z(B), z(B), z(B), z(B), z(16, 8), z(8)
    lens = (ctypes.c_int * 16)(*([2] * 16))
    good = dict(logits=x.data_ptr(), V=V, ld=V, prompt=prompt.data_ptr(), ld_prompt=PL, plen=plen.data_ptr(),
                toks=toks.data_ptr(), T=T, gen0=gen0.data_ptr(), step=step.data_ptr(), ngram=ngram.data_ptr(),
                mt=mt.data_ptr(), words=words.data_ptr(), lens=lens, n_words=16, eos=eos.data_ptr(), n_eos=8,
                out=out.data_ptr(), ld_out=V, B=B)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vis_ban_f32(a["logits"], a["V"], a["ld"], a["prompt"], a["ld_prompt"], a["plen"], a["toks"], a["T"], a["gen0"],
                               a["step"], a["ngram"], a["mt"], a["words"], a["lens"], a["n_words"], a["eos"], a["n_eos"],
                               a["out"], a["ld_out"], a["B"], torch.cuda.current_stream().cuda_stream)

    bad = [dict(logits=None), dict(prompt=None), dict(plen=None), dict(toks=None), dict(gen0=None), dict(step=None),
           dict(ngram=None), dict(mt=None), dict(words=None), dict(eos=None), dict(out=None), dict(lens=None),
           dict(V=0), dict(V=262145), dict(ld=V - 1), dict(ld_out=V - 1), dict(B=0), dict(B=65), dict(T=0), dict(ld_prompt=0),
           dict(n_words=17), dict(n_words=-1), dict(lens=(ctypes.c_int * 16)(*([2] * 15 + [9]))),
           dict(lens=(ctypes.c_int * 16)(*([0] + [2] * 15))), dict(n_eos=9), dict(n_eos=-1),
           dict(logits=x.data_ptr() + 2), dict(out=out.data_ptr() + 2), dict(words=words.data_ptr() + 1),
           dict(step=step.data_ptr() + 2), dict(out=x.data_ptr())]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the wrapper raises before the library sees anything it would refuse
    for kw in (dict(word_len=[9]), dict(word_len=[1] * 17), dict(n_eos=9)):
        a = dict(word_len=[2], n_eos=1)
        a.update(kw)
        with pytest.raises(hip.HipLibraryError):
            hip.ban(x, prompt, plen, toks, gen0, step, ngram, mt, words, a["word_len"], eos, a["n_eos"], out.view(torch.float32))
    with pytest.raises(hip.HipLibraryError):
        hip.ban(x, prompt, plen, toks, gen0, step, ngram, mt, words.view(8, 16)[:, :8], [2], eos, 1, out.view(torch.float32))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0 and call(n_words=0, lens=None, n_eos=0) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ----------------------------------------------------------------------------- engines
def _record_picks(monkeypatch):
    """BanBuffers.apply wrapped to keep, per launch, the rows the launch read and wrote (slot 0's) and the counters."""
    seen, orig = [], BanBuffers.apply

    def apply(self, logits, tokens, step, slot=0):
        out = orig(self, logits, tokens, step, slot)
        first = (lambda t: t[0] if t.dim() == 2 else t)
        seen.append((first(logits).clone(), first(out).clone(), int(step.reshape(-1)[0]), int(self.gen0[slot])))
        return out
    monkeypatch.setattr(BanBuffers, "apply", apply)
    return seen, orig


def _no_ngram_twice(prompt, reply, n):
    """No n-gram that ends in the reply occurs earlier in prompt + reply."""
    h = list(prompt) + list(reply)
    grams = [tuple(h[i:i + n]) for i in range(len(h) - n + 1)]
    return all(grams[i] not in grams[:i] for i in range(max(len(prompt) - n + 1, 0), len(grams)))


def _engine_checks(eng, a, b, monkeypatch, kw, single_is_batch_exact: bool):
    eos = list(eng.cfg.eos_ids)
    vocab = eng.cfg.vocab
    plain = eng.generate(*a, **kw)
    # --- no_repeat_ngram_size = 2, eager: every pick is the argmax of the row it read with ban_ref's ids taken out
    seen, orig = _record_picks(monkeypatch)
    eager = eng.generate(*a, no_repeat_ngram_size=2, use_graph=False, **kw)
    monkeypatch.setattr(BanBuffers, "apply", orig)
    repeats = not _no_ngram_twice(a[0], plain, 2)          # whether the plain reply gives the ban anything to do
    print(f"the plain reply repeats a bigram: {repeats}")
    assert len(seen) == len(eager) and (eager != plain) == repeats
    for k, (raw, out, step, gen0) in enumerate(seen):
        assert step - gen0 == k
        banned = sorted(ban_ref(a[0], eager[:k], 2, vocab=vocab))
        want = raw.clone()
        want[banned] = -float("inf")
        assert torch.equal(want.view(torch.int32), out.view(torch.int32)), k
        assert int(torch.argmax(out)) == eager[k], k
    assert _no_ngram_twice(a[0], eager, 2)
    assert eng.generate(*a, no_repeat_ngram_size=2, **kw) == eager                  # graph replay
    assert eng.ban_on is False and eng._ban_key() == (False,)
    assert eng.generate(*a, **kw) == plain                                           # off again
    # --- min_tokens: EOS all but forced ends the reply at once; min_tokens=5 gives exactly 5 tokens in front of it
    bias = {e: 100.0 for e in eos}
    at_once = eng.generate(*a, max_new_tokens=16, logit_bias=bias)
    assert [t for t in at_once if t not in eos] == [] and eng.last_finish[0][0] == "eos"
    held = eng.generate(*a, max_new_tokens=16, logit_bias=bias, min_tokens=5)
    assert len([t for t in held if t not in eos]) == 5 and not set(held[:5]) & set(eos) and eng.last_finish[0][0] == "eos"
    assert len(held) == 5 + (1 if eng.keep_eos else 0)
    # --- bad_words: the token at k, as text, banned: the reply is the same in front of k, differs at k, never holds the id
    tok = eng.tokenizer
    k = next(i for i, t in enumerate(plain) if i >= 1 and t not in plain[:i] and tok.encode(tok.decode([t])) == [t])
    word = tok.decode([plain[k]])
    without = eng.generate(*a, bad_words=[word], **kw)
    assert without[:k] == plain[:k] and without[k] != plain[k] and plain[k] not in without
    # --- n = 2 with a seed: both choices obey both bans
    two = eng.generate_batch([a], n=2, seeds=[5], no_repeat_ngram_size=2, bad_words=[word], **dict(kw, temperature=1.0))[0]
    assert len(two) == 2
    for choice in two:
        assert _no_ngram_twice(a[0], choice, 2) and plain[k] not in choice
    # --- a batch mixing on and off rows: the off row is its reply from a call without the switches, the on rows are theirs
    off = eng.generate_batch([a, b, a], **kw)
    mixed = eng.generate_batch([a, b, a], no_repeat_ngram_size=[2, None, None], **kw)
    assert mixed[1] == off[1] and mixed[2] == off[2] and (mixed[0] != off[0]) == (not _no_ngram_twice(a[0], off[0], 2))
    moved = eng.generate_batch([b, a, a], no_repeat_ngram_size=[None, None, 2], **kw)
    assert moved[2] == mixed[0] and _no_ngram_twice(a[0], mixed[0], 2)              # whatever slot the request runs in
    assert eng.generate_batch([a, b, a], no_repeat_ngram_size=[2, None, None], use_graph=False, **kw)[0] == mixed[0]
    print(f"single == row of a batch of three: {eager == mixed[0]}")
    if single_is_batch_exact:
        assert mixed[0] == eager
    else:
        assert mixed[0][:1] == eager[:1]
    with pytest.raises(ValueError, match="JSON"):
        eng.generate(*a, max_new_tokens=4, min_tokens=2, json_mode=True)


def test_qwen_engine(device, monkeypatch):
    """single == in a batch of three, token for token: with VIS_ROWS_GEMV=3 the batched step is the single-sequence
    arithmetic, so nothing but the ban parameters could differ."""
    monkeypatch.setenv("VIS_ROWS_GEMV", "3")
    cfg, eng = _qwen_engine(device, max_batch=4)
    a, b = _qwen_reqs(device)
    _engine_checks(eng, a, b, monkeypatch, dict(max_new_tokens=24, ignore_eos=True), True)


def test_mllama_engine(device, monkeypatch):
    """The batched step of this engine is not the single-sequence arithmetic: single and in-batch agree on the prompt pass's
    pick, and the full reply is compared between batches that hold the request in different slots."""
    eng, a, b = _mllama(device)
    _engine_checks(eng, a, b, monkeypatch, dict(max_new_tokens=24, stop_on_eos=False), False)


@pytest.mark.parametrize("model", ["synthetic:tiny", "synthetic:mllama-tiny"])
def test_client_min_tokens_and_bad_words(device, tmp_path, model):
    from vision_inspection_system_amd.client import LocalVLMClient, get_model
    c = LocalVLMClient()
    m = _msgs(tmp_path, 1)
    lm = get_model(model)
    bias = {str(e): 100 for e in lm.cfg.eos_ids}
    kept = 1 if lm.engine.keep_eos else 0
    r = c.chat.completions.create(model=model, messages=m, max_tokens=16, logit_bias=bias)
    assert r.usage["completion_tokens"] == kept and r.choices[0].finish_reason == "stop"
    r = c.chat.completions.create(model=model, messages=m, max_tokens=16, logit_bias=bias, min_tokens=5)
    assert r.usage["completion_tokens"] == 5 + kept and r.choices[0].finish_reason == "stop"
    many = c.complete_many(model, [m, m], max_tokens=16, no_repeat_ngram_size=2, bad_words=["e", "th"], min_tokens=4)
    assert many[0].choices[0].message.content == many[1].choices[0].message.content
    assert "e" not in many[0].choices[0].message.content and "th" not in many[0].choices[0].message.content
    assert many[0].usage["completion_tokens"] >= 4
    with pytest.raises(ValueError):
        c.chat.completions.create(model=model, messages=m, max_tokens=4, min_tokens=5)
    with pytest.raises(ValueError):
        c.chat.completions.create(model=model, messages=m, max_tokens=4, min_tokens=2, response_format={"type": "json_object"})
