"""Token bans (the ``no_repeat_ngram_size=`` / ``bad_words=`` / ``min_tokens=`` keywords of the engines' generate and
generate_batch): the switches that depend on the SEQUENCE of tokens rather than on single ids.

While any of them is on, every pick - prompt pass or decode step, single or batched, eager or graph-replayed, nucleus
sampling, penalties and shaping included - is handed the row vis_ban_f32 wrote instead of the logits it would have read: a
copy (of the penalised row while penalties are on) with the banned ids at -inf.  With h = the prompt ids followed by the ids
generated so far, L of them (transformers' meaning: the prompt counts):

    no_repeat_ngram_size = n:  h[i+n-1] is banned for every i with i + n - 1 < L and h[i .. i+n-2] == h[L-n+1 .. L-1]
                               (transformers' NoRepeatNGramLogitsProcessor: no n-gram occurs twice; n = 1 bans every id of h)
    bad_words:                 the last id of a word of m ids is banned when m == 1, or when the m - 1 ids in front of it are
                               the last m - 1 of h (transformers' NoBadWordsLogitsProcessor, vLLM's bad_words); a match may
                               begin in the prompt
    min_tokens = k:            every EOS id is banned while fewer than k tokens have been generated (vLLM's min_tokens)

The raw row stays where it is (logprobs keep reading it).  n and k live in device memory, one per slot, so requests of one
batch may differ and a captured decode graph serves any values; the words are one table per request group.  Out of scope,
refused with ValueError: any of the three together with ``json_mode`` / ``json_schema`` (a ban could leave the grammar no
token).  ``min_tokens`` bans EOS ids only: a ``stop`` string may still end the reply earlier.  ``ban_ref`` is the numpy
restatement the tests compare the kernel against."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .penalties import per_request

MAX_NGRAM = 64
MAX_WORDS = hip.BAN_MAX_WORDS            # rows of the device table, both spellings of a word counted
MAX_WORD_LEN = hip.BAN_MAX_WORD_LEN      # ids of one word
MAX_EOS = hip.BAN_MAX_EOS
NEUTRAL = (0, 0)                         # (no_repeat_ngram_size, min_tokens) of a request that asks for neither


def _integer(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def check_ngram(n) -> int:
    """None or 0 (off) or an integer in 1..64."""
    if n is None:
        return 0
    if not _integer(n) or not 0 <= int(n) <= MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size must be None or an integer in 0..{MAX_NGRAM}")
    return int(n)


def check_min_tokens(k, max_tokens: Optional[int] = None) -> int:
    """None or 0 (off) or an integer >= 1, at most ``max_tokens`` where that is known."""
    if k is None:
        return 0
    if not _integer(k) or int(k) < 0:
        raise ValueError("min_tokens must be None or an integer >= 0")
    if max_tokens is not None and int(k) > int(max_tokens):
        raise ValueError(f"min_tokens={int(k)} exceeds max_tokens={int(max_tokens)}")
    return int(k)


def check_bad_words(words) -> Optional[Tuple[str, ...]]:
    """None or an empty list (off) or a list of at most 16 non-empty strings.  How many ids a string has, and whether both
    of its spellings fit the table, is judged against the tokenizer when the request is switched on (bad_word_ids)."""
    if words is None:
        return None
    if isinstance(words, (str, bytes)) or not isinstance(words, Sequence):
        raise ValueError("bad_words must be None or a list of strings")
    if len(words) > MAX_WORDS:
        raise ValueError(f"bad_words holds {len(words)} entries, at most {MAX_WORDS} are allowed")
    for w in words:
        if not isinstance(w, str) or not w:
            raise ValueError("bad_words: every entry must be a non-empty string")
    return tuple(words) or None


class BanRequest(NamedTuple):
    rows: List[Tuple[int, int]]              # per request: (no_repeat_ngram_size, min_tokens)
    words: Optional[Tuple[str, ...]]         # the group's bad words


def check_ban(no_repeat_ngram_size, bad_words, min_tokens, n: int, max_tokens: Optional[int] = None, *, json_mode=False,
              json_schema=None) -> Optional[BanRequest]:
    """The bans of n requests - ``no_repeat_ngram_size`` and ``min_tokens`` one value for the group or one per request,
    ``bad_words`` one list for the group - or None when no request asks for any (bans off: the engines launch what they
    launch without the keywords).  Together with JSON mode or a schema they are refused."""
    ns = per_request(no_repeat_ngram_size, n, check_ngram, "no_repeat_ngram_size")
    ks = per_request(min_tokens, n, lambda k: check_min_tokens(k, max_tokens), "min_tokens")
    words = check_bad_words(bad_words)
    rows = list(zip(ns, ks))
    if words is None and all(r == NEUTRAL for r in rows):
        return None
    if json_mode or json_schema is not None:
        raise ValueError("no_repeat_ngram_size / bad_words / min_tokens together with JSON mode or a JSON schema is not "
                         "supported: a ban could leave the grammar no token")
    return BanRequest(rows, words)


def ban_kwargs(ban: Optional[BanRequest]) -> dict:
    """The first request of check_ban's result as the keywords of a single-request call ({} when off)."""
    if ban is None:
        return {}
    return {"no_repeat_ngram_size": ban.rows[0][0], "min_tokens": ban.rows[0][1], "bad_words": list(ban.words or ()) or None}


def bad_word_ids(words: Optional[Sequence[str]], tokenizer) -> List[Tuple[int, ...]]:
    """The id sequences the device table gets for ``words``: each string as the tokenizer encodes it and - where the
    tokenizer has another spelling of the same length for the word behind a space (vLLM's rule: the first id differs) - that
    spelling too.  ValueError for a word of no or more than 8 ids and for more than 16 sequences."""
    out: List[Tuple[int, ...]] = []
    for w in words or ():
        ids = tuple(int(t) for t in tokenizer.encode(w))
        spaced = tuple(int(t) for t in tokenizer.encode(" " + w.lstrip()))
        forms = [ids]
        if len(spaced) == len(ids) and spaced and ids and spaced[0] != ids[0]:
            forms.append(spaced)
        for f in forms:
            if not 1 <= len(f) <= MAX_WORD_LEN:
                raise ValueError(f"bad_words: {w!r} has {len(f)} token ids, 1..{MAX_WORD_LEN} are allowed")
            if f not in out:
                out.append(f)
    if len(out) > MAX_WORDS:
        raise ValueError(f"bad_words: {len(out)} token sequences (both spellings of a word counted) exceed the table of "
                         f"{MAX_WORDS}")
    return out


def ban_ref(prompt_ids: Sequence[int], generated_ids: Sequence[int], ngram: int = 0, words: Sequence[Sequence[int]] = (),
            min_tokens: int = 0, eos_ids: Sequence[int] = (), vocab: Optional[int] = None) -> set:
    """The ids vis_ban_f32 takes out of one row's pick, as a set (ids outside [0, vocab) dropped when vocab is given)."""
    h = np.concatenate([np.asarray(list(prompt_ids), dtype=np.int64).reshape(-1),
                        np.asarray(list(generated_ids), dtype=np.int64).reshape(-1)])
    L, n = h.size, int(ngram)
    banned = set()
    if n == 1:
        banned.update(h.tolist())
    elif n > 1 and L >= n:
        win = np.lib.stride_tricks.sliding_window_view(h, n)           # every n-gram of h: rows i = h[i .. i+n-1]
        hit = (win[:, :n - 1] == h[L - n + 1:]).all(axis=1)
        banned.update(win[hit, n - 1].tolist())
    for w in words:
        w = [int(t) for t in w]
        m = len(w)
        if m == 1 or (m > 1 and L >= m - 1 and h[L - m + 1:].tolist() == w[:m - 1]):
            banned.add(w[m - 1])
    if len(generated_ids) < int(min_tokens):
        banned.update(int(e) for e in eos_ids)
    return {v for v in banned if vocab is None or 0 <= v < vocab}


class BanBuffers:
    """One engine's device state of vis_ban_f32, one row per slot (prompt passes of different slots may run on different
    streams): n and min_tokens, the prompt's ids and their number, where the generated ids start in the slot's token row,
    and the rows the pick kernels read; the group's word table and the model's EOS ids."""

    def __init__(self, slots: int, ctx: int, vocab: int, eos_ids: Sequence[int], device):
        if len(eos_ids) > MAX_EOS:
            raise ValueError(f"min_tokens: the model has {len(eos_ids)} EOS ids, the device table holds {MAX_EOS}")
        i32 = dict(dtype=torch.int32, device=device)
        self.ngram = torch.zeros(slots, **i32)
        self.min_tokens = torch.zeros(slots, **i32)
        self.plen = torch.zeros(slots, **i32)
        self.gen0 = torch.zeros(slots, **i32)
        self.prompt = torch.zeros((slots, ctx), **i32)
        self.words = torch.zeros((MAX_WORDS, MAX_WORD_LEN), **i32)
        self.word_len: Tuple[int, ...] = ()
        self.eos = torch.zeros(MAX_EOS, **i32)
        self.n_eos = len(eos_ids)
        if self.n_eos:
            self.eos[:self.n_eos].copy_(torch.tensor([int(e) for e in eos_ids], dtype=torch.int32))
        self.out = torch.empty((slots, vocab), dtype=torch.float32, device=device)
        self.slots, self.ctx, self.vocab = slots, ctx, vocab
        self._loaded: list = []

    def load(self, word_ids: Sequence[Tuple[int, ...]], streams=()) -> None:
        """Make ``word_ids`` (bad_word_ids' result) the word table of the launches that follow.  Called before a request
        group's first prompt pass, outside any captured graph: the copy runs on the current stream once everything queued on
        ``streams`` has finished, and those streams then wait for it."""
        word_ids = [tuple(w) for w in word_ids]
        self.word_len = tuple(len(w) for w in word_ids)
        if word_ids == self._loaded:
            return
        table = np.zeros((MAX_WORDS, MAX_WORD_LEN), dtype=np.int32)
        for i, w in enumerate(word_ids):
            table[i, :len(w)] = w
        cur = torch.cuda.current_stream(self.words.device) if self.words.is_cuda else None
        for s in streams if cur is not None else ():
            cur.wait_stream(s)
        self.words.copy_(torch.from_numpy(table))
        for s in streams if cur is not None else ():
            s.wait_stream(cur)
        self._loaded = word_ids

    def begin(self, slot: int, prompt_ids: torch.Tensor, step: torch.Tensor, ngram: int, min_tokens: int) -> None:
        """A new request in ``slot``, on the current stream ahead of its prompt pass's pick: its n and min_tokens, its
        prompt ids (int32 on the device) and where its generated ids start - at the position ``step`` (int32 [1], device)
        names now, the one the prompt pass's pick is about to fill."""
        n = int(prompt_ids.numel())
        if n > self.ctx:
            raise ValueError(f"a prompt of {n} ids does not fit the ban history of {self.ctx}")
        self.ngram[slot].fill_(int(ngram))
        self.min_tokens[slot].fill_(int(min_tokens))
        self.plen[slot].fill_(n)
        self.prompt[slot, :n].copy_(prompt_ids.reshape(-1))
        self.gen0[slot:slot + 1].copy_(step.reshape(-1))

    def apply(self, logits: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """The rows of slots slot .. slot + B - 1 with their banned ids at -inf (logits [V] or [B, V]; left intact)."""
        if logits.dim() == 2:
            B = logits.shape[0]
            out = self.out[slot:slot + B]
        else:
            B, out = 1, self.out[slot]
        s = slice(slot, slot + B)
        hip.ban(logits, self.prompt[s], self.plen[s], tokens, self.gen0[s], step, self.ngram[s], self.min_tokens[s],
                self.words, self.word_len, self.eos, self.n_eos, out)
        return out
