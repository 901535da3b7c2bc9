"""Several choices per request (``n``) from one prompt pass: where every choice's slot lies, which rows a choice's slot holds
itself and which it reads from the slot that ran the prompt pass (the fork tables of vis_decode_attn_forked), and the
host-side contract of those tables.  Pure Python: no device, no engine."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

FORK_ALIGN = 64      # a fork length is a multiple of one decode-attention split (hip.DECODE_KEYS_PER_SPLIT)


def check_n(n, max_batch: int) -> Optional[int]:
    """``n`` of one request: None, or an integer in 1..max_batch (bools, floats and strings are refused)."""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int):
        raise ValueError("n must be an integer")
    if not 1 <= n <= max_batch:
        raise ValueError(f"n must lie in 1..{max_batch} (max_batch)")
    return n


def check_n_list(n, n_req: int, max_batch: int) -> Optional[List[int]]:
    """``n`` of a group of requests: None, one integer for every request, or a sequence with one integer per request; the
    total of all choices must fit max_batch."""
    if n is None:
        return None
    if isinstance(n, (str, bytes)):
        raise ValueError("n must be an integer or one integer per request")
    if isinstance(n, (list, tuple)):
        if len(n) != n_req:
            raise ValueError(f"n: {len(n)} values for {n_req} requests")
        ns = [check_n(v, max_batch) for v in n]
        if any(v is None for v in ns):
            raise ValueError("n: one integer per request")
    else:
        ns = [check_n(n, max_batch)] * n_req
    if sum(ns) > max_batch:
        raise ValueError(f"{sum(ns)} choices do not fit max_batch={max_batch}")
    return ns


class ForkLayout(NamedTuple):
    slots: List[List[int]]                     # request j -> the slot of each of its choices (choice 0 = its root)
    parent: List[int]                          # per slot: the slot whose cache holds its keys [0, fork_len)
    fork_len: List[int]                        # per slot: a multiple of 64; 0 = reads everything from its own cache
    holds: List[int]                           # per slot: rows [0, holds) of its OWN cache are written
    copies: List[Tuple[int, int, int, int]]    # (child, root, lo, hi): rows [lo, hi) of the root are copied into the child


def fork_layout(prompt_lens: Sequence[int], n: Sequence[int], prefix_len: int, max_batch: int) -> ForkLayout:
    """Slots and fork tables of a batch whose request j (prompt of prompt_lens[j] rows, in slot j as today) has n[j] choices.

    Roots keep slots 0..R-1 in request order; the children follow them, request by request.  A child of a prompt of S rows
    reads rows [0, 64 * (S // 64)) from its root and gets rows [64 * (S // 64), S) copied.  ``prefix_len`` (a multiple of
    64, 0 = none): the text prefix every root holds a copy of - every root but slot 0 reads it from slot 0."""
    R = len(prompt_lens)
    if len(n) != R:
        raise ValueError(f"n: {len(n)} values for {R} requests")
    total = sum(n)
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in n):
        raise ValueError("n: integers >= 1")
    if total > max_batch:
        raise ValueError(f"{total} choices do not fit max_batch={max_batch}")
    if prefix_len < 0 or prefix_len % FORK_ALIGN or any(S < 1 or prefix_len > S for S in prompt_lens):
        raise ValueError("bad text prefix length")
    slots = [[j] for j in range(R)]
    parent = [0 if prefix_len else j for j in range(R)]
    fork_len = [prefix_len if j else 0 for j in range(R)]
    holds = list(prompt_lens)
    copies = []
    nxt = R
    for j in range(R):
        S = prompt_lens[j]
        fl = FORK_ALIGN * (S // FORK_ALIGN)
        for _ in range(n[j] - 1):
            slots[j].append(nxt)
            parent.append(j if fl else nxt)
            fork_len.append(fl)
            holds.append(0 if fl else S)
            copies.append((nxt, j, fl, S))
            nxt += 1
    lay = ForkLayout(slots, parent, fork_len, holds, copies)
    check_fork_tables(lay.parent, lay.fork_len, holds=lay.holds)
    return lay


def check_fork_tables(parent: Sequence[int], fork_len: Sequence[int], cache_tokens: Optional[int] = None,
                      holds: Optional[Sequence[int]] = None) -> None:
    """The contract of the fork tables, checked on the host before any launch (the kernels only make table contents
    harmless): every parent lies in the batch, every fork length is a multiple of 64 inside the cache, and a parent holds
    the rows its children read ITSELF - it is its own parent (parent[parent[b]] == parent[b]), or reads nothing from
    another slot (fork_len 0), or ``holds`` says its own cache has those rows (a root that took a copy of the batch's text
    prefix).  A child of a child is refused."""
    B = len(parent)
    if len(fork_len) != B or (holds is not None and len(holds) != B):
        raise ValueError("fork tables: one entry per sequence")
    for b in range(B):
        p, fl = parent[b], fork_len[b]
        if isinstance(p, bool) or isinstance(fl, bool) or not isinstance(p, int) or not isinstance(fl, int):
            raise ValueError("fork tables hold integers")
        if not 0 <= p < B:
            raise ValueError(f"fork tables: parent {p} of sequence {b} lies outside the batch of {B}")
        if fl < 0 or fl % FORK_ALIGN or (cache_tokens is not None and fl >= cache_tokens):
            raise ValueError(f"fork tables: fork_len {fl} of sequence {b} is not a multiple of {FORK_ALIGN} inside the cache")
    for b in range(B):
        p, fl = parent[b], fork_len[b]
        if fl == 0 or p == b:
            continue
        own = parent[p] == p or fork_len[p] == 0 or (holds is not None and holds[p] >= fl)
        if not own:
            raise ValueError(f"fork tables: sequence {b} forks from {p}, which reads those rows from {parent[p]} itself")
        if holds is not None and holds[p] < fl:
            raise ValueError(f"fork tables: sequence {p} holds {holds[p]} rows, sequence {b} reads {fl} from it")
