"""Hand-made histories for the prompt-lookup drafter, shared by the CPU test of spec.propose() and the GPU test of
vis_spec_draft: (history, ids of it that are the prompt, k, prompt_lookup_max, prompt_lookup_min, expected drafts)."""

PROPOSE_CASES = [
    # the match straddles the prompt / reply boundary: [1, 2 | 3] is found again at the end
    ([7, 1, 2, 3, 4, 8, 1, 2, 3], 3, 3, 3, 2, [4, 8, 1]),
    # two earlier occurrences of [1, 2]: the latest one wins
    ([1, 2, 5, 1, 2, 6, 1, 2], 4, 3, 2, 2, [6, 1, 2]),
    ([1, 2, 5, 1, 2, 6, 1, 2], 4, 1, 2, 2, [6]),
    # the continuation is shorter than k
    ([1, 2, 1, 2], 2, 3, 2, 2, [1, 2]),
    ([4, 4], 1, 3, 1, 1, [4]),
    # no match
    ([1, 2, 3, 4, 5], 5, 3, 4, 2, []),
    ([6], 1, 3, 4, 1, []),
    # m falls from max to min: nothing at 4 and 3, [2, 3] at 2
    ([9, 2, 3, 7, 5, 2, 3], 2, 3, 4, 2, [7, 5, 2]),
    # the longest window wins over a later match of a shorter one
    ([1, 2, 3, 4, 9, 2, 3, 5, 1, 2, 3], 6, 2, 3, 2, [4, 9]),
    # the history is exactly as long as the window: no room for an earlier copy at that m
    ([3, 3, 3], 3, 2, 3, 1, [3]),
]
