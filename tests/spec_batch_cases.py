"""Shared by tests/test_spec_batch.py and tests/test_spec_batch_gpu.py: the prompts of the engine tests (they repeat
themselves, so the prompt lookup has something to draft) and small builders."""
import numpy as np

PHRASE = [72, 105, 33, 116, 104, 101, 114, 101, 32, 119]
N_NEW = 20


def prompts(n: int):
    """n text prompts of different lengths: a phrase repeated (rotated per request), and every third one random."""
    rng = np.random.default_rng(23)
    out = []
    for b in range(n):
        if b % 3 == 2:
            out.append([256] + rng.integers(1, 490, 30 + b).tolist())
        else:
            ph = PHRASE[b % 5:] + PHRASE[:b % 5]
            out.append([256] + ph * (3 + b % 3) + ph[:2 + b % 4])
    return out
