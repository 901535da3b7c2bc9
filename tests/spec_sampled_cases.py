"""Inputs and float64 expectations for vis_spec_accept_sampled (csrc/spec.hip), built with the reference of the token pick,
tests/pick_exact.py: row r of a launch at step st must produce the token of  argmax_i fl(v_i * inv_temp + gumbel_noise(seed,
st + r, i)), ties to the lower id.  `candidates` gives, per draw, the ids a correct kernel may pick; a draw with one candidate
is decisive.  A table entry is valid only if at most pick_exact.AMBIGUOUS_CAP (1 %) of its draws are ambiguous - a condition on
the INPUTS, met from the reference alone: an entry whose first inputs miss it is rebuilt from the next generator seed, as
pick_exact._resolve does.  An entry holds at most 4 rows x 3 steps = 12 draws, so the cap means: none.

CPU only: numpy and float64, never the library under test."""
import dataclasses
import functools

import numpy as np

from pick_exact import AMBIGUOUS_CAP, candidates, logit_row

VS = (200, 1000, 4099, 70001, 152064)      # nb = 1; 4 blocks with a ragged last one; 17 blocks; the nb = 256 stride loop (twice)
STARTS = (0, 5, 1000)
INV_TEMPS = (0.0, 0.5, 10.0)
SEEDS = (0, 0xFFFFFFFF)
ROW_KINDS = ("tie_wg", "nan", "gauss8", "gauss1", "tie_wave", "shaped", "const")


def params_words(inv_temp: float, seed: int) -> np.ndarray:
    """The 8 bytes vis_spec_accept_sampled reads, as two int32: the bits of the f32 inv_temp, the seed modulo 2^32."""
    return np.array([np.float32(inv_temp).view(np.uint32), int(seed) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def diff_rows(V: int) -> np.ndarray:
    """Four logit rows for the differential test at V: a planted tie (two workgroups where V has two), all NaN, two Gaussians."""
    rng = np.random.default_rng([23, V])
    rows = np.stack([logit_row(k, V, rng) for k in ROW_KINDS[:4]])
    rows.setflags(write=False)
    return rows


def diff_row_ids(R: int):
    """Which of diff_rows' rows a launch of R rows carries: R = 1 the NaN row, 3 and 4 the tie and the NaN row."""
    return [(R + r) % 4 for r in range(R)]


@dataclasses.dataclass(eq=False)
class SampledCase:
    name: str
    V: int
    R: int
    inv_temp: float
    seed: int
    kinds: tuple
    logits: np.ndarray         # [R, V] f32

    @functools.cached_property
    def expected(self):
        """{st: [candidates of row r at hash counter st + r]}"""
        ids = np.arange(self.V)
        return {st: [candidates(self.logits[r], self.inv_temp, self.seed, st + r, ids) for r in range(self.R)] for st in STARTS}

    def ambiguous_share(self) -> float:
        draws = [c for per_st in self.expected.values() for c in per_st]
        return sum(len(c) > 1 for c in draws) / len(draws)


def _case(V, R, inv_temp, seed, off):
    for attempt in range(32):
        rng = np.random.default_rng([29, V, R, int(inv_temp * 2), attempt])
        kinds = tuple(ROW_KINDS[(off + attempt + r) % len(ROW_KINDS)] for r in range(R))
        logits = np.stack([logit_row(k, V, rng) for k in kinds])
        case = SampledCase(f"V{V}-R{R}-t{inv_temp}-s{seed:x}", V, R, inv_temp, seed, kinds, logits)
        if case.ambiguous_share() <= AMBIGUOUS_CAP:
            logits.setflags(write=False)
            return case
    raise AssertionError(f"V={V} R={R} inv_temp={inv_temp}: no inputs within the ambiguity cap")


@functools.lru_cache(maxsize=None)
def cases(V: int):
    """The entries of one vocabulary size: both sampling temperatures and the greedy one, R / seed / row kinds rotating."""
    vi = VS.index(V)
    return tuple(_case(V, 1 + (vi + ti) % 4, t, SEEDS[(vi + ti) % 2], 2 * vi + 3 * ti) for ti, t in enumerate((0.5, 10.0, 0.0, 10.0)))
