"""Shared by test_json_schema.py and test_json_schema_gpu.py: pydantic models whose model_json_schema() is the schema under
test (pydantic is the independent oracle: it wrote the schema and it judges the documents), seeded random instances, and
seeded random walks over a compiled DFA."""
import random
from typing import List, Literal, Optional

import numpy as np
from pydantic import BaseModel

from vision_inspection_system_amd import json_schema as S


# no code validators on these three: the schema is their whole contract
class Flat(BaseModel):
    name: str
    count: int
    ratio: float
    ok: bool
    kind: Literal["a", "b", "ab"]
    note: Optional[str] = None


class Pos(BaseModel):
    x: float
    y: float


class Item(BaseModel):
    id: int
    tag: Literal["x", "yy", "naïve"]
    pos: Optional[Pos] = None


class Nested(BaseModel):
    title: str
    items: List[Item]
    level: Optional[Literal["low", "high"]] = None
    flags: List[bool] = []
    nothing: None = None
    version: Literal[3] = 3


class AllOptional(BaseModel):
    a: Optional[int] = None
    b: Optional[str] = None
    c: Optional[List[int]] = None


class Closed(BaseModel):
    """Every document is short: a reply under this schema always reaches its end."""
    a: Literal["x", "y"]
    b: bool
    c: None


STRINGS = ["", "bolt", "a b", "café", "日本", "\U0001f600", "q\"uote", "back\\slash", "tab\there", "nl\nx", "\x01",
           "/", " "]


def _s(rng):
    return "".join(rng.choice(STRINGS) for _ in range(rng.randint(0, 3)))


def _f(rng):
    return rng.choice([0.0, -0.0, 1.5, -2.25e-7, 6.02e23, 1e16, 3.0, rng.uniform(-1e3, 1e3)])


def _i(rng):
    return rng.choice([0, -1, 7, 10 ** 12, -(10 ** 15), rng.randint(-999, 999)])


def random_instance(model, rng: random.Random):
    if model is Flat:
        return Flat(name=_s(rng), count=_i(rng), ratio=_f(rng), ok=rng.random() < 0.5, kind=rng.choice(["a", "b", "ab"]),
                    note=rng.choice([None, _s(rng)]))
    if model is Nested:
        items = [Item(id=_i(rng), tag=rng.choice(["x", "yy", "naïve"]),
                      pos=rng.choice([None, Pos(x=_f(rng), y=_f(rng))])) for _ in range(rng.randint(0, 3))]
        return Nested(title=_s(rng), items=items, level=rng.choice([None, "low", "high"]),
                      flags=[rng.random() < 0.5 for _ in range(rng.randint(0, 3))])
    if model is AllOptional:
        return AllOptional(a=rng.choice([None, _i(rng)]), b=rng.choice([None, _s(rng)]),
                           c=rng.choice([None, [], [_i(rng), _i(rng)]]))
    from vision_inspection_system_amd.schemas import BoundingBox, DefectInfo, VLMAnalysisResult
    assert model is VLMAnalysisResult
    defects = [DefectInfo(type=_s(rng), location=_s(rng),
                          bbox=rng.choice([None, BoundingBox(x=rng.uniform(0, 50), y=rng.uniform(0, 50), width=rng.uniform(1, 50),
                                                             height=rng.uniform(1, 50))]),
                          safety_impact=rng.choice(["CRITICAL", "MODERATE", "COSMETIC"]), reasoning=_s(rng),
                          confidence=rng.choice(["high", "medium", "low"]), recommended_action=_s(rng))
               for _ in range(rng.randint(0, 3))]
    return VLMAnalysisResult(object_identified=_s(rng), overall_condition=rng.choice(["damaged", "good", "uncertain"]),
                             defects=defects, overall_confidence=rng.choice(["high", "medium", "low"]),
                             analysis_reasoning=rng.choice([None, _s(rng)]),
                             inferred_criticality=rng.choice([None, "low", "medium", "high"]),
                             failure_reason=rng.choice([None, _s(rng)]))


def distance_to_accept(dfa: S.SchemaDFA) -> np.ndarray:
    """Fewest bytes from each state to an accepting one."""
    n = dfa.n_states
    dist = np.full(n, 10 ** 9, dtype=np.int64)
    dist[(dfa.state_flags & S.STATE_ACCEPT) != 0] = 0
    t = dfa.trans.astype(np.int64)
    live = t != S.DEAD
    while True:
        nxt = np.where(live, dist[np.where(live, t, 0)], 10 ** 9).min(axis=1) + 1
        new = np.minimum(dist, nxt)
        if (new == dist).all():
            return dist
        dist = new


def random_walk(dfa: S.SchemaDFA, rng: random.Random, dist: np.ndarray, wander: int = 60, limit: int = 4000,
                stop_at=None):
    """Random accepted bytes from the start state: free for ``wander`` bytes, then three steps in four take a byte that
    brings the end nearer, so the walk terminates.  Returns (bytes, end state); stops early when ``stop_at(state, out)``."""
    by_class = [[b for b in range(256) if dfa.byte_class[b] == c] for c in range(dfa.n_classes)]
    s, out = dfa.start, bytearray()
    while not dfa.state_flags[s] & S.STATE_ACCEPT and len(out) < limit:
        if stop_at is not None and stop_at(s, out):
            break
        classes = [c for c in range(dfa.n_classes) if dfa.trans[s, c] != S.DEAD]
        if len(out) >= wander and rng.random() < 0.75:
            classes = [c for c in classes if dist[dfa.trans[s, c]] < dist[s]]
        c = rng.choice(classes)
        out.append(rng.choice(by_class[c]))
        s = int(dfa.trans[s, c])
    return bytes(out), s
