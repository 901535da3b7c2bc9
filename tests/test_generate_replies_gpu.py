"""``generate`` / ``generate_batch`` of both engines on MI355X against tests/golden/generate_replies.json: the replies of the
cases of tests/golden/gen_generate_replies.py (greedy, sampled, stop string, logprobs, ignoring EOS, batches - eager, lazy
with a failing request, with ``n`` - the one-request routes, a text-only prompt, a reply the context cuts), recorded at the
commit the file names, before the generation loops of the two engines became one.  Tokens, ``last_finish``, the logprob
tokens and the ``decode_steps`` / ``sequences`` of ``last_timing`` compare exactly, a failed request by its exception's type;
the logprob values within 1e-4, the bound tests/test_logprobs_gpu.py puts on the same quantity."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_generate_replies as G  # noqa: E402

pytestmark = pytest.mark.gpu
LOGPROB_TOL = 1e-4

with open(os.path.join(HERE, "golden", "generate_replies.json")) as _f:
    GOLDEN = json.load(_f)["models"]


@pytest.fixture(scope="module")
def engines(device):
    """model -> (engine, requests), each built on first use and kept for the module."""
    built = {}

    def get(model):
        if model not in built:
            built[model] = G.MODELS[model](device)
        return built[model]
    return get


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(G.MODELS)
    for model in G.MODELS:
        assert sorted(GOLDEN[model]["cases"]) == sorted(G.cases_of(model))


def _same_logprobs(got, want, where):
    if want is None or got is None:
        assert got is None and want is None, where
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for g, w in zip(got, want):
            _same_logprobs(g, w, where)
    else:
        assert got["top_ids"] == want["top_ids"], where
        for key in ("token_logprobs", "top_logprobs"):
            g, w = np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
            assert g.shape == w.shape and (g.size == 0 or np.abs(g - w).max() <= LOGPROB_TOL), (where, key)


@pytest.mark.parametrize("model,name", [(m, c) for m in G.MODELS for c in G.cases_of(m)])
def test_reply_is_the_recorded_one(engines, model, name):
    eng, reqs = engines(model)
    want = GOLDEN[model]["cases"][name]
    got = G.run_case(model, name, eng, reqs, bytes(GOLDEN[model]["stop"]))
    got = json.loads(json.dumps(got))      # tuples as the file holds them
    print(model, name, {k: v for k, v in got.items() if k != "logprobs"})
    assert sorted(got) == sorted(want)
    for key in got:
        if key == "logprobs":
            _same_logprobs(got[key], want[key], (model, name))
        else:
            assert got[key] == want[key], (model, name, key)
