"""Nucleus sampling and per-request seeds, the parts that need no GPU: the float64 reference of the kept set, the
vis_sample_f32 argument checks (before any HIP call), and the argument validation of the client (before any model is
loaded), the engines and the agents."""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETRY_SUBSTRINGS = ("429", "rate", "413", "payload")


@pytest.fixture(scope="module")
def lib():
    p = os.path.join(ROOT, "vision-inspection-system_amd", "csrc", "libvis_hip.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    from vision_inspection_system_amd import hip
    return hip.load()


def _brute(x, T, p, allow=None):
    """Kept set by the definition: every prefix of the sorted order, the first whose mass reaches p (at least one)."""
    ids = [i for i in range(len(x)) if allow is None or allow[i]]
    if not ids:
        return set()
    ids.sort(key=lambda i: (-x[i], i))
    if T == 0:
        return {ids[0]}
    if p >= 1:
        return set(ids)
    m = x[ids[0]]
    w = [math.exp((x[i] - m) / T) for i in ids]
    Z = sum(w)
    acc = 0.0
    for n, wi in enumerate(w, 1):
        acc += wi
        if acc >= p * Z:
            return set(ids[:n])
    return set(ids)


@pytest.mark.parametrize("seed", range(6))
def test_nucleus_ref_matches_brute_force(seed):
    from vision_inspection_system_amd.sampling import nucleus_ref
    rng = np.random.default_rng(seed)
    V = 37
    x = np.round(rng.normal(0, 2, V), 1)          # rounded: ties among the logits
    x[[3, 11, 20]] = x.max()                       # a tie at the top
    allow = rng.random(V) < 0.6
    for T in (0.0, 0.3, 1.0, 2.5):
        for p in (0.0, 0.1, 0.5, 0.9, 0.999, 1.0):
            for a in (None, allow):
                r = nucleus_ref(x, T, p, a)
                want = _brute(list(x), T, p, None if a is None else list(a))
                if T > 0 and 0 < p < 1:
                    # skip the rare row where the float64 sums of the two methods straddle p Z
                    cum = r.cum[r.nkeep - 1] if r.nkeep else 1.0
                    if abs(cum - p) < 1e-12 or (r.nkeep > 1 and abs(r.cum[r.nkeep - 2] - p) < 1e-12):
                        continue
                assert set(np.flatnonzero(r.keep)) == want, (T, p, a is None)
                assert r.nkeep == len(want)


def test_nucleus_ref_edges():
    from vision_inspection_system_amd.sampling import nucleus_ref
    x = np.array([1.0, 3.0, 3.0, 2.0, 3.0])
    # p = 0: the top token, ties to the lower index
    assert list(np.flatnonzero(nucleus_ref(x, 1.0, 0.0).keep)) == [1]
    # p = 1: everything; T = 0: the greedy token whatever p is
    assert nucleus_ref(x, 1.0, 1.0).nkeep == 5
    assert list(np.flatnonzero(nucleus_ref(x, 0.0, 1.0).keep)) == [1]
    # a boundary inside the tie group: 3 equal weights, p = 0.5 of a mass dominated by them needs 2 of them (ids 1, 2)
    r = nucleus_ref(x, 0.01, 0.5)
    assert list(np.flatnonzero(r.keep)) == [1, 2]
    # a constant row: the cut counts ids in order
    c = np.zeros(10)
    assert list(np.flatnonzero(nucleus_ref(c, 1.0, 0.25).keep)) == [0, 1, 2]
    assert nucleus_ref(c, 1.0, 0.3).nkeep == 3 and nucleus_ref(c, 1.0, 0.31).nkeep == 4
    # a mask: the nucleus of the renormalised allowed distribution; an empty mask keeps nothing
    allow = np.array([True, False, False, True, True])
    assert list(np.flatnonzero(nucleus_ref(x, 0.01, 0.5, allow).keep)) == [4]
    assert nucleus_ref(x, 1.0, 0.5, np.zeros(5, bool)).nkeep == 0


def test_sample_entry_point_rejects_bad_arguments_without_gpu(lib):
    from vision_inspection_system_amd import hip
    assert "vis_sample_f32" in hip.exported_symbols() and "vis_sample_ws_bytes" in hip.exported_symbols()
    V, B = 152064, 4
    ws1 = int(lib.vis_sample_ws_bytes(V, 1))
    assert ws1 > 0 and lib.vis_sample_ws_bytes(V, B) == B * ws1
    assert lib.vis_sample_ws_bytes(0, 1) == 0 and lib.vis_sample_ws_bytes(V, 65) == 0 and lib.vis_sample_ws_bytes(V, 0) == 0
    p = 4096     # any non-null address: nothing is launched when an argument is refused

    def call(logits=p, V=V, ld=V, allow=None, ld_allow=0, inv_temp=1.0, top_p=0.9, seeds=p, tokens=p, T=64, cur=p,
             step=p, batch=B, ws=p, nkeep=None):
        return lib.vis_sample_f32(logits, V, ld, allow, ld_allow, inv_temp, top_p, seeds, tokens, T, cur, step, batch, ws,
                                  nkeep, None)
    for bad in (dict(logits=None), dict(seeds=None), dict(tokens=None), dict(cur=None), dict(step=None), dict(ws=None),
                dict(V=0), dict(V=-3), dict(batch=0), dict(batch=65), dict(ld=V - 1), dict(top_p=float("nan")),
                dict(top_p=-0.1), dict(top_p=1.5), dict(inv_temp=-1.0), dict(inv_temp=float("nan")),
                dict(allow=p, ld_allow=(V + 63) // 64 - 1), dict(allow=p + 4, ld_allow=(V + 63) // 64)):
        assert call(**bad) == 1, bad


BAD_ARGS = [dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=True), dict(top_p="0.9"),
            dict(seed=1.5), dict(seed=True), dict(seed="7")]


@pytest.mark.parametrize("kw", BAD_ARGS)
def test_client_rejects_bad_sampling_arguments_before_loading(kw):
    from vision_inspection_system_amd import client as C
    c = C.LocalVLMClient()
    # a model id that does not exist: a check after loading would raise FileNotFoundError instead
    with pytest.raises(ValueError) as e:
        c.chat.completions.create(model="/nonexistent/model-dir", messages=[{"role": "user", "content": "hi"}],
                                  max_tokens=4, temperature=1.0, **kw)
    msg = str(e.value).lower()
    assert not any(s in msg for s in RETRY_SUBSTRINGS), msg
    with pytest.raises(ValueError) as e:
        c.complete_many("/nonexistent/model-dir", [[{"role": "user", "content": "hi"}]], 1.0, 4, **kw)
    assert not any(s in str(e.value).lower() for s in RETRY_SUBSTRINGS)


def test_argument_checks():
    from vision_inspection_system_amd.sampling import check_seed, check_seeds, check_top_p, row_seed
    assert check_top_p(None) is None and check_top_p(0) == 0.0 and check_top_p(1) == 1.0 and check_top_p(0.9) == 0.9
    assert check_top_p(np.float32(0.5)) == 0.5
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "0.9", [0.9]):
        with pytest.raises(ValueError):
            check_top_p(bad)
    assert check_seed(None) is None and check_seed(7) == 7 and check_seed(-1) == -1 and check_seed(np.int64(3)) == 3
    for bad in (1.5, True, "7"):
        with pytest.raises(ValueError):
            check_seed(bad)
    assert check_seeds(None, 3) is None and check_seeds([1, 2, 3], 3) == [1, 2, 3]
    for bad in ([1, 2], [1, 2, "3"], [1, None, 3], "123", 5):
        with pytest.raises(ValueError):
            check_seeds(bad, 3)
    assert row_seed(-1) == 0xFFFFFFFF and row_seed(2 ** 32 + 5) == 5


@pytest.mark.parametrize("engine_mod,cls", [("engine", "Qwen2VLEngine"), ("mllama_engine", "MllamaEngine")])
def test_engines_check_sampling_arguments_first(engine_mod, cls):
    import importlib
    E = getattr(importlib.import_module(f"vision_inspection_system_amd.{engine_mod}"), cls)
    eng = E.__new__(E)           # no device state: the checks run before anything touches the GPU
    eng.max_batch = 4
    reqs = [([1, 2], None), ([3, 4], None)]
    for bad in (dict(top_p=1.5), dict(top_p=True), dict(seeds=[1]), dict(seeds=[1, 2.5]), dict(seeds=[True, 2]),
                dict(seeds="ab")):
        with pytest.raises(ValueError):
            eng.generate_batch(reqs, **bad)
    for bad in (-0.5, float("nan"), "1"):
        with pytest.raises(ValueError):
            eng.generate([1, 2], top_p=bad)


def test_canned_client_records_sampling_arguments():
    from vision_inspection_system_amd.client import CannedResponseClient
    c = CannedResponseClient("OK")
    c.chat.completions.create(model="m", messages=[], top_p=0.9, seed=7)
    c.chat.completions.create(model="m", messages=[])
    assert c.calls[0]["top_p"] == 0.9 and c.calls[0]["seed"] == 7
    assert c.calls[1]["top_p"] is None and c.calls[1]["seed"] is None


def test_agents_seed_switch(monkeypatch):
    from vision_inspection_system_amd import agents
    from vision_inspection_system_amd.client import CannedResponseClient
    monkeypatch.delenv("VIS_SEED", raising=False)
    assert agents.seed_kwargs() == {}
    monkeypatch.setenv("VIS_SEED", "")
    assert agents.seed_kwargs() == {}
    monkeypatch.setenv("VIS_SEED", "1234")
    assert agents.seed_kwargs() == {"seed": 1234}
    monkeypatch.setenv("VIS_SEED", "x")
    with pytest.raises(ValueError):
        agents.seed_kwargs()
    for env, want in ((None, None), ("42", 42)):
        if env is None:
            monkeypatch.delenv("VIS_SEED", raising=False)
        else:
            monkeypatch.setenv("VIS_SEED", env)
        agent = agents.VLMInspectorAgent.__new__(agents.VLMInspectorAgent)
        agent.client, agent.model_id, agent.temperature, agent.max_tokens = CannedResponseClient(reply="{}"), "m", 0.1, 64
        agent.logger = agents._logger("t")
        assert agent._call_with_retry([{"role": "user", "content": "x"}]) == "{}"
        assert agent.client.calls[-1]["seed"] == want
