"""Draw-exact tests of the five pick entry points on MI355X against tests/pick_exact.py: which token a given (seed, step,
row) must produce, masks, the nucleus cut record, the step >= max_tokens rule and the all-NaN row.

Every launch starts from sentinels (tokens = -1, cur_token = -1, nkeep = -1, NaN / 0xFF workspaces) and every test checks
tokens[step], cur_token, step + 1 and that no other token slot was touched.  A decisive draw (one candidate) must match
exactly; an ambiguous one (<= 1 % of any entry, tests/test_pick_exact.py) passes when the pick is among its candidates.
No tolerance here comes from the kernels' output."""
import numpy as np
import pytest
import torch

import pick_exact as P
from vision_inspection_system_amd import hip

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(autouse=True)
def _needs_gpu(device):
    """Every test here runs on the GPU (the device fixture skips without one)."""


def _dev_logits(logits, pad):
    """[B, V] device view; pad: rows 5 floats apart more than V, +inf in between (ld_logits = V + 5)."""
    B, V = logits.shape
    if not pad:
        return torch.from_numpy(logits).cuda()
    buf = torch.full((B, V + 5), float("inf"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.from_numpy(logits).cuda()
    return buf[:, :V]


def _dev_words(words):
    return None if words is None else torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def _i32(a, B=None):
    t = torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.int32)).cuda()
    return t if B is None else t.expand(B).contiguous()


def _check_picks(name, expected, curs, steps, tokens, start):
    """expected [S][B] candidate arrays; curs, steps [S, B] (cur_token and the step counter after launch s); tokens [B, T_TOK]
    after the last launch; start [B]."""
    S, B = curs.shape
    want = np.full((B, P.T_TOK), -1, dtype=np.int64)
    for s in range(S):
        for b in range(B):
            cand, pick = expected[s][b], int(curs[s, b])
            assert pick in cand.tolist(), (name, "launch", s, "row", b, "pick", pick, "candidates", cand.tolist()[:8])
            assert int(steps[s, b]) == int(start[b]) + s + 1, (name, s, b)
            if int(start[b]) + s < P.T_TOK:
                want[b, int(start[b]) + s] = pick
    assert (tokens.reshape(B, P.T_TOK) == want).all(), (name, "token slots")


def _run_argmax(c):
    x, allow, B = _dev_logits(c.logits, c.pad), _dev_words(c.words), c.B
    tokens = torch.full((B, P.T_TOK), -1, dtype=torch.int32, device="cuda")
    cur = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    step = _i32([c.start], B)
    wv = torch.empty(256 * B, dtype=torch.float32, device="cuda")
    wi = torch.empty(256 * B, dtype=torch.int32, device="cuda")
    curs, steps = [], []
    for _ in range(P.STEPS):
        wv.fill_(NAN); wi.fill_(-1); cur.fill_(-1)
        if allow is None:
            hip.argmax(x, wv, wi, tokens, cur, step, c.T, c.seed)
        else:
            hip.argmax_masked(x, wv, wi, tokens, cur, step, allow, c.T, c.seed)
        curs.append(cur.clone()); steps.append(step.clone())
    _check_picks(c.name, c.expected, torch.stack(curs).cpu().numpy(), torch.stack(steps).cpu().numpy(), tokens.cpu().numpy(),
                 np.full(B, c.start))


@pytest.mark.parametrize("V", P.VS_ARGMAX + (152064,))
def test_argmax(V):
    """(a) vis_argmax_f32: one workgroup / many / the 256-workgroup cap and the second grid-stride trip; B in {1, 3, 64}; every
    temperature; 8 consecutive steps from 0, 5 (steps 8.. store no token) and 2^31 - 9; wrapping row seeds; ld_logits = V + 5
    with +inf padding; Gaussian, tied, constant, -inf-holding, all -inf (lowest id) and all-NaN (id 0) rows."""
    for c in P.argmax_cases(V):
        _run_argmax(c)


@pytest.mark.parametrize("V", P.VS_ARGMAX + (152064,))
def test_argmax_masked(V):
    """(b) vis_argmax_masked_f32 on the same tables: random 10 %, the last id alone, live bits past V in the last word,
    alternating whole words, an empty row (id 0)."""
    for c in P.argmax_cases(V, True):
        _run_argmax(c)


def _run_gemv(c, x_override=None):
    N = c.N
    x = torch.from_numpy(c.x if x_override is None else x_override).to(torch.bfloat16).cuda()
    W = torch.from_numpy(c.W).to(torch.bfloat16).cuda()
    assert (W.float().cpu().numpy() == c.W).all()                     # the table's weights are bf16 values
    nw = None if c.norm_w is None else torch.from_numpy(c.norm_w).to(torch.bfloat16).cuda()
    allow = None if c.words is None else _dev_words(c.words)
    logits = torch.empty(N, dtype=torch.float32, device="cuda")
    wv = torch.empty(2048, dtype=torch.float32, device="cuda")
    wi = torch.empty(2048, dtype=torch.int32, device="cuda")
    tokens = torch.full((P.T_TOK,), -1, dtype=torch.int32, device="cuda")
    cur = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    step = _i32([c.start])
    curs, steps, outs = [], [], []
    for _ in range(P.GEMV_STEPS):
        logits.fill_(NAN); wv.fill_(NAN); wi.fill_(-1); cur.fill_(-1)
        if allow is None:
            hip.gemv_argmax(x, W, logits, wv, wi, tokens, cur, step, norm_w=nw, temperature=c.T, seed=c.seed)
        else:
            hip.gemv_argmax_masked(x, W, logits, wv, wi, tokens, cur, step, allow, norm_w=nw, temperature=c.T, seed=c.seed)
        curs.append(cur.clone()); steps.append(step.clone()); outs.append(logits.clone())
    outs = torch.stack(outs).cpu().numpy()
    assert (outs.view(np.int32) == outs[0].view(np.int32)).all(), (c.name, "logits differ between launches")
    return outs[0], torch.stack(curs).cpu().numpy(), torch.stack(steps).cpu().numpy(), tokens.cpu().numpy()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N", P.NS_GEMV)
def test_gemv_argmax(N, masked):
    """(c) vis_gemv_bf16_argmax(_masked), K = 64: the reference's input is the f32 logits the launch wrote.  Distinct logits
    and planted exact ties (identical weight rows in one pair, two waves, two workgroups), odd N, both grid rules, with and
    without the fused norm, T in {0, 0.7}, the masks of (b) and the odd last row alone."""
    for c in P.gemv_cases(N, masked):
        got, curs, steps, tokens = _run_gemv(c)
        expected = c.expected if np.array_equal(got, c.logits) else c.expected_for(got)
        _check_picks(c.name, expected, curs, steps, tokens, np.array([c.start]))
        # the table's weights make every product and sum exact in f32: the logits are the ones its ambiguity cap was taken on
        assert np.array_equal(got, c.logits), (c.name, "logits", np.flatnonzero(got != c.logits)[:8])


@pytest.mark.parametrize("masked", [False, True])
def test_gemv_argmax_all_nan_row_picks_id_0(masked):
    """A NaN in x makes every logit NaN: nothing comparable, the pick is id 0 (never the 0x7fffffff sentinel)."""
    c = P.gemv_cases(513, masked)[2 if not masked else 0]
    x = c.x.copy()
    x[5] = np.nan
    got, curs, steps, tokens = _run_gemv(c, x)
    assert np.isnan(got).all()
    zero = [[np.zeros(1, dtype=np.int64)] for _ in range(P.GEMV_STEPS)]
    _check_picks(c.name + "-nan", zero, curs, steps, tokens, np.array([c.start]))


def _run_sample(c):
    x, allow, B = _dev_logits(c.logits, c.pad), _dev_words(c.words), c.B
    tokens = torch.full((B, P.T_TOK), -1, dtype=torch.int32, device="cuda")
    cur = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    step = _i32(c.steps)
    seeds = torch.from_numpy(c.seeds.view(np.int32).copy()).cuda()
    nkeep = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ws = hip.sample_ws(c.V, B, "cuda")
    ws.fill_(0xFF)
    hip.sample(x, tokens, cur, step, seeds, ws, c.T, c.p, allow=allow, nkeep=nkeep)
    rec = np.ascontiguousarray(ws.cpu().numpy()[:, :8])
    cut_v, cut_i = rec[:, :4].copy().view(np.float32)[:, 0], rec[:, 4:].copy().view(np.int32)[:, 0]
    nk, picks = nkeep.cpu().numpy(), cur.cpu().numpy()
    expected = []
    for b, nu in enumerate(c.nucleus):
        what = (c.name, "row", b, c.kinds[b], c.mask_kinds[b] if c.mask_kinds else "")
        n = int(nk[b])
        assert nu.n_lo <= n <= nu.n_hi, what + ("nkeep", n, nu.n_lo, nu.n_hi)
        if nu.exact:
            assert n == nu.n_lo, what
        if nu.open:
            assert cut_v[b] == -np.inf and int(cut_i[b]) == P.NO_ID, what + ("open cut", cut_v[b], cut_i[b])
        else:
            at = int(nu.order[n - 1])
            assert int(cut_i[b]) == at and cut_v[b] == c.logits[b, at], what + ("cut", cut_v[b], cut_i[b], at)
        cand = c.pick_candidates(b, n)
        assert not np.isnan(c.logits[b, cand]).any() or nu.order.size == 0, what
        expected.append(cand)
    _check_picks(c.name, [expected], picks[None], step.cpu().numpy()[None], tokens.cpu().numpy(), c.steps)


@pytest.mark.parametrize("V", P.VS_SAMPLE + (152064,))
def test_sample(V):
    """(d) vis_sample_f32: the cut record (v*, i*) is the element at position nkeep - 1 of the (logit desc, id asc) order,
    nkeep lies in [n_lo, n_hi] (equal to the integer emulation on the exact-weight rows: tie groups below, at and above the
    1024-member LDS limit), the pick is a candidate of the Gumbel-max over exactly that prefix with seeds[b] and step[b];
    (-inf, 0x7fffffff) at top_p = 1.  Two-level rows cut inside the lower tie group, a tie group straddling the cut, Gaussian
    rows, rows with -inf and NaN entries, the masks of (b)."""
    for c in P.sample_cases(V):
        _run_sample(c)


def test_five_entry_points_agree_with_the_model():
    """(e) one row at T = 0.7 through all five entry points: each must give the MODEL's pick (for vis_sample_f32: top_p = 1 and
    the row seed), masked ones the model's pick over the mask."""
    c = P.gemv_cases(8191)[2]
    assert c.T == 0.7 and c.norm_w is None
    L, curs, steps, tokens = _run_gemv(c)
    _check_picks(c.name, c.expected_for(L), curs, steps, tokens, np.array([c.start]))
    rng = np.random.default_rng(5)
    words = P.mask_words("lastword", c.N, rng)
    free = P.candidates(L, c.inv_temp, c.seed, c.start, np.arange(c.N))
    words[int(free[0]) // 64] &= ~np.uint64(1 << (int(free[0]) % 64))       # the mask forbids the unmasked pick
    ids = {False: np.arange(c.N), True: P.allowed_ids(words, c.N)}
    model = {m: P.candidates(L, c.inv_temp, c.seed, c.start, ids[m]) for m in (False, True)}
    assert len(model[False]) == 1 and len(model[True]) == 1 and model[False][0] != model[True][0], "pick another table row"
    assert int(curs[0, 0]) == model[False][0]
    cm = P.GemvCase(c.name + "-masked", c.N, c.T, c.start, c.seed, c.x, c.W, None, c.logits, c.tie, words, "lastword")
    Lm, curs, steps, tokens = _run_gemv(cm)
    assert np.array_equal(Lm, L) and int(curs[0, 0]) == model[True][0]
    ac = P.ArgmaxCase("entry-argmax", c.N, 1, c.T, c.start, c.seed, True, L[None], ("gemv",))
    am = P.ArgmaxCase("entry-argmax-masked", c.N, 1, c.T, c.start, c.seed, False, L[None], ("gemv",), words[None], ("lastword",))
    assert ac.expected[0][0].tolist() == model[False].tolist() and am.expected[0][0].tolist() == model[True].tolist()
    _run_argmax(ac)
    _run_argmax(am)
    for masked in (False, True):
        sc = P.SampleCase("entry-sample", c.N, 1, c.T, 1.0, masked, L[None], ("gemv",), np.array([c.seed], dtype=np.uint32),
                          np.array([c.start], dtype=np.int32), words[None] if masked else None, ("lastword",) if masked else ())
        assert sc.nucleus[0].open and sc.pick_candidates(0, sc.nucleus[0].n_lo).tolist() == model[masked].tolist()
        _run_sample(sc)
