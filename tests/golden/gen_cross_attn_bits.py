"""Generator of tests/golden/cross_attn_bits.json: the output bits of the six decode-step cross-attention entry points
(vis_decode_cross_attn, _batch, _draft and their _fp8 forms) as one build of the library computes them.

Needs an MI355X.  Run it with VIS_HIP_LIB pointing at a build of the commit whose bits are to be pinned (hip.py's A/B
switch); tests/test_cross_attn_bits_gpu.py rebuilds the same inputs through this module and compares the library under test
against the file.  Re-run it, on purpose, only when a change is meant to alter what these kernels compute.

Inputs are seeded integer draws that every format holds exactly: q and bf16 K / V are integers in [-8, 8] times 2^-2, the
q_norm weight is an integer in [1, 3] times 2^-1, fp8 codes are uniform bytes with the two NaN codes replaced by 0x38, scales
are integers in [1, 3] times 2^-9 (K) or 2^-7 (V).  Rows at or past the key count hold poison: NaN rows (bf16), code 0x7F and
inf scales (fp8).  q is always the leading Hq * 128 columns of packed rows of (Hq + 2 Hkv) * 128, the batch forms read K / V
as layer 1 of a [B, 2, ...] buffer (a batch stride that skips a layer), the workspaces and the output start as NaN.

Per launch the file keeps the sha256 of the concatenated input bytes, of ``out``, and of the ``part_o`` / ``part_ml`` slots of
the splits that ran (ceil(count / 64) per sequence; the other slots are stale by contract).  The streaming form of the bf16
batch (VIS_DECODE_ATTN_STREAM=2) writes no partials: ``out`` alone.

Usage:  python tests/golden/gen_cross_attn_bits.py [--out FILE] [--commit HASH]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS, SCALE = 1e-5, 128 ** -0.5
T_KEYS = 192                                        # three splits of 64 keys, the last one ragged for most counts
COUNTS = (1, 64, 65, 191, 192)
HEADS = [(1, 1), (2, 1), (8, 2), (7, 1), (8, 1)]    # every instantiated group size; G = 7, 8: only two draft rows fit
BATCH = 3
STREAM_ENV = "VIS_DECODE_ATTN_STREAM"


def cases() -> list:
    """(id, fmt, Hq, Hkv, form, stream): ``stream`` is the value of VIS_DECODE_ATTN_STREAM for the bf16 batch form, else None."""
    out = []
    for fmt in ("bf16", "fp8"):
        for Hq, Hkv in HEADS:
            out.append((f"{fmt}-{Hq}x{Hkv}-single", fmt, Hq, Hkv, "single", None))
            for st in (("0", "2") if fmt == "bf16" else (None,)):
                out.append((f"{fmt}-{Hq}x{Hkv}-batch" + (f"-stream{st}" if st else ""), fmt, Hq, Hkv, "batch", st))
            out.append((f"{fmt}-{Hq}x{Hkv}-draft", fmt, Hq, Hkv, "draft", None))
    return out


def _seed(fmt, Hq, Hkv, form) -> int:
    return 100000 * ("bf16", "fp8").index(fmt) + 1000 * Hq + 10 * Hkv + ("single", "batch", "draft").index(form)


def _kv(rng, fmt, Hkv, count):
    """The static keys / values of one sequence in ``fmt`` as numpy arrays (bf16 values as float32)."""
    if fmt == "bf16":
        k = rng.integers(-8, 9, (Hkv, T_KEYS, 128)).astype(np.float32) * 0.25
        v = rng.integers(-8, 9, (Hkv, T_KEYS, 128)).astype(np.float32) * 0.25
        k[:, count:], v[:, count:] = np.nan, np.nan
        return [k, v]

    def codes():
        c = rng.integers(0, 256, size=(Hkv, T_KEYS, 128)).astype(np.uint8)
        c[(c & 0x7F) == 0x7F] = 0x38                          # no NaN code among the live rows
        c[:, count:] = 0x7F
        return c
    kq, vq = codes(), codes()
    ksc = rng.integers(1, 4, (Hkv, T_KEYS)).astype(np.float32) * np.float32(2.0 ** -9)
    vsc = rng.integers(1, 4, (Hkv, T_KEYS)).astype(np.float32) * np.float32(2.0 ** -7)
    ksc[:, count:], vsc[:, count:] = np.inf, np.inf
    return [kq, ksc, vq, vsc]


def _bytes(t) -> bytes:
    t = t.detach().contiguous().cpu()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(_bytes(t))
    return h.hexdigest()


def _ran(part, seqs, Hq, ns, width, counts):
    """The slots of the splits that ran, sequence by sequence: [seq][Hq][: ceil(count / 64)][width]."""
    p = part.view(seqs, Hq, ns, width)
    return [p[s, :, :-(-counts[s] // 64)] for s in range(seqs)]


def _launches(fmt, Hq, Hkv, form):
    """Yields (sub-id, rows or batch, counts, numpy inputs) for every launch of a case, in a fixed order."""
    rng = np.random.default_rng(_seed(fmt, Hq, Hkv, form))
    nq = (Hq + 2 * Hkv) * 128
    w = rng.integers(1, 4, 128).astype(np.float32) * 0.5
    if form == "batch":
        counts = [int(c) for c in rng.choice(COUNTS, BATCH)]
        qbuf = rng.integers(-8, 9, (BATCH, nq)).astype(np.float32) * 0.25
        per_seq = [_kv(rng, fmt, Hkv, c) for c in counts]
        # [B, 2 layers, ...]: layer 0 is filler of the same kind, the launch reads layer 1
        kv = [np.stack([np.stack([np.zeros_like(s[i]), s[i]]) for s in per_seq]) for i in range(len(per_seq[0]))]
        yield "b3", BATCH, counts, qbuf, w, kv
        return
    G = Hq // Hkv
    for count in COUNTS:
        qbuf = rng.integers(-8, 9, (4, nq)).astype(np.float32) * 0.25
        kv = _kv(rng, fmt, Hkv, count)
        if form == "single":
            yield f"n{count}", 1, [count], qbuf, w, kv
        else:
            for R in range(1, 5):
                if R * G <= 16:
                    yield f"n{count}-r{R}", R, [count] * R, qbuf, w, kv


def run_case(hip, device, fmt, Hq, Hkv, form, stream) -> dict:
    """Every launch of one case on the loaded library -> {sub-id: {"in", "out"[, "part_o", "part_ml"]}} of sha256 digests."""
    ns = T_KEYS // hip.DECODE_KEYS_PER_SPLIT
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).to(device)
    res = {}
    for sub, n, counts, qbuf, w, kv in _launches(fmt, Hq, Hkv, form):
        qd, wd = bf(qbuf), bf(w)
        kvd = [bf(a) if a.dtype == np.float32 and fmt == "bf16" else torch.from_numpy(a).to(device) for a in kv]
        nk = torch.tensor([c - 1 for c in (counts if form == "batch" else counts[:1])], dtype=torch.int32, device=device)
        part_o = torch.full((n * Hq * ns * 128,), float("nan"), dtype=torch.float32, device=device)
        part_ml = torch.full((n * Hq * ns * 2,), float("nan"), dtype=torch.float32, device=device)
        out = torch.full((n, Hq * 128), float("nan"), dtype=torch.bfloat16, device=device)
        tail = (nk, part_o, part_ml, out, Hq, Hkv, 128, ns, SCALE, EPS)
        sfx = "" if fmt == "bf16" else "_fp8"
        if form == "single":
            getattr(hip, "decode_cross_attn" + sfx)(qd[0, :Hq * 128].contiguous(), wd, *kvd, nk, part_o, part_ml, out[0], *tail[4:])
        elif form == "draft":
            getattr(hip, "decode_cross_attn" + sfx + "_draft")(qd[:n, :Hq * 128], wd, *kvd, *tail)
        else:
            old = os.environ.get(STREAM_ENV)
            if stream is not None:
                os.environ[STREAM_ENV] = stream
            try:
                getattr(hip, "decode_cross_attn" + sfx + "_batch")(qd[:, :Hq * 128], wd, *[t[:, 1] for t in kvd], *tail)
            finally:
                if stream is not None:
                    if old is None:
                        del os.environ[STREAM_ENV]
                    else:
                        os.environ[STREAM_ENV] = old
        torch.cuda.synchronize()
        rec = {"in": _sha(qd, wd, *kvd, nk), "out": _sha(out)}
        if stream != "2":
            rec["part_o"] = _sha(*_ran(part_o, n, Hq, ns, 128, counts))
            rec["part_ml"] = _sha(*_ran(part_ml, n, Hq, ns, 2, counts))
        res[sub] = rec
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "cross_attn_bits.json"))
    ap.add_argument("--commit", default=None, help="the commit the loaded library was built from")
    a = ap.parse_args()
    from vision_inspection_system_amd import hip
    hip.load()
    device = torch.device("cuda:0")
    doc = {"commit": a.commit, "library": "VIS_HIP_LIB" if os.environ.get("VIS_HIP_LIB") else "csrc/libvis_hip.so",
           "key_tokens": T_KEYS, "counts": list(COUNTS), "cases": {}}
    for cid, fmt, Hq, Hkv, form, stream in cases():
        doc["cases"][cid] = run_case(hip, device, fmt, Hq, Hkv, form, stream)
        print(cid, len(doc["cases"][cid]), "launches", flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
