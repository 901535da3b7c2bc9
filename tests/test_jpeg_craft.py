"""Crafted-JPEG parity on the CPU: files written coefficient by coefficient (tests/jpeg_craft.py) - DC at the format's
limits, sparse blocks with large AC terms, samples on either side of every limit a range-limit rule cares about,
saturated chroma under every subsampling - through csrc/jpeg_host.c + oracle/jpeg_ref.py against PIL's decode of the
same bytes.  PIL-written files (tests/test_jpeg.py) never leave the interval [-512, 511] in which all libjpeg range
limits agree; these do.

The rule pinned here: the split decoder saturates (clamp(x + 128, 0, 255), what libjpeg-turbo's SIMD inverse DCT does and
plain C libjpeg's 10-bit mask does not) and accepts a stream only while T = sum g[u] |coef q| <= 8000 in every block
(derivation: csrc/jpeg_host.c, RANGE_LIMIT), which keeps every 16-bit intermediate of the SIMD code inside int16;
anything above is declined with reason "range" and takes the PIL path.  Plain saturation alone is NOT PIL's rule: it
misses PIL on crafted files whose column pass fits int16 (a 16-bit sum of two such values wraps), which is why the bound
is on the sums and not only on the values.  ``test_crafted_survey`` prints the counts.

Also here: the stand-alone AddressSanitizer + UBSan sweep of the host parser (tests/jpeg_host_sweep.c)."""
import io
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as JC
import test_jpeg
from oracle import jpeg_ref as R
from vision_inspection_system_amd import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = JC.crafted_cases()
GAIN = np.array([1024, 1421, 1339, 1421, 1024, 1421, 1339, 1421], dtype=np.int64)    # csrc/jpeg_host.c, restated
LIMIT = 8000 * 1024


def pil_rgb(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def weighted_sum_max(coeffs_by_comp, qts):
    """max over blocks of 1024 T = sum GAIN[u] |coef| q, u = vertical frequency (natural index >> 3)."""
    m = 0
    for c, q in zip(coeffs_by_comp, qts):
        x = np.abs(np.asarray(c, dtype=np.int64).reshape(-1, 8, 8)) * np.asarray(q, dtype=np.int64).reshape(8, 8)
        m = max(m, int((x * GAIN[None, :, None]).sum(axis=(1, 2)).max()))
    return m


@lru_cache(maxsize=None)
def survey(i):
    case = CASES[i]
    jc, reason = J.parse_status(case.data)
    return {"case": case, "jc": jc, "reason": reason, "domain": case.domain(),
            "t1024": weighted_sum_max(case.coeffs, case.qts), "pil": pil_rgb(case.data)}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_crafted_file_is_decoded_like_pil_or_declined_for_range(i):
    s = survey(i)
    case, jc, d = s["case"], s["jc"], s["domain"]
    assert s["pil"].shape == (case.height, case.width, 3)            # PIL takes every crafted file: the fallback exists
    if d["in_range"]:
        assert s["reason"] == "ok", "a file inside [-512, 511] must stay on the split path"
    if not (d["deq_int16"] and d["col_int16"]):
        assert s["reason"] == "range", "beyond the int16 conditions decoders disagree: must be declined"
    if jc is None:
        assert s["reason"] == "range" and s["t1024"] > LIMIT and not d["in_range"], (s["reason"], s["t1024"], d)
        return
    assert s["t1024"] <= LIMIT and d["deq_int16"] and d["col_int16"]
    # the parser returns exactly what the builder put in (this also pins the builder)
    assert jc.size == (case.width, case.height) and jc.ncomp == len(case.coeffs)
    assert np.array_equal(jc.coeffs.astype(np.int64), np.concatenate(case.coeffs))
    assert all(np.array_equal(jc.qt[c].astype(np.int64), case.qts[c]) for c in range(jc.ncomp))
    got = R.decode(jc.as_dict(), jc.coeffs)
    assert np.array_equal(got, s["pil"]), f"sample range [{d['min']}, {d['max']}]"


def test_crafted_survey():
    """Every crafted file is either decoded by the split path (bit-equal to PIL, the test above) or declined with reason
    "range": none escapes, so the 80 % floor on handled out-of-range files holds with room.  The set really contains
    what it is for: files in range, out of range, beyond each int16 condition, and samples at every limit."""
    rows = [survey(i) for i in range(len(CASES))]
    inr = [r for r in rows if r["domain"]["in_range"]]
    out = [r for r in rows if not r["domain"]["in_range"]]
    out_dec = [r for r in out if r["jc"] is not None]
    out_decl = [r for r in out if r["jc"] is None and r["reason"] == "range"]
    int16 = [r for r in out if r["domain"]["deq_int16"] and r["domain"]["col_int16"]]
    int16_decl = [r for r in int16 if r["jc"] is None]
    print(f"crafted files: {len(rows)}; in range {len(inr)}; out of range {len(out)} = {len(out_dec)} decoded by the "
          f"split path + {len(out_decl)} declined (range); out of range with both int16 conditions: {len(int16)}, "
          f"of which declined {len(int16_decl)}; beyond dequantised int16: "
          f"{sum(not r['domain']['deq_int16'] for r in rows)}, beyond column-pass int16: "
          f"{sum(not r['domain']['col_int16'] for r in rows)}")
    assert len(out_dec) + len(out_decl) == len(out)
    assert (len(out_dec) + len(out_decl)) >= 0.8 * len(out)
    assert len(inr) >= 50 and len(out_dec) >= 20 and len(out_decl) >= 20
    assert any(not r["domain"]["deq_int16"] for r in rows) and any(not r["domain"]["col_int16"] for r in rows)
    for level in (-512, -129, -128, 127, 128, 511, 512):           # both sides of every limit are among the extremes
        for side in (level - 1, level, level + 1):
            assert any(side in (r["domain"]["min"], r["domain"]["max"]) for r in rows), side
    sizes = {(r["case"].width, r["case"].height) for r in rows}
    assert sizes >= {(8, 8), (16, 16), (17, 9), (1, 1), (33, 17)}
    assert {r["case"].layout for r in rows} == {"grey", "444", "422", "420"}


def test_the_bound_is_where_the_code_says():
    """DC-only, quantiser 4: T = 4 |dc| exactly (g[0] = 1).  8000 is accepted, 8004 is declined."""
    for dc, want in ((2000, "ok"), (-2000, "ok"), (2001, "range"), (-2001, "range")):
        b = [np.zeros((1, 1, 64), dtype=np.int64)]
        b[0][0, 0, 0] = dc
        data = JC.build(8, 8, "grey", b, [[4] * 64])
        jc, reason = J.parse_status(data)
        assert reason == want, (dc, reason)
        if jc is not None:
            assert np.array_equal(R.decode(jc.as_dict(), jc.coeffs), pil_rgb(data))
    # an odd vertical frequency weighs 1421/1024: natural index 8 (zig-zag 2), quantiser 8 -> T = 1.3877 * 8 |c|
    for c, want in ((720, "ok"), (721, "range")):
        b = [np.zeros((1, 1, 64), dtype=np.int64)]
        b[0][0, 0, 2] = c
        assert (1421 * 8 * c <= LIMIT) == (want == "ok")
        assert J.parse_status(JC.build(8, 8, "grey", b, [[8] * 64]))[1] == want


def test_pil_written_files_stay_on_the_split_path():
    """The decline rule must not switch the GPU path off for photographs: every PIL-written test image is accepted, and
    the largest T among them (q85 noise) is about half the limit."""
    worst = 0
    for name, data in test_jpeg.cases():
        jc, reason = J.parse_status(data)
        assert reason == "ok" and jc is not None, name
        o, per = 0, []
        for c in range(jc.ncomp):
            n = jc.bw[c] * jc.bh[c]
            per.append(jc.coeffs[o:o + n])
            o += n
        worst = max(worst, weighted_sum_max(per, [jc.qt[c] for c in range(jc.ncomp)]))
    print(f"largest T among the PIL-written files: {worst / 1024:.0f} (limit 8000)")
    assert worst <= 0.75 * LIMIT


def test_parse_status_names_the_other_reasons():
    img = Image.fromarray(test_jpeg._smooth(np.random.default_rng(3), 24, 40))
    b = io.BytesIO()
    img.save(b, format="JPEG", progressive=True)
    assert J.parse_status(b.getvalue()) == (None, "unsupported")
    good = test_jpeg.jpeg_bytes(img, quality=85)
    assert J.parse_status(good[:len(good) // 2]) == (None, "corrupt")
    assert J.parse_status(b"no") == (None, "corrupt")
    jc, reason = J.parse_status(good)
    assert reason == "ok" and jc.size == (40, 24)


# ------------------------------------------------------------------------------------------------ sanitizer sweep
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]    # gcc: the runtime inside the program, whatever the loader adds


def test_host_parser_sanitizer_sweep(tmp_path):
    """csrc/jpeg_host.c parses bytes from the network.  Built stand-alone with ASan + UBSan (tests/jpeg_host_sweep.c has
    the main) and run as a child process over every prefix, single-byte substitution and deletion and 20 000 random
    mutations of six small files: exit status 0 means no out-of-bounds access, no undefined behaviour."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for flags in (SAN_FLAGS + STATIC_RUNTIME, SAN_FLAGS):
        ok = subprocess.run([cc, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if ok.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the C compiler lacks the address/undefined sanitizers: " + ok.stderr[-200:])
    exe = tmp_path / "jpeg_host_sweep"
    subprocess.run([cc, *flags, "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "jpeg_host_sweep.c"),
                    os.path.join(os.path.dirname(os.path.abspath(J.__file__)), "csrc", "jpeg_host.c"), "-o", str(exe)],
                   check=True)
    rgb = test_jpeg._smooth(np.random.default_rng(11), 24, 40)
    files = {"s444.jpg": dict(subsampling=0), "s420.jpg": dict(subsampling=2),
             "s422r.jpg": dict(subsampling=1, restart_marker_blocks=2)}
    paths = []
    for name, kw in files.items():
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, format="JPEG", quality=85, **kw)
        (tmp_path / name).write_bytes(b.getvalue())
        paths.append(str(tmp_path / name))
    b = io.BytesIO()
    Image.fromarray(rgb[..., 0]).save(b, format="JPEG", quality=85)
    (tmp_path / "grey.jpg").write_bytes(b.getvalue())
    paths.append(str(tmp_path / "grey.jpg"))
    by_name = {c.name: c for c in CASES}
    for k, name in enumerate(("sparse 2 422 17x9 q4", "chroma +1-1 420 33x17")):    # one declined for range, one decoded
        (tmp_path / f"craft{k}.jpg").write_bytes(by_name[name].data)
        paths.append(str(tmp_path / f"craft{k}.jpg"))
    run = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=600)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stderr[-3000:]
    counts = dict(kv.split("=") for kv in run.stdout.split())
    assert int(counts["files"]) == 6 and int(counts["decoded"]) > 0 and int(counts["range"]) > 0
    assert int(counts["ok"]) == int(counts["decoded"]) + int(counts["range"]) + int(counts["decode_corrupt"])
