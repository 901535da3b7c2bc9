"""CPU references for the image front end's row kernels (csrc/misc.hip): float64 and numpy only, never the library.

vis_patchify_u8 / vis_patchify_tiles_u8 write bf16((u / 255 - mean) / std) for a pixel level u and a channel: 768 distinct
values.  ``level_table`` holds, per (channel, level), the bf16 a correct kernel MUST write - round-to-nearest-even of the
float64 value - and the one or two it MAY write where that value lies within relative 2^-21 of a rounding boundary
(the kernel evaluates u * (1/255) - mean, times 1/std, in f32, with or without contraction: 1/255 and 1/std are each
rounded once, the two operations once each; 2^-21 = 8 f32 unit roundoffs covers them).  mean and std are the f32 numbers
the kernel receives.  At most AMBIGUOUS_CAP of the 768 values may be ambiguous (asserted on the CPU).

The layouts are restated with numpy reshapes, not with the kernels' index arithmetic."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
REL = 2.0 ** -21
AMBIGUOUS_CAP = 0.02
SENTINEL = 0x7FC1            # a quiet NaN with a payload bit: the fill of every bf16 output buffer, as int16


def bf16_bits(v):
    """float64 array -> bf16 bit patterns (uint16) by ONE round-to-nearest-even from float64 (normal range only)."""
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(v)                                   # |v| = m 2^e, m in [0.5, 1): 8 significant bits -> quantum 2^(e-8)
    q = np.ldexp(1.0, e - 8)
    r = np.round(v / q) * q                              # numpy rounds half to even; v / q and the product are exact
    f = r.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), r)
    bits = f.view(np.uint32)
    assert not (bits & 0xFFFF).any()
    return (bits >> 16).astype(np.uint16)


def level_table(mean=CLIP_MEAN, std=CLIP_STD):
    """(must, lo, hi): three [3, 256] uint16 tables; a value is ambiguous where lo != hi, and then must is one of them."""
    m = np.asarray(mean, dtype=np.float32).astype(np.float64)[:, None]
    s = np.asarray(std, dtype=np.float32).astype(np.float64)[:, None]
    v = (np.arange(256, dtype=np.float64)[None, :] / 255.0 - m) / s
    a, b = bf16_bits(v * (1 - REL)), bf16_bits(v * (1 + REL))
    return bf16_bits(v), np.minimum(a, b), np.maximum(a, b)


def ambiguous_share(table):
    _, lo, hi = table
    return float((lo != hi).mean())


def check_levels(got_bits, levels, channels, table, what=""):
    """got_bits: uint16 array; levels / channels: same-shape integer arrays naming the pixel level and channel behind
    each element.  Bit-equal to the must-table, or to lo / hi where the value is ambiguous."""
    must, lo, hi = (t[channels, levels] for t in table)
    ok = (got_bits == must) | (got_bits == lo) | (got_bits == hi)
    if not ok.all():
        i = tuple(int(k[0]) for k in np.nonzero(~ok))
        raise AssertionError(f"{what}: {int((~ok).sum())} wrong elements; first at {i}: level {int(levels[i])} channel "
                             f"{int(channels[i])} got {int(got_bits[i]):#06x} want {int(must[i]):#06x}")


def qwen_layout(a):
    """[H, W, 3] -> [patches, 1176] in the order of the Qwen2-VL processor: channel-first, 14 x 14 patches, 2 x 2 merge
    groups, the temporal pair (both copies the same frame).  The reshape of tests/test_kernels_gpu.py."""
    H, W, _ = a.shape
    gh, gw = H // 14, W // 14
    x = a.transpose(2, 0, 1)
    p = x.reshape(3, gh // 2, 2, 14, gw // 2, 2, 14).transpose(1, 4, 2, 5, 0, 3, 6)
    return np.broadcast_to(p[:, :, :, :, :, None], (*p.shape[:5], 2, 14, 14)).reshape(gh * gw, 1176)


def channel_image(H, W):
    return np.broadcast_to(np.arange(3, dtype=np.int64), (H, W, 3))


def tiles_layout(a, tiles_h, tiles_w, tile):
    """[tiles_h * tile, tiles_w * tile, 3] canvas -> [tiles, (tile / 14)^2, 588]: tiles row-major, patches row-major inside
    a tile, features (channel, row in patch, column in patch)."""
    G = tile // 14
    p = a.reshape(tiles_h, G, 14, tiles_w, G, 14, 3).transpose(0, 3, 1, 4, 6, 2, 5)
    return p.reshape(tiles_h * tiles_w, G * G, 588)
