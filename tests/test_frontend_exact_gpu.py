"""The image front end's row kernels (csrc/misc.hip), exactly: vis_patchify_u8, vis_patchify_tiles_u8, vis_gather_rows,
vis_scatter_rows, vis_add_rows_bf16.  References are built on the CPU (tests/frontend_exact.py); outputs are compared
as bit patterns; every output buffer is pre-filled with a NaN sentinel so that a skipped or a stray store shows."""
import ctypes

import numpy as np
import pytest
import torch

import frontend_exact as F

TABLE = F.level_table()
gpu = pytest.mark.gpu


def test_level_table_is_almost_everywhere_unambiguous():
    """CPU: at most 2 % of the 768 (level, channel) values may sit within 2^-21 of a bf16 rounding boundary (today none
    does), the padded level 0 never, and the bf16 rounding helper agrees with torch's on exact f32 inputs."""
    share = F.ambiguous_share(TABLE)
    print(f"ambiguous patchify values: {share * 768:.0f} of 768 ({share:.2%})")
    assert share <= F.AMBIGUOUS_CAP
    assert (TABLE[1][:, 0] == TABLE[2][:, 0]).all()
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]                      # ties: to even, both directions; zero
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(F.bf16_bits(x.astype(np.float64)), want)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _sentinel(shape, device):
    return torch.full(shape, F.SENTINEL, dtype=torch.int16, device=device).view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------- vis_patchify_u8
@gpu
@pytest.mark.parametrize("H,W,row0,ld", [(28, 28, 0, 1176), (28, 2800, 0, 1216), (2800, 28, 0, 1280), (56, 84, 7, 1216),
                                         (56, 84, 7, 1176), (1176, 1176, 0, 1216)])
def test_patchify_is_bit_exact(device, H, W, row0, ld):
    """1176 x 1176 at ld_out 1216: 7056 patches x 152 chunks > 4096 blocks x 256 items - the grid-stride loop iterates."""
    assert (H, W) != (1176, 1176) or (H // 14) * (W // 14) * (ld // 8) > 4096 * 256
    from vision_inspection_system_amd import hip
    rng = np.random.default_rng(H * 10007 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.reshape(-1)[:256] = np.arange(256)                              # every level occurs, whatever the draw
    n = (H // 14) * (W // 14)
    tail = 5
    out = _sentinel((row0 + n + tail, ld), device)
    hip.patchify(torch.from_numpy(img).to(device), out, row0, F.CLIP_MEAN, F.CLIP_STD)
    got = _bits(out)
    assert (got[:row0] == F.SENTINEL).all() and (got[row0 + n:] == F.SENTINEL).all()       # rows before and after
    body = got[row0:row0 + n]
    F.check_levels(body[:, :1176], F.qwen_layout(img.astype(np.int64)), F.qwen_layout(F.channel_image(H, W)), TABLE,
                   f"patchify {H}x{W}")
    assert (body[:, 1176:] == 0).all()                                                     # pad columns: +0.0 exactly
    assert len(np.unique(img)) == 256


@gpu
def test_patchify_rejections_leave_the_output_untouched(device):
    from vision_inspection_system_amd import hip
    lib = hip.load()
    mean = (ctypes.c_float * 3)(*F.CLIP_MEAN)
    std = (ctypes.c_float * 3)(*F.CLIP_STD)
    std0 = (ctypes.c_float * 3)(F.CLIP_STD[0], 0.0, F.CLIP_STD[2])
    st = torch.cuda.current_stream().cuda_stream
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def call(H, W, ld, out_ptr, sd=std):
        img = torch.zeros((H, W, 3), dtype=torch.uint8, device=device)
        return lib.vis_patchify_u8(img.data_ptr(), out_ptr, H, W, ld, 0, p(mean), p(sd), st)

    out = _sentinel((16, 1280), device)
    assert call(28, 28, 1216, out.data_ptr()) == 0                     # the control: this call is fine
    out = _sentinel((16, 1280), device)
    assert call(42, 28, 1216, out.data_ptr()) != 0                     # H not a multiple of 28
    assert call(28, 42, 1216, out.data_ptr()) != 0
    assert call(28, 28, 1168, out.data_ptr()) != 0                     # ld_out below the 1176 features
    assert call(28, 28, 1180, out.data_ptr()) != 0                     # ld_out not a multiple of 8
    assert call(28, 28, 1216, out.data_ptr(), std0) != 0               # std = 0
    assert call(28, 28, 1216, out.data_ptr() + 2) != 0                 # misaligned out
    torch.cuda.synchronize()
    assert (_bits(out) == F.SENTINEL).all()


# ------------------------------------------------------------------------------------------- vis_patchify_tiles_u8
TILE_CASES = [(tile, th, tw, short) for tile in (28, 560) for (th, tw) in ((1, 1), (1, 4), (4, 1), (2, 2))
              for short in (0, 1)]


@gpu
@pytest.mark.parametrize("tile,th,tw,short", TILE_CASES)
def test_patchify_tiles_is_bit_exact(device, tile, th, tw, short):
    _run_tiles(device, tile, th, tw, th * tile - short, tw * tile - short, 592 if short else 640)


@gpu
def test_patchify_tiles_beyond_the_grid_cap(device):
    """2 x 2 tiles of 560 at ld_out = 1344: 4 x 1600 x 168 items > 4096 blocks x 256 - the stride loop iterates."""
    assert 4 * 1600 * (1344 // 8) > 4096 * 256
    _run_tiles(device, 560, 2, 2, 1100, 1119, 1344)


def _run_tiles(device, tile, th, tw, H, W, ld):
    from vision_inspection_system_amd import hip
    rng = np.random.default_rng(tile * 1000 + th * 100 + tw * 10 + (H % 7))
    img = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)             # no level 0 inside: padding is told apart
    G = tile // 14
    per = G * G + 1
    absent = 2                                                       # rows of tiles that are not there: untouched
    out = _sentinel(((th * tw + absent) * per, ld), device)
    hip.patchify_tiles(torch.from_numpy(img).to(device), out, th, tw, tile, F.CLIP_MEAN, F.CLIP_STD)
    got = _bits(out).reshape(th * tw + absent, per, ld)
    assert (got[th * tw:] == F.SENTINEL).all()
    assert (got[:, 0] == F.SENTINEL).all()                           # the CLS row of every tile
    canvas = np.zeros((th * tile, tw * tile, 3), dtype=np.int64)
    canvas[:H, :W] = img
    levels = F.tiles_layout(canvas, th, tw, tile)
    chans = F.tiles_layout(F.channel_image(th * tile, tw * tile), th, tw, tile)
    body = got[:th * tw, 1:]
    F.check_levels(body[..., :588], levels, chans, TABLE, f"tiles {tile} {th}x{tw} {H}x{W}")
    pad = levels == 0
    assert pad.sum() == (th * tile * tw * tile - H * W) * 3
    assert (body[..., :588][pad] == TABLE[0][chans[pad], 0]).all()    # padded pixels: bf16((0 - mean) / std), exactly
    assert (body[..., 588:] == 0).all()


# ------------------------------------------------------------------------------------------------------ row movers
N_LIST = (1, 3, 4, 5, 257)
D_LIST = (8, 520, 3584, 8192)                                         # 520: 65 chunks = one wrap of the 64 lanes + a tail
I32_MAX = 2 ** 31 - 1


def _row_pattern(rows, D, salt):
    """int16 patterns that name their row (element 0) and differ from row to row and column to column everywhere."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    j = np.arange(D, dtype=np.int64)[None, :]
    a = ((r * 131 + j * 7 + salt) % 0x7F00).astype(np.uint16)         # below the NaN / inf patterns
    a[:, 0] = r[:, 0] + salt
    return a


def _ids(n, n_table, rng):
    special = [-1, 0, n_table - 1, n_table, I32_MAX, 5, 5, -I32_MAX - 1]
    k = n % len(special)
    ids = (special[k:] + special[:k])[:n]
    ids += [int(v) for v in rng.integers(0, n_table, n - len(ids))]
    return np.array(ids, dtype=np.int64)


def _dev_i16(a, device):
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)


@gpu
@pytest.mark.parametrize("D", D_LIST)
def test_gather_rows_clamps_and_copies_whole_rows(device, D):
    from vision_inspection_system_amd import hip
    n_table = 37
    table = _row_pattern(n_table, D, 1000)
    seen = set()
    for n in N_LIST:
        ids = _ids(n, n_table, np.random.default_rng(n))
        seen.update(int(i) for i in ids)
        out = _sentinel((n + 3, D), device)
        hip.gather_rows(_dev_i16(table, device), torch.from_numpy(ids.astype(np.int32)).to(device), out[:n])
        got = _bits(out)
        assert np.array_equal(got[:n], table[np.clip(ids, 0, n_table - 1)]), (D, n)
        assert (got[n:] == F.SENTINEL).all()
    assert {-1, 0, n_table - 1, n_table, I32_MAX} <= seen


@gpu
@pytest.mark.parametrize("D", D_LIST)
def test_scatter_rows_skips_out_of_range_targets(device, D):
    from vision_inspection_system_amd import hip
    for n in N_LIST:
        rng = np.random.default_rng(100 + n)
        n_dst = n + 6
        src = _row_pattern(n, D, 2000)
        bad = [-1, n_dst, I32_MAX, -I32_MAX - 1, n_dst, -1]
        idx = np.array([bad[(i // 3) % len(bad)] for i in range(n)], dtype=np.int64)
        kept = [i for i in range(n) if n == 1 or i % 3]              # every third row is skipped (not the only row)
        pool = [0, n_dst - 1] + [int(v) for v in 1 + rng.permutation(n_dst - 2)]
        idx[kept] = pool[:len(kept)]                                 # distinct targets: the result is defined
        dst = _sentinel((n_dst, D), device)
        hip.scatter_rows(_dev_i16(src, device), torch.from_numpy(idx.astype(np.int32)).to(device), dst)
        want = np.full((n_dst, D), F.SENTINEL, dtype=np.uint16)
        for i, t in enumerate(idx):
            if 0 <= t < n_dst:
                want[t] = src[i]
        assert np.array_equal(_bits(dst), want), (D, n)


@gpu
@pytest.mark.parametrize("D", D_LIST)
def test_add_rows_is_one_f32_add_rounded_once(device, D):
    from vision_inspection_system_amd import hip
    n_table = 9
    for n in N_LIST:
        g = torch.Generator().manual_seed(7 * D + n)
        mk = lambda rows: (torch.randn((rows, D), generator=g) *
                           torch.exp2(torch.randint(-12, 13, (rows, D), generator=g).float())).to(torch.bfloat16)
        x, t = mk(n), mk(n_table)
        x[:, 0] = torch.arange(n, dtype=torch.float32).to(torch.bfloat16)                 # rows name themselves
        t[:, 0] = (1024 + 8 * torch.arange(n_table, dtype=torch.float32)).to(torch.bfloat16)
        ids = _ids(n, n_table, np.random.default_rng(n + D))
        cl = torch.from_numpy(np.clip(ids, 0, n_table - 1))
        want = (x.float() + t[cl].float()).to(torch.bfloat16)
        if n >= 5:
            ex = torch.frexp(x.float())[1] - torch.frexp(t[cl].float())[1]
            assert (ex.abs() > 8).any() and (ex.abs() <= 8).any()     # pairs where the smaller term is below half an ulp
        buf = _sentinel((n + 2, D + 8), device)                        # ldx = D + 8; two rows nobody owns
        buf[:n, :D] = x.to(device)
        hip.add_rows(buf[:n, :D], t.to(device), torch.from_numpy(ids.astype(np.int32)).to(device))
        got = _bits(buf)
        assert np.array_equal(got[:n, :D], want.view(torch.int16).numpy().view(np.uint16)), (D, n)
        assert (got[:n, D:] == F.SENTINEL).all() and (got[n:] == F.SENTINEL).all()
