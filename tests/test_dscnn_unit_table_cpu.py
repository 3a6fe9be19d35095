"""CPU test of the DS-CNN unit descriptor table (kws_host_dscnn_units, csrc/kws_dscnn_units.h): the words every DS-CNN load
places behind the device image and the persistent batched forward reads in place of block_phase's per-unit geometry.  Checked
against a NumPy restatement of that geometry, written from the kernel's description (csrc/kws_dscnn_geom.h and block_phase in
csrc/kws_dscnn_stages.h) and not from the packer: output position of a lane, clamp into the map, row and column, the three
own-column tap slots (interior, ring slot P, outside slot P + 1), the neighbour masks, the store mask.  Every block, every tile
(the K-split leftover tiles of blocks 1 and 2 included), all 64 lanes."""
import numpy as np
import pytest

from kws import _native as native

TW = 30                                            # output positions per tile: 32 MFMA columns minus two halo columns
OFF_IN = {1: 9152, 2: 0, 3: 22976, 4: 0}           # LDS float offset of the plane block n reads (Z0, Z1, Z2, Z3)
LDS_FLOATS = 40960


def geometry(n):
    """Block n (1..4): output map H x W; its stored input plane HI x WI (block 1 reads conv1's output, which has no ring; the
    others read the previous block's interior, one ring narrower than their own map)."""
    H, W = 45 + 2 * n, 1 + 2 * n
    ring = n > 1
    HI, WI = (H - 2, W - 2) if ring else (H, W)
    return H, W, ring, HI, WI


def pidx(c, p, S):
    """Channel pairs interleaved per position in planes of S floats."""
    return (c >> 1) * 2 * S + 2 * p + (c & 1)


def expected_block(n):
    H, W, ring, HI, WI = geometry(n)
    POUT, PIN = H * W, HI * WI
    SIN = PIN + 2
    tiles = -(-POUT // TW)
    want = np.zeros((tiles, 2, 64, 4), np.uint32)
    for t in range(tiles):
        for lane in range(64):
            half, col = lane >> 5, lane & 31
            pos = t * TW - 1 + col                 # column 0 and column 31 are halo
            valid = 1 <= col <= TW and pos < POUT
            posc = min(max(pos, 0), POUT - 1)
            h, x = divmod(posc, W)
            for dh in (-1, 0, 1):
                o = 1 if ring else 0
                hh, xx = h + dh - o, x - o
                if 0 <= hh < HI and 0 <= xx < WI:
                    a = hh * WI + xx                # a stored interior value
                elif ring and 0 <= h + dh < H:
                    a = PIN                         # on the relu(bias) ring
                else:
                    a = PIN + 1                     # outside the padded map: zero
                want[t, 0, lane, dh + 1] = OFF_IN[n] + pidx(8 * half, a, SIN)
            want[t, 0, lane, 3] = 0xFFFFFFFF if valid else 0
            want[t, 1, lane, 0] = np.float32(1.0 if x > 0 else 0.0).view(np.uint32)
            want[t, 1, lane, 1] = np.float32(1.0 if x < W - 1 else 0.0).view(np.uint32)
    return want


@pytest.fixture(scope="module")
def table():
    return native.host_dscnn_units()


def test_size_alignment_and_bases(table):
    words, base = table
    tiles = [-(-((45 + 2 * n) * (1 + 2 * n)) // TW) for n in range(1, 5)]
    assert tiles == [5, 9, 12, 16]
    assert base.tolist() == [0, 5, 14, 26, 42]
    assert words.shape == (42, 2, 64, 4) and words.dtype == np.uint32
    assert words.nbytes == 42 * 64 * 32 and words.nbytes % 16 == 0
    # behind the image, whose size is a whole number of 16-byte rows for every class count and channel count
    for C, Cin in [(12, 1), (35, 1), (1, 1), (64, 1), (12, 3), (7, 64)]:
        from oracle import dscnn as o_dscnn

        blob = o_dscnn.flatten_state(o_dscnn.random_state(1, num_classes=C, input_channels=Cin))
        image, _ = native.host_dscnn_image(blob, C, Cin)
        assert image.size % 4 == 0, (C, Cin, image.size)


def test_size_protocol():
    import ctypes as C

    need = C.c_size_t(0)
    assert native.lib().kws_host_dscnn_units(None, 0, C.byref(need), None) == native.KWS_OK
    assert need.value == 42 * 2 * 64 * 4
    small = np.zeros(16, np.uint32)
    rc = native.lib().kws_host_dscnn_units(small.ctypes.data_as(C.POINTER(C.c_uint32)), small.size, None, None)
    assert rc != native.KWS_OK and not small.any()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_every_tile_and_lane_of_block(table, n):
    words, base = table
    got = words[base[n - 1]:base[n]]
    want = expected_block(n)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"block {n}: {len(bad)} words differ, first (tile, part, lane, word) {bad[:5].tolist()}"


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_properties_of_block(table, n):
    """What the kernel relies on, stated without the restatement: every position is stored by exactly one lane pair, every tap
    read stays inside its plane (and so inside LDS, with the upper 32 channels' base too), pad words are zero."""
    words, base = table
    got = words[base[n - 1]:base[n]]
    H, W, ring, HI, WI = geometry(n)
    POUT, SIN = H * W, HI * WI + 2
    stores = np.zeros(POUT, np.int64)
    for t in range(got.shape[0]):
        for lane in range(64):
            if got[t, 0, lane, 3]:
                assert got[t, 0, lane, 3] == 0xFFFFFFFF
                stores[t * TW - 1 + (lane & 31)] += 1
    assert (stores == 2).all()  # both half-waves (they hold different output channels)
    taps = got[:, 0, :, :3].astype(np.int64)
    half = (np.arange(64) >> 5)[None, :, None]
    rel = taps - OFF_IN[n] - 8 * half * SIN  # = 2 * slot
    assert (rel % 2 == 0).all() and (rel >= 0).all() and (rel // 2 <= HI * WI + 1).all()
    # the farthest read: channel pair 8 * half + 62 of the plane, 8 bytes wide
    assert (taps + 62 * SIN + 1 < LDS_FLOATS).all()
    assert not got[:, 1, :, 2:].any()
    assert np.isin(got[:, 1, :, :2], [0, np.float32(1.0).view(np.uint32)]).all()


def test_leftover_tiles_are_the_last_tiles(table):
    """The K-split leftover units (a quarter per wavefront) read the fifth tile of block 1 and the ninth of block 2."""
    words, base = table
    for n, tile, n_pos in [(1, 4, 21), (2, 8, 5)]:
        d = words[base[n - 1] + tile]
        assert base[n - 1] + tile == base[n] - 1
        assert int(np.count_nonzero(d[0, :32, 3])) == n_pos
