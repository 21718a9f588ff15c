"""tests/strip_format.py - the NumPy restatement of the strip formats of include/hz_hip.h that tests/test_gpu_strips.py
holds the kernels to - against what it restates, on the CPU: its conversion against the naive loop of
tests/naive_host_math.py, its encoder and decoder against the oracle's images, and the sizes horizonator_amd/sharding.py
computes against its layout."""
import numpy as np
import pytest

import hzutil
import naive_host_math as nv
import oracle
import strip_format as sf
from horizonator_amd import sharding

ZOO = {c["name"]: c for c in hzutil.zoo_cases()}


def naive_tanel(W, H, az0, az1):
    """tan(elevation) per GL row as ranges_from_depth() uses it: the lower half computed, the upper half mirrored"""
    t = np.empty(H, np.float32)
    for y in range(H - H // 2):
        t[y] = nv.get_tanel(y, W, H, az0, az1)
    for y in range(H // 2):
        t[H - 1 - y] = -nv.get_tanel(y, W, H, az0, az1)
    return t


@pytest.mark.parametrize("znear,zfar", [(100.0, 40000.0), (10.0, 5e8)])
@pytest.mark.parametrize("H", [6, 7])
def test_convert_equals_the_naive_loop(H, znear, zfar):
    W, az0, az1 = 9, -33.5, 140.25
    k = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    z24 = ((k * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 24)).astype(np.uint32)
    z24[0, 0], z24[0, 1], z24[0, 2], z24[0, 3] = 0, 1, 0xFFFFFE, 0xFFFFFF
    z24[H - 1, W - 1], z24[H - 1, 0], z24[H // 2, 4], z24[H // 2, 5] = 0, 0xFFFFFE, 1, 0xFFFFFF
    z24[1, :] = 0xFFFFFF
    z24[2, ::2] = 0x800000
    red = ((k * np.uint64(97)) % np.uint64(256)).astype(np.uint8)
    red[0, 0], red[0, 1] = 0, 255
    bgr, ranges = sf.convert(z24, red, naive_tanel(W, H, az0, az1), znear, zfar)
    want = nv.ranges_from_depth(z24[::-1], W, H, az0, az1, znear, zfar)
    assert ranges.dtype == np.float32 and np.array_equal(ranges.view(np.uint32), want.view(np.uint32))
    sky = z24 == 0xFFFFFF
    assert np.array_equal(ranges == -1.0, sky) and sky.sum() >= W + 2 and (ranges[~sky] > 0).all()
    assert np.array_equal(bgr[..., 0], np.where(sky, 255, 0)) and not bgr[..., 1].any()
    assert np.array_equal(bgr[..., 2], np.where(sky, 0, red))


# all of the image is terrain, part of it, none of it (the reference's terrain fractions: tests/golden/zoo_checksums.json)
@pytest.mark.parametrize("permuted", [False, True], ids=["rows_in_order", "rows_permuted"])
@pytest.mark.parametrize("name,fraction", [("checker-zoom12", (1.0, 1.0)), ("cliff-near360", (0.05, 0.95)), ("flat0-z005", (0.0, 0.0))])
def test_oracle_images_survive_the_sparse_strip(name, fraction, permuted):
    c = ZOO[name]
    W, H = c["W"], c["H"]
    v = oracle.make_view(**c["view"])
    want = oracle.render(hzutil.zoo_mosaic(c["family"], c["N"]), v, W, H)
    f = float((want["z24"] != 0xFFFFFF).mean())
    assert fraction[0] <= f <= fraction[1]
    red = want["bgr"][..., 2]
    ms = sf.mask_words(W) + (3 if permuted else 0)
    order = (np.arange(H) * 7 + 11) % H if permuted else None               # 7 is prime to every height used
    stream = sf.pack_sparse(want["z24"], red, ms, order)
    assert stream.dtype == np.uint32 and stream.size == sf.header_words(H, ms) + int(stream[0])
    terrain, z24, r8 = sf.unpack_sparse(stream, H, W, ms)
    assert np.array_equal(terrain, want["index"] >= 0) and np.array_equal(z24, want["z24"]) and np.array_equal(r8, red)
    bgr, ranges = sf.convert(z24, r8, oracle.tanel(W, H, v.az_deg0, v.az_deg1), v.znear, v.zfar)
    assert np.array_equal(bgr, want["bgr"])
    assert np.array_equal(ranges.view(np.uint32), want["ranges"].view(np.uint32))
    if permuted and f > 0:
        assert not np.array_equal(stream, sf.pack_sparse(want["z24"], red, ms))
    # ... and the dense words hold the same
    words = sf.pack_dense(want["z24"], red)
    assert np.array_equal(words >> 8, want["z24"]) and np.array_equal((words & 0xFF).astype(np.uint8), red)


@pytest.mark.parametrize("width", [1, 31, 32, 33, 65536])
def test_sharding_sizes_agree_with_the_layout(width):
    H = 3
    ms = sharding.sparse_mask_stride(width)
    assert ms == sf.mask_words(width) == len(range(0, width, 32))
    hdr = sharding.sparse_header_words(H, ms)
    assert hdr == sf.header_words(H, ms)
    # one terrain pixel, in the last column of the middle row: its mask bit is the last bit the stride has room for, and
    # its word is the first behind the header
    z24 = np.full((H, width), 0xFFFFFF, np.uint32)
    red = np.zeros((H, width), np.uint8)
    z24[1, width - 1], red[1, width - 1] = 0x123456, 0x78
    stream = sf.pack_sparse(z24, red, ms)
    assert stream.size == hdr + 1 and stream[0] == 1 and stream[hdr] == 0x12345678
    assert list(stream[1:1 + H]) == [0, 0, 1]
    mask = stream[1 + H:hdr]
    at = 1 * ms + (width - 1) // 32
    assert mask[at] == 1 << ((width - 1) % 32) and mask.astype(bool).sum() == 1 and at == 2 * ms - 1
