"""The strips of the multi-GPU gather as include/hz_hip.h describes them, restated in NumPy.

TEST CODE, written from the header's comments (hz_hip_pack, hz_hip_pack_sparse and the conversions that read what they
write, with what INTEGRATION.md adds about mask padding and sky words) and not from the kernels: an encoder and a decoder that share nothing with hz_k_resolve.h, so that a packer and an
unpacker that agree with each other and not with the published format show (tests/test_strip_format.py holds this module to
the oracle and to tests/naive_host_math.py on the CPU; tests/test_gpu_strips.py holds the kernels to it).

Images are top row first everywhere.  z24 is the raw 24-bit depth, 0xFFFFFF where no terrain; red the shade byte.

  packed strip   uint32 [H][stride]: z24<<8 | red8 per pixel.  A sky word has 0xFFFFFF in its upper 24 bits; the header
                 promises nothing about its low byte.
  sparse strip   a stream of uint32:
                   [0]                 T, the number of terrain pixels
                   [1 .. 1+H)          row_base[row]
                   [1+H .. HDR)        terrain mask, mask_stride words per row: bit c%32 of word c/32; bits of columns beyond
                                       the strip's last are 0, words from ceil(ncols/32) on are padding nobody reads
                   [HDR .. HDR+T)      z24<<8 | red8 of the terrain pixels: row `row` from HDR + row_base[row] on, left to
                                       right; the rows in any order
                 with HDR = 1 + H + H*mask_stride.
"""
import numpy as np

Z24_SKY = 0xFFFFFF


def mask_words(ncols):
    """mask words of a row that carry columns: ceil(ncols / 32), the smallest mask_stride"""
    return (int(ncols) + 31) // 32


def header_words(H, mask_stride):
    """HDR: the words before the terrain words"""
    return 1 + int(H) + int(H) * int(mask_stride)


def pack_dense(z24, red):
    """uint32[H, SW]: z24<<8 | red8"""
    z24 = np.asarray(z24, np.uint32)
    assert z24.ndim == 2 and z24.shape == np.shape(red) and int(z24.max(initial=0)) <= Z24_SKY
    return (z24 << np.uint32(8)) | np.asarray(red, np.uint8).astype(np.uint32)


def pack_sparse(z24, red, mask_stride, row_order=None):
    """the whole stream, HDR + T words.  row_order: the rows in the order in which their words lie in the data (any
    permutation of range(H); default top to bottom)"""
    words = pack_dense(z24, red)
    H, SW = words.shape
    assert mask_stride >= mask_words(SW)
    terrain = np.asarray(z24, np.uint32) != Z24_SKY
    count = terrain.sum(axis=1).astype(np.int64)
    T = int(count.sum())
    order = np.arange(H) if row_order is None else np.asarray(row_order, np.int64)
    assert sorted(order.tolist()) == list(range(H))
    HDR = header_words(H, mask_stride)
    out = np.zeros(HDR + T, np.uint32)
    out[0] = T
    mask = out[1 + H:HDR].reshape(H, mask_stride)
    rows, cols = np.nonzero(terrain)
    np.bitwise_or.at(mask, (rows, cols // 32), np.uint32(1) << (cols % 32).astype(np.uint32))
    at = 0
    for row in order.tolist():
        out[1 + row] = at
        out[HDR + at:HDR + at + count[row]] = words[row][terrain[row]]
        at += int(count[row])
    assert at == T
    return out


def unpack_sparse(stream, H, ncols, mask_stride):
    """(terrain bool[H, ncols], z24 uint32[H, ncols] with 0xFFFFFF on the sky, red uint8[H, ncols] with 0 there)"""
    stream = np.asarray(stream, np.uint32)
    HDR = header_words(H, mask_stride)
    T = int(stream[0])
    assert mask_stride >= mask_words(ncols) and stream.size >= HDR + T
    row_base = stream[1:1 + H].astype(np.int64)
    mask = stream[1 + H:HDR].reshape(H, mask_stride)
    c = np.arange(ncols)
    terrain = ((mask[:, c // 32] >> (c % 32).astype(np.uint32)) & np.uint32(1)).astype(bool) if ncols else np.zeros((H, 0), bool)
    z24 = np.full((H, ncols), Z24_SKY, np.uint32)
    red = np.zeros((H, ncols), np.uint8)
    for row in range(H):
        n = int(terrain[row].sum())
        assert row_base[row] + n <= T, "a row's words lie beyond T"
        w = stream[HDR + row_base[row]:HDR + row_base[row] + n]
        z24[row, terrain[row]] = w >> np.uint32(8)
        red[row, terrain[row]] = (w & np.uint32(0xFF)).astype(np.uint8)
    assert int(terrain.sum()) == T
    return terrain, z24, red


def convert(z24, red, tanel, znear, zfar):
    """the readback conversion (reference horizonator-lib.c:185, fragment.glsl:15-16, horizonator-lib.c:1013-1025):
    (bgr uint8[H, W, 3], ranges float32[H, W]).  Sky: B = 255, range -1.  Terrain: R = red, range = hypotf(len, tanel*len)
    with len = depth*(zfar-znear) + znear in float32 and depth = float32(z24 / 16777215.0), the arithmetic of
    tests/naive_host_math.py::ranges_from_depth vectorised.  tanel: tan(elevation) per GL row, row 0 = BOTTOM row."""
    f32, f64 = np.float32, np.float64
    z24 = np.asarray(z24, np.uint32)
    H, W = z24.shape
    tanel = np.asarray(tanel, f32)
    assert tanel.shape == (H,)
    sky = z24 == Z24_SKY
    bgr = np.zeros((H, W, 3), np.uint8)
    bgr[..., 0] = np.where(sky, 255, 0)
    bgr[..., 2] = np.where(sky, 0, np.asarray(red, np.uint8))
    with np.errstate(invalid="ignore", over="ignore"):
        depth = (z24.astype(f64) / f64(16777215.0)).astype(f32)
        length = depth * (f32(zfar) - f32(znear)) + f32(znear)          # float32 after every operation
        zt = tanel[::-1, None] * length
        assert length.dtype == f32 and zt.dtype == f32
        # hypotf of two floats: the sum of their squares is exact in double but for its last rounding
        r = np.sqrt(length.astype(f64) * length.astype(f64) + zt.astype(f64) * zt.astype(f64)).astype(f32)
    return bgr, np.where(sky, f32(-1.0), r).astype(f32)
