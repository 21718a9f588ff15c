"""The HIP path on image shapes next to the size rules of its kernels.  The other GPU tests draw many kinds of ground and
view into a narrow band of shapes (333x111 .. 1024x256, W 17..899 by H 9..399, a few round sizes up to 32768x8192);
hz_hip_create() takes any W, H >= 1 with W*H < 2^29, and which kernel or branch runs depends on the shape in many places:

  hz_plan.cpp        the short cull of whole cells (packed 16-bit pixel boxes, hz_k_march.h) is off for W < 64, W > 65535, H > 65535
  hz_convert.cpp     k_resolve4 for sector widths divisible by 4 into 16-byte aligned buffers, k_resolve otherwise; bands of rows
                     clamped to H; hz_hip_pack_sparse takes sectors of up to 65536 columns
  HZ_SEG = 256       the unit of the `touched` bytes, of one wave of k_resolve4 and of k_hiz: images narrower than a segment,
                     255 / 256 / 257 columns, sectors that end inside one
  tiles              k_hiz 8 x 4 and 32 x 16 in units of 16 rows, k_tile_* 64 x 64, the textured resolve's chunks of 256
                     pixels: images smaller than one of them
  hz_hostpath.cpp    blobs of 4 rows x 2048 columns with a 16-bit row field, the dense path from 65536 rows on, four bands
                     of rows (H < 4), up to eight azimuth sectors (W < 8)

hzutil.shape_cases() puts zoo grounds under their zoo views at 1x1 .. 16384x4, 65535x8 .. 70001x7 and 8x65536 .. 8x140001,
and, because the short cull only runs on rows of vertices that are all inside the view volume, which those wide and tall
shapes have none of, at 65535x64 .. 65537x63 from two metres above level ground and at 64x65535 .. 63x66000 over 360 degrees
(with the tests of W and H taken out of hz_plan.cpp:127 the draws of 65536x64, 65537x63 and 64x65536 differ from the oracle
on 47 to 434136 pixels, those of 65535x64, 64x65535 and 63x66000 on none: tried once while this file was written).
Likewise the host path's test of H: the terrain of 8x65536 and 7x70001 lies around row H/2, which a blob's 16-bit row field
still holds; that of 8x140001 around row 70000 (with `H <= 65535` taken out of hz_hostpath.cpp the delivery of 8x140001
differs on 1948 pixels, the others on none).
Every comparison is bit for bit on all four outputs against the CPU oracle; up to 16384 pixels a side the image and the
depth also hash to what the reference's shaders drew on llvmpipe (tests/golden/shape_checksums.json, to which
tests/test_oracle_golden.py holds the oracle too: that entitles these tests to the oracle's index and ranges).  llvmpipe
draws no more than 16384 pixels a side: the wide and tall shapes are held to the oracle alone.

No framebuffer here is above 4 Mpix."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import hzutil
import oracle
import strip_format as sf
from test_gpu_strips import check_dense, check_sparse

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = hzutil.shape_cases()
BY_ID = {c["id"]: c for c in SHAPES}
with open(os.path.join(GOLD, "shape_checksums.json")) as _f:
    SHAPE_GOLD = json.load(_f)
SKY = sf.Z24_SKY
SENT = 0x5EA15EA1               # what a device buffer holds before a call (tests/test_gpu_strips.py checks for it behind a strip)
GUARD = 4099                    # words behind the last one a call may write
OUTPUTS = ("bgr", "ranges", "index", "z24")
same = hzutil.same_render


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(c):
    return hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"])


@functools.lru_cache(maxsize=6)
def _oracle_full(case_id):
    """the oracle's whole image of a case: computed once, shared by the tests next to each other that draw it, never
    written to.  (A sector is compared with its columns: tests/test_oracle_golden.py holds the oracle's sector draws to them)"""
    c = BY_ID[case_id]
    m, v = _inputs(c)
    out = oracle.render(m, v, c["W"], c["H"])
    for a in out.values():
        a.setflags(write=False)
    return out


def _columns(full, c0, c1):
    return {k: a[:, c0:c1] for k, a in full.items()}


def _shown(W, H, ground=None):
    """the case of a shape that shows terrain on the oracle (the fixture's count): on `ground` (a zoo family) if given"""
    mine = [c for c in SHAPES if (c["W"], c["H"]) == (W, H) and SHAPE_GOLD[c["id"]]["terrain_pixels"] > 0
            and (ground is None or c["family"] == ground)]
    assert mine, (W, H, ground)
    return mine[0]


def _hzview(v):
    out = hzutil.hzlib.View()
    for name, _ in hzutil.hzlib.View._fields_:
        setattr(out, name, getattr(v, name))
    return out


# ---- every case, both rasterisers -----------------------------------------------------------------

@pytest.mark.parametrize("raster", [1, 2])                  # (the rasterisers of one case next to each other: one oracle draw)
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c["id"])
def test_shape_case_equals_the_oracle_and_the_reference_draw(case, raster):
    """a fresh context: the whole image, then the case's sector (one column at column 0 or W-1, widths and starts that are
    no multiple of 4, six columns across column 65536, the last three)"""
    m, v = _inputs(case)
    W, H = case["W"], case["H"]
    want = _oracle_full(case["id"])
    g = SHAPE_GOLD[case["id"]]
    assert _sha(m) == g["mosaic_sha256"] and int((want["index"] >= 0).sum()) == g["terrain_pixels"]
    with hzutil.HipDev(m, W, H, raster=raster) as dev:
        hip = dev.render(v)
        same(hip, want, f"{case['id']} raster {raster}")
        if "bgr_sha256" in g:
            assert _sha(hip["bgr"]) == g["bgr_sha256"], "image differs from the reference's shaders' on llvmpipe"
            assert _sha(hip["z24"]) == g["z24_sha256"], "depth differs from the reference's shaders' on llvmpipe"
        terrain = hip["index"] >= 0
        assert np.array_equal((hip["ranges"] > 0) | np.isnan(hip["ranges"]), terrain) and hip["index"].max() < 2 * (case["N"] - 1) ** 2
        c0, c1 = case["c0"], case["c1"]
        same(dev.render(v, c0, c1), _columns(want, c0, c1), f"{case['id']} raster {raster} [{c0},{c1})")


# ---- delivery paths on the same draws ---------------------------------------------------------------

DELIVERY_SHAPES = [(1, 1), (7, 1), (3, 5), (15, 4), (16, 9), (255, 3), (256, 4), (257, 5), (65, 65), (2049, 5),
                   (65536, 8), (70001, 7), (8, 65536), (7, 70001), (8, 140001)]


def _unaligned_sector(W):
    """a sector whose first column and whose width are no multiples of four (the whole image where it is too narrow for that)"""
    if W < 7:
        return 0, W
    c0 = (W // 3) | 1
    c1 = W - 2 if (W - 2 - c0) % 4 else W - 3
    return c0, c1


class _Dev:
    """a context holding a case's ground, with device buffers for the calls that deliver into device memory"""

    def __init__(self, case):
        import torch
        self.torch = torch
        self.case = case
        self.m, self.v = _inputs(case)
        self.W, self.H = case["W"], case["H"]
        self.dev = hzutil.HipDev(self.m, self.W, self.H)
        self.lib, self.h = self.dev.lib, self.dev.dev
        self.hv = _hzview(self.v)
        self.tanel = np.ascontiguousarray(oracle.tanel(self.W, self.H, self.hv.az_deg0, self.hv.az_deg1), np.float32)

    def close(self):
        self.dev.close()

    def err(self):
        return (self.lib.hz_hip_last_error() or b"").decode()

    def draw(self, c0, c1):
        assert self.lib.hz_hip_set_sector(self.h, c0, c1) == 0, self.err()
        assert self.lib.hz_hip_draw(self.h, C.byref(self.hv)) == 0, self.err()

    def words(self, n, fill=SENT):
        t = self.torch.full((n,), fill, dtype=self.torch.int32, device="cuda:0")
        self.torch.cuda.synchronize()
        return t

    def sync(self):
        assert self.lib.hz_hip_sync(self.h) == 0, self.err()


@pytest.fixture
def ctx():
    made = []

    def make(case):
        made.append(_Dev(case))
        return made[-1]
    yield make
    for d in made:
        d.close()


_NP = {"bgr": (np.uint8, 3), "ranges": (np.float32, 1), "index": (np.int32, 1), "z24": (np.uint32, 1)}


@pytest.mark.parametrize("shape", DELIVERY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_resolve_into_device_buffers_each_output_alone_and_all_together(shape, ctx):
    """hz_hip_resolve (k_resolve4 where the sector width is a multiple of 4 and the buffers are 16-byte aligned, k_resolve
    otherwise; both clear the framebuffer behind themselves, so every call but the first reads a draw made again): the whole
    image and a sector whose start and width are no multiples of 4, each of the four outputs asked for alone and all
    together; where k_resolve4 would run, once more into buffers that start four bytes off a multiple of 16"""
    case = _shown(*shape)
    d = ctx(case)
    torch = d.torch
    want_full = _oracle_full(case["id"])
    for c0, c1 in dict.fromkeys([(0, d.W), _unaligned_sector(d.W)]):
        SW = c1 - c0
        want = _columns(want_full, c0, c1)
        asks = [(k,) for k in OUTPUTS] + [OUTPUTS] + ([OUTPUTS + ("off",)] if SW % 4 == 0 else [])
        for ask in asks:
            off = 1 if "off" in ask else 0
            bufs = {}
            for k in OUTPUTS:
                if k in ask:
                    # 32-bit words throughout (the image's bytes too: H*SW*3 is a multiple of 4 where it matters for `off`)
                    nwords = (d.H * SW * _NP[k][1] * np.dtype(_NP[k][0]).itemsize + 3) // 4
                    bufs[k] = d.words(off + nwords + GUARD)
            d.draw(c0, c1)
            ptr = {k: (bufs[k].data_ptr() + 4 * off if k in bufs else None) for k in OUTPUTS}
            assert d.lib.hz_hip_resolve(d.h, C.byref(d.hv), d.tanel.ctypes.data, ptr["bgr"], ptr["ranges"], ptr["index"], ptr["z24"]) == 0, d.err()
            d.sync()
            got = {}
            for k, t in bufs.items():
                raw = t.cpu().numpy().view(np.uint32)
                n = d.H * SW * _NP[k][1] * np.dtype(_NP[k][0]).itemsize
                got[k] = raw[off:].view(np.uint8)[:n].view(_NP[k][0]).reshape((d.H, SW, 3) if k == "bgr" else (d.H, SW))
                tail = raw[off + (n + 3) // 4:]
                assert (raw[:off] == SENT).all() and (tail == SENT).all(), f"{case['id']} [{c0},{c1}) {ask}: {k} written outside its buffer"
            same(got, {k: want[k] for k in got}, f"{case['id']} [{c0},{c1}) hz_hip_resolve {ask}")


def _sparse_sector(W):
    """hz_hip_pack_sparse takes sectors of up to 65536 columns: the whole image, or its last 65536 columns"""
    return (0, W) if W <= 65536 else (W - 65536, W)


@pytest.mark.parametrize("shape", DELIVERY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_packed_and_sparse_strips_hold_the_format_and_convert_to_the_oracles_image(shape, ctx):
    """hz_hip_pack + hz_hip_resolve_packed and hz_hip_pack_sparse + hz_hip_resolve_sparse: the words written against
    tests/strip_format.py's encoding of the oracle's image (its decoder reads them back), the conversion of those words
    against the oracle's image and ranges"""
    case = _shown(*shape)
    d = ctx(case)
    lib, h = d.lib, d.h
    want_full = _oracle_full(case["id"])
    W, H = d.W, d.H
    for dense in (True, False):
        for c0, c1 in dict.fromkeys([(0, W) if dense else _sparse_sector(W), _unaligned_sector(W)]):
            n = c1 - c0
            want = _columns(want_full, c0, c1)
            what = f"{case['id']} [{c0},{c1}) {'dense' if dense else 'sparse'}"
            d.draw(c0, c1)
            ms = sf.mask_words(n) + (0 if n % 64 else 1)
            buf = d.words((H * n if dense else sf.header_words(H, ms) + H * n) + GUARD)
            if dense:
                assert lib.hz_hip_pack(h, buf.data_ptr()) == 0, d.err()
            else:
                assert lib.hz_hip_pack_sparse(h, buf.data_ptr(), ms) == 0, d.err()
            d.sync()
            got = buf.cpu().numpy().view(np.uint32)
            if dense:
                check_dense(got, want["z24"], want["bgr"][..., 2], what)
            else:
                check_sparse(got, want["z24"], want["bgr"][..., 2], ms, what)
                terrain, z24, red = sf.unpack_sparse(got[:sf.header_words(H, ms) + int(got[0])], H, n, ms)
                assert np.array_equal(z24, want["z24"]) and np.array_equal(red[terrain], want["bgr"][..., 2][terrain]), what
            # ... and back: into full-width outputs prefilled with something else
            img = d.torch.full((H, W, 3), 77, dtype=d.torch.uint8, device="cuda:0")
            rng = d.torch.full((H, W), -7.0, dtype=d.torch.float32, device="cuda:0")
            d.torch.cuda.synchronize()
            if dense:
                rc = lib.hz_hip_resolve_packed(h, C.byref(d.hv), d.tanel.ctypes.data, buf.data_ptr(), n, n, c0, img.data_ptr(), rng.data_ptr())
            else:
                rc = lib.hz_hip_resolve_sparse(h, C.byref(d.hv), d.tanel.ctypes.data, buf.data_ptr(), ms, n, c0, img.data_ptr(), rng.data_ptr())
            assert rc == 0, d.err()
            d.sync()
            img, rng = img.cpu().numpy(), rng.cpu().numpy()
            same({"bgr": img[:, c0:c1], "ranges": rng[:, c0:c1]}, {"bgr": want["bgr"], "ranges": want["ranges"]}, what + " converted")
            assert (np.delete(img, np.s_[c0:c1], axis=1) == 77).all() and (np.delete(rng, np.s_[c0:c1], axis=1) == -7.0).all(), what + ": columns beside the strip written"
            bgr2, rng2 = sf.convert(want["z24"], want["bgr"][..., 2], d.tanel, d.hv.znear, d.hv.zfar)
            assert np.array_equal(bgr2, want["bgr"]) and np.array_equal(np.isnan(rng2), np.isnan(want["ranges"])) \
                and np.array_equal(np.nan_to_num(rng2, nan=-7.0), np.nan_to_num(want["ranges"], nan=-7.0)), what + ": strip_format's conversion"


def test_sparse_packer_takes_65536_columns_and_refuses_65537(ctx):
    """... with its message, and leaves its output as it was"""
    case = _shown(70001, 7, "checker")
    d = ctx(case)
    W, H = d.W, d.H
    n = 65537
    ms = sf.mask_words(n)
    d.draw(W - n, W)
    buf = d.words(sf.header_words(H, ms) + H * n + GUARD)
    assert d.lib.hz_hip_pack_sparse(d.h, buf.data_ptr(), ms) == -1
    assert "sectors of up to 65536 columns" in d.err()
    d.sync()
    assert (buf.cpu().numpy().view(np.uint32) == SENT).all()
    # the same draw, one column fewer: taken (and compared with the oracle in the test above)
    assert d.lib.hz_hip_set_sector(d.h, W - 65536, W) == 0
    assert d.lib.hz_hip_draw(d.h, C.byref(d.hv)) == 0, d.err()
    assert d.lib.hz_hip_pack_sparse(d.h, buf.data_ptr(), sf.mask_words(65536)) == 0, d.err()
    d.sync()
    want = _columns(_oracle_full(case["id"]), W - 65536, W)
    assert int(buf[0].item()) == int((want["z24"] != SKY).sum())


@pytest.mark.parametrize("shape", [(70001, 7), (7, 70001), (8, 65536), (8, 140001)], ids=lambda s: "%dx%d" % s)
def test_read_depth_at_the_corners_and_at_the_last_terrain_pixel(shape, ctx):
    """hz_hip_read_depth on the widest and tallest images: the four corners, the first and the last terrain pixel (columns
    beyond 65535, rows beyond 32767 and, at 140001 rows, beyond 65535), and a refusal outside the image"""
    case = _shown(*shape, ground="checker")
    d = ctx(case)
    W, H = d.W, d.H
    want = _oracle_full(case["id"])["z24"]
    d.draw(0, W)
    ys, xs = np.nonzero(want != SKY)
    by_col = np.argmax(xs)
    points = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1])), (int(xs[by_col]), int(ys[by_col]))]
    assert max(p[0] for p in points[4:]) > 65535 or max(p[1] for p in points[4:]) > 32767
    for x, y in points:
        rc, z = d.dev.read_depth(x, y)
        assert rc == 0 and z == int(want[y, x]), (case["id"], x, y, z, int(want[y, x]))
    assert d.dev.read_depth(W, 0)[0] == -1 and d.dev.read_depth(0, H)[0] == -1


@pytest.mark.parametrize("shape", [(8, 65536), (7, 70001), (8, 140001)], ids=lambda s: "%dx%d" % s)
def test_host_begin_refuses_more_than_65535_rows_and_the_context_renders_on(shape, ctx):
    """a blob's row field has 16 bits: such images deliver with hz_hip_render_to_host() only (the dense path)"""
    case = _shown(*shape)
    d = ctx(case)
    W, H = d.W, d.H
    bgr, rng = np.full((H, W, 3), 7, np.uint8), np.full((H, W), 7.0, np.float32)
    assert d.lib.hz_hip_host_begin(d.h, C.byref(d.hv), d.tanel.ctypes.data, bgr.ctypes.data, rng.ctypes.data, None, None) == -1
    assert "images of more than 65535 rows" in d.err() and "hz_hip_render_to_host() only" in d.err()
    assert (bgr == 7).all() and (rng == 7.0).all()
    want = _oracle_full(case["id"])
    for k in range(2):                                      # render_to_host, then draw + resolve_to_host
        same(d.dev.render(d.v), want, f"{case['id']} after the refusal, call {k}")


# ---- forced modes on the shapes they were never run at ----------------------------------------------

MODES = [
    dict(HZ_TWO_PASS="1", HZ_HIZ="1", HZ_NEAR_CELLS="16"),
    dict(HZ_TILES="1", HZ_TWO_PASS="1"),
    dict(HZ_TILES="1", HZ_TWO_PASS="1", HZ_TILE_LIST="3"),
    dict(HZ_QUEUE_CAPACITY="1"),
    dict(HZ_NO_WORKLIST="1"),
    dict(HZ_RESOLVE_CLEARS="0"),
    dict(HZ_HOST_DENSE="1"),
]
MODE_SHAPES = [s for s in hzutil.SHAPES_TINY if s[0] <= 257 and s[1] <= 33] + [(65, 65), (33, 17)]


def _mode_id(m):
    return " ".join(f"{k}={v}" for k, v in m.items())


def _check_case_whole_and_sector(c, what, raster=0):
    """one fresh context: the whole image (hz_hip_render_to_host), then the case's sector (hz_hip_draw + hz_hip_resolve_to_host)"""
    m, v = _inputs(c)
    want = _oracle_full(c["id"])
    with hzutil.HipDev(m, c["W"], c["H"], raster=raster) as dev:
        same(dev.render(v), want, f"{c['id']} {what}")
        same(dev.render(v, c["c0"], c["c1"]), _columns(want, c["c0"], c["c1"]), f"{c['id']} [{c['c0']},{c['c1']}) {what}")


@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
@pytest.mark.parametrize("shape", MODE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_forced_modes_on_tiny_and_one_segment_images(shape, mode, monkeypatch):
    """two rounds with coarse depth and a first round of 16 cells, the tile bins (with lists of three), queues of one
    record, every strip launched, conversions that do not clear, the dense host path - on images smaller than a tile of
    each, every ground of the shape"""
    for k, x in mode.items():
        monkeypatch.setenv(k, x)
    for c in [c for c in SHAPES if (c["W"], c["H"]) == shape]:
        _check_case_whole_and_sector(c, _mode_id(mode), raster=2)


@pytest.mark.parametrize("mode", [MODES[0], MODES[1], MODES[3]], ids=_mode_id)
@pytest.mark.parametrize("shape", [(70001, 7), (7, 70001)], ids=lambda s: "%dx%d" % s)
def test_forced_modes_on_the_widest_and_the_tallest_image(shape, mode, monkeypatch):
    for k, x in mode.items():
        monkeypatch.setenv(k, x)
    _check_case_whole_and_sector(_shown(*shape, ground="checker"), _mode_id(mode), raster=2)


@pytest.mark.parametrize("mode", [MODES[0], MODES[1]], ids=_mode_id)
@pytest.mark.parametrize("case_id", ["65536x64-stairs-near360-vz202", "64x65536-coast-near360"])
def test_forced_modes_where_the_short_cull_has_rows_and_the_size_switches_it_off(case_id, mode, monkeypatch):
    """the early depth test (pairs of pixels, coarse depth) and the tile bins at columns beyond 65535 and rows beyond 32767
    of images in which whole rows of vertices lie inside the view volume"""
    for k, x in mode.items():
        monkeypatch.setenv(k, x)
    _check_case_whole_and_sector(BY_ID[case_id], _mode_id(mode), raster=2)


@pytest.mark.parametrize("sectors", [1, 3, 4, 8])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 1), (9, 300), (70001, 7), (5, 3), (33, 65535), (8, 65536), (8, 140001)], ids=lambda s: "%dx%d" % s)
def test_host_delivery_in_sectors_on_narrow_low_wide_and_tall_images(shape, sectors, monkeypatch):
    """HZ_HOST_SECTORS = 1, 3, 4, 8 on W = 1, 3, 7, 9, 70001 and H = 1, 3, 5, 65535, 65536: sectors narrower than a column
    are not made, 65535 rows are the last a blob's row field holds, 65536 rows take the dense path; at 140001 rows the
    terrain itself lies in rows that 16 bits do not hold"""
    monkeypatch.setenv("HZ_HOST_SECTORS", str(sectors))
    c = _shown(*shape)
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    want = _oracle_full(c["id"])
    with hzutil.HipDev(m, W, H) as dev:
        for k in range(3):                              # render_to_host, draw + resolve_to_host, render_to_host again
            same(dev.render(v), want, f"{c['id']} {sectors} sectors call {k}")
        for ask in (("bgr",), ("ranges", "z24"), ("index",)):
            got = dev.render(v, want=ask)
            same(got, {k: want[k] for k in ask}, f"{c['id']} {sectors} sectors {ask}")
        same(dev.render(v, c["c0"], c["c1"]), _columns(want, c["c0"], c["c1"]), f"{c['id']} {sectors} sectors [{c['c0']},{c['c1']})")


# ---- one context reused across draws ------------------------------------------------------------------

REUSE = [((7, 1), ("bowl-near360", "checker-near360", "coast-near360")), ((64, 1), ("bowl-near360", "checker-near360", "coast-near360")),
         ((3, 5), ("spikes-near360", "checker-near360", "coast-near360")), ((15, 4), ("coast-near360", "flat0-near360", "checker-near360"))]


@pytest.mark.parametrize("shape,grounds", REUSE, ids=lambda x: "%dx%d" % x if isinstance(x[0], int) else None)
def test_draws_into_a_framebuffer_smaller_than_a_segment_do_not_leak_into_the_next(shape, grounds):
    """one context, three grounds in turn with hz_hip_upload_mosaic between them - a ground that shows terrain, one that
    shows none, one that shows terrain (judged on the oracle's draws) - twice round, so that every framebuffer of the ring
    has held another ground: `touched` bytes and queue records of the draw before"""
    W, H = shape
    zoo = {c["name"]: c for c in hzutil.zoo_cases()}
    draws = []
    for name in grounds:
        z = zoo[name]
        view = dict(z["view"])
        view["aspect"] = float(np.float32(W) / np.float32(H))
        m, v = hzutil.zoo_mosaic(z["family"], z["N"]), oracle.make_view(**view)
        draws.append((name, m, v, oracle.render(m, v, W, H)))
    shown = [int((d[3]["index"] >= 0).sum()) for d in draws]
    assert shown[0] > 0 and shown[1] == 0 and shown[2] > 0, shown
    assert len({d[1].shape for d in draws}) == 1
    with hzutil.HipDev(draws[0][1], W, H) as dev:
        for rnd in range(2):
            for name, m, v, want in draws:
                assert dev.lib.hz_hip_upload_mosaic(dev.dev, m.ctypes.data) == 0
                same(dev.render(v), want, f"{W}x{H} round {rnd}: {name}")


# ---- the textured resolve -----------------------------------------------------------------------------

@pytest.mark.parametrize("case_id,seed", hzutil.SHAPE_TEX_CASES, ids=lambda x: x if isinstance(x, str) else None)
def test_textured_resolve_on_images_smaller_than_a_chunk_and_wider_than_65536(case_id, seed):
    """k_shade_tex walks chunks of 256 pixels: an image of one pixel, of one row of seven, of rows shorter than, and one
    pixel longer than, a chunk, of 70001 columns - against the oracle's textured draw (which oracle/make_golden.py holds
    to llvmpipe's where llvmpipe can draw the shape; the image's hash is the fixture's)"""
    c = BY_ID[case_id]
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    t, texels = hzutil.shape_tex_inputs(c, seed)
    t = hzutil.orc_tex(t)
    want = oracle.render(m, v, W, H, tex=t, texels=texels)
    assert SHAPE_GOLD[case_id]["tex_seed"] == seed and _sha(want["bgr"]) == SHAPE_GOLD[case_id]["tex_bgr_sha256"]
    assert (want["index"] >= 0).any() and not np.array_equal(want["bgr"], _oracle_full(case_id)["bgr"])
    with hzutil.HipDev(m, W, H) as dev:
        dev.set_texture(t, texels)
        for k in range(2):                              # render_to_host, then draw + resolve_to_host
            same(dev.render(v), want, f"{case_id} textured, call {k}")
        same(dev.render(v, c["c0"], c["c1"]), _columns(want, c["c0"], c["c1"]), f"{case_id} textured [{c['c0']},{c['c1']})")
        dev.texture_off()
        same(dev.render(v), _oracle_full(case_id), f"{case_id} plain again")


# ---- the Python mirror --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (64, 1)], ids=lambda s: "%dx%d" % s)
def test_python_mirror_on_one_row_and_odd_heights(shape):
    """horizonator.from_mosaic: hz_host.c derives the uniform values and its own tan(elevation) table (H = 1, odd H);
    render_full equals the oracle's draw of the values the context reports.  The vertical field of view follows the
    aspect: 360 degrees into one pixel look at all elevations at once, so narrower extents too"""
    import horizonator_amd
    W, H = shape
    N = 128
    m = hzutil.zoo_mosaic("bowl", N)                   # the viewer at the bottom: terrain at elevation 0 all round
    window = (1200, N // 2, 10, 45, 300, 417)          # cells per degree, radius, origin tile lon / lat, origin cell i / j
    lat, lon = 45.0 + (417 + N / 2 - 0.3) / 1200.0, 10.0 + (300 + N / 2 + 0.4) / 1200.0
    h = horizonator_amd.horizonator.from_mosaic(lat, lon, W, H, window, m)
    try:
        shown = 0
        for az0, az1 in ((-180.0, 180.0), (170.0, 530.0), (20.0, 110.0), (44.0, 46.0)):
            image, ranges, index, z24 = h.render_full(az0, az1, znear=10.0, zfar=30000.0)
            want = oracle.render(m, oracle.make_view(**h.view()), W, H)
            same(dict(bgr=image, ranges=ranges, index=index, z24=z24), want, f"{W}x{H} az [{az0},{az1}]")
            image2, ranges2 = h.render(az0, az1, znear=10.0, zfar=30000.0)
            assert np.array_equal(image2, want["bgr"]) and np.array_equal(ranges2, want["ranges"])
            shown += int((want["index"] >= 0).sum())
        assert shown > 0
    finally:
        h.close()


# ---- the size limit -----------------------------------------------------------------------------------

def test_create_refuses_images_of_2_to_the_29_pixels_and_sizes_below_one():
    lib = hzutil.hzlib.load()

    def err():
        return (lib.hz_hip_last_error() or b"").decode()
    for W, H in ((32768, 16384), (536870912, 1), (1, 536870912), (23171, 23171)):
        assert W * H >= 1 << 29
        assert not lib.hz_hip_create(0, 64, W, H)
        assert "images of up to 2^29 pixels" in err() and f"{W} x {H}" in err()
    for W, H in ((0, 5), (5, 0), (-1, 5), (5, -7)):
        assert not lib.hz_hip_create(0, 64, W, H)
        assert "bad sizes" in err()
