"""The textured resolve (k_shade_tex in hz_k_tex.h, the sampler and blend of hz_tex.h, the textured branches of
hz_convert.cpp and hz_hostpath.cpp) on the terrain zoo.  On the smooth surface of the other textured tests a handful of
triangles next to the viewer are cut by the clipper; on hzutil.zoo_mosaic()'s ground most of the picture is, so the
kernel's LDS slots for clipped pieces run out and its per-pixel fallback shades the rest (tests/test_texture_golden.py
counts that on the oracle's index image).  The texture placements of hzutil.ZOO_TEX_PLACEMENTS add what textures inside
(0, 1) never gave the sampler: GL_REPEAT far outside [0, 1] on power-of-two and other sizes, minification, magnification,
decreasing s, the seam itself.  Each draw is compared with the CPU oracle bit for bit, and its full image hashes to what
the reference's shaders drew on llvmpipe (tests/golden/zoo_tex_checksums.json; tests/test_texture_golden.py holds the
oracle to the same hashes)."""
import contextlib
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import hzutil
import oracle
from test_gpu_terrain_zoo import _same

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ZOO = {c["name"]: c for c in hzutil.zoo_cases()}
ZOO_TEX = hzutil.zoo_tex_cases()
BY_ID = {e["id"]: e for e in ZOO_TEX}
with open(os.path.join(GOLD, "zoo_tex_checksums.json")) as _f:
    ZOO_TEX_GOLD = json.load(_f)
FULL_CROSS = [hzutil.zoo_tex_entry(name) for name in hzutil.ZOO_TEX_FULL_CROSS]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(e):
    """zoo case, mosaic, view, texture parameters (as the oracle takes them) and texels of an entry of zoo_tex_cases()"""
    c = ZOO[e["name"]]
    t, texels = hzutil.zoo_tex_inputs(e, c)
    return c, hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"]), hzutil.orc_tex(t), texels


@functools.lru_cache(maxsize=4)
def _oracle_full(entry_id):
    """the oracle's textured draw of an entry's whole image: computed once, shared by the tests of that entry, never
    written to"""
    c, m, v, t, texels = _inputs(BY_ID[entry_id])
    out = oracle.render(m, v, c["W"], c["H"], tex=t, texels=texels)
    for a in out.values():
        a.setflags(write=False)
    return out


def _columns(full, c0, c1):
    return {k: a[:, c0:c1] for k, a in full.items()}


@pytest.fixture(scope="module")
def contexts():
    """one context per mosaic and image size for the whole file: making a context costs several draws' time, and
    replacing the mosaic and the texture between draws is part of what is under test"""
    devs = {}
    yield devs
    for dev in devs.values():
        dev.close()


@contextlib.contextmanager
def _context(contexts, c, m, raster=0):
    """the file's context of zoo case c's size, holding mosaic m; a test that fails on it gives it up"""
    key = (c["N"], c["W"], c["H"])
    dev = contexts.pop(key, None) or hzutil.HipDev(m, c["W"], c["H"])
    try:
        assert dev.lib.hz_hip_set_raster(dev.dev, raster) == 0
        assert dev.lib.hz_hip_upload_mosaic(dev.dev, np.ascontiguousarray(m, np.int16).ctypes.data) == 0
        yield dev
    except BaseException:
        dev.close()
        raise
    contexts[key] = dev


# ---- a. every entry, both rasterisers ------------------------------------------------------------

@pytest.mark.parametrize("raster", [1, 2])                  # (the rasterisers of one entry next to each other: one oracle draw)
@pytest.mark.parametrize("entry", ZOO_TEX, ids=lambda e: e["id"])
def test_zoo_tex_entry_equals_the_oracle_and_the_reference_draw(entry, raster, contexts):
    c, m, v, t, texels = _inputs(entry)
    W, H = c["W"], c["H"]
    want = _oracle_full(entry["id"])
    with _context(contexts, c, m, raster) as dev:
        dev.set_texture(t, texels)
        if (c["c0"], c["c1"]) != (0, W):
            _same(dev.render(v, c["c0"], c["c1"]), _columns(want, c["c0"], c["c1"]),
                  f"{entry['id']} raster {raster} [{c['c0']},{c['c1']})")
        hip = dev.render(v)
    _same(hip, want, f"{entry['id']} raster {raster}")
    g = ZOO_TEX_GOLD[entry["id"]]
    assert _sha(hip["bgr"]) == g["bgr_sha256"], "image differs from the reference's shaders' on llvmpipe"
    assert _sha(hip["z24"]) == g["z24_sha256"], "depth differs from the reference's shaders' on llvmpipe"
    assert float((hip["index"] >= 0).mean()) == g["terrain_fraction"]


# ---- b. narrow and odd sectors --------------------------------------------------------------------

def _sector_cases():
    by_name = {}
    for name, c0, c1 in hzutil.zoo_tex_sectors():
        by_name.setdefault(name, []).append((c0, c1))
    return sorted(by_name.items())


@pytest.mark.parametrize("name,sectors", _sector_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_narrow_sectors_where_clipped_triangles_start_a_run_on_every_row(name, sectors, contexts):
    """sectors 1, 17, 63, 64 and 65 columns wide: a 256-pixel chunk spans up to 256 rows, the clipped triangles next to
    the viewer start a run on each of them, and all but the first four runs take the per-pixel path.  Each sector against
    the oracle's draw of that sector and against the same columns of the full textured image"""
    e = hzutil.zoo_tex_entry(name)
    c, m, v, t, texels = _inputs(e)
    W, H = c["W"], c["H"]
    with _context(contexts, c, m) as dev:
        dev.set_texture(t, texels)
        full = dev.render(v)
        _same(full, _oracle_full(e["id"]), f"{e['id']} whole")
        for c0, c1 in sectors:
            part = dev.render(v, c0, c1)
            _same(part, oracle.render(m, v, W, H, c0, c1, tex=t, texels=texels), f"{e['id']} [{c0},{c1}) against the oracle's sector")
            _same(part, _columns(full, c0, c1), f"{e['id']} [{c0},{c1}) against the whole image")


# ---- c. more chunks than the launch has blocks ------------------------------------------------------

@pytest.mark.parametrize("name", ["checker-near360", "coast-near360"])
def test_image_of_more_chunks_than_blocks_walks_the_grid_stride_loop(name):
    """8192x520 pixels are 16 640 chunks, the launch is capped at 256*64 blocks: the last 256 chunks (the bottom eight
    rows) are the second trip of 256 blocks, whose LDS tables held another chunk before"""
    c = ZOO[name]
    W, H = 8192, 520
    assert (W * H + 255) // 256 == 256 * 64 + 256
    m = hzutil.zoo_mosaic(c["family"], c["N"])
    v = oracle.make_view(**dict(c["view"], aspect=float(np.float32(W) / np.float32(H))))
    t = hzutil.orc_tex(hzutil.zoo_tex(c, "wrap", (3, 2)))
    texels = hzutil.hash_texture(t.tex_h, t.tex_w, seed=5, blocky=1)
    want = oracle.render(m, v, W, H, tex=t, texels=texels)
    assert (want["index"][-8:] >= 0).mean() >= 0.9, "the second trip would shade next to nothing"
    _same(hzutil.hip_render(m, v, W, H, tex=t, texels=texels), want, f"{name} {W}x{H}")


# ---- d. one context, many hand-overs ----------------------------------------------------------------

def _sizes():
    return sorted({(c["N"], c["W"], c["H"]) for c in ZOO.values()})


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "N%d_%dx%d" % s)
def test_textured_and_plain_draws_alternate_on_one_context(size):
    """ONE context per mosaic and image size, the mosaic replaced between draws and the families interleaved, twice
    round the framebuffer ring.  A textured resolve leaves the framebuffer for the next draw to clear, a plain one clears
    behind itself: here each follows the other, on different ground.  Along the way the texture is replaced by one of
    another size, the parameters alone are replaced, parameters of another size are refused, and a textured context is
    asked for everything but the colour.  Every draw against the oracle"""
    N, W, H = size
    mine = [e for e in ZOO_TEX if (ZOO[e["name"]]["N"], ZOO[e["name"]]["W"], ZOO[e["name"]]["H"]) == size]
    mine.sort(key=lambda e: ZOO_TEX_GOLD[e["id"]]["terrain_fraction"])
    order = []
    while mine:                                         # full ground first, empty ground next
        order.append(mine.pop())
        if mine:
            order.append(mine.pop(0))
    seen, resident = set(), None
    with hzutil.HipDev(hzutil.zoo_mosaic(ZOO[order[0]["name"]]["family"], N), W, H, raster=0) as dev:
        n = 0
        for rnd in range(2):
            for e in order:
                c, m, v, t, texels = _inputs(e)
                assert dev.lib.hz_hip_upload_mosaic(dev.dev, m.ctypes.data) == 0
                c0, c1 = (c["c0"], c["c1"]) if rnd == 0 else (0, W) if (c["c0"], c["c1"]) != (0, W) else (W // 7, W - W // 9)
                what = f"draw {n}: {e['id']} [{c0},{c1})"
                step = n % 4
                n += 1
                if step == 1:
                    # off: a clearing resolve behind a textured one
                    dev.texture_off()
                    _same(dev.render(v, c0, c1), oracle.render(m, v, W, H, c0, c1), what + " untextured")
                    seen.add("off")
                    continue
                # on (again), with this entry's texture: of another size than the resident one more often than not
                dev.set_texture(t, texels)
                if resident not in (None, (t.tex_w, t.tex_h)):
                    seen.add("resized")
                resident = (t.tex_w, t.tex_h)
                if step == 2:
                    # a textured context asked for everything but the colour: the plain draw's arrays, a clearing resolve
                    got = dev.render(v, c0, c1, want=("ranges", "index", "z24"))
                    assert sorted(got) == ["index", "ranges", "z24"]
                    _same(got, oracle.render(m, v, W, H, c0, c1, want=("ranges", "index", "z24")), what + " without the colour")
                    seen.add("subset")
                if step == 3:
                    # parameters of another size without texels: refused with a message, nothing changes ...
                    other = hzutil.zoo_tex(c, "inside", (e["ntiles"][1] + 1, e["ntiles"][0]))
                    assert (other.tex_w, other.tex_h) != (t.tex_w, t.tex_h)
                    assert dev.set_texparams(other) != 0 and b"size" in dev.lib.hz_hip_last_error()
                    _same(dev.render(v, c0, c1), oracle.render(m, v, W, H, c0, c1, tex=t, texels=texels), what + " after a refusal")
                    # ... and the parameters alone for the resident texture: another placement of the same texels
                    p2 = "flipped" if e["placement"] != "flipped" else "far_out"
                    t = hzutil.orc_tex(hzutil.zoo_tex(c, p2, e["ntiles"]))
                    assert dev.set_texparams(t) == 0, dev.lib.hz_hip_last_error()
                    what += f" moved to {p2}"
                    seen.add("params")
                _same(dev.render(v, c0, c1), oracle.render(m, v, W, H, c0, c1, tex=t, texels=texels), what)
    # what the docstring promises did happen (a group of one case makes two draws only)
    assert len(order) < 2 or {"off", "subset", "params"} <= seen
    assert len({e["ntiles"] for e in order}) < 2 or "resized" in seen


# ---- e. option switches --------------------------------------------------------------------------------

# name -> fields of hz_options_t (what hz_options_from_env makes of HZ_RESOLVE_CLEARS=0, HZ_TWO_PASS=1 HZ_NEAR_CELLS=24,
# HZ_TILES=1 HZ_TWO_PASS=1 (HZ_TILE_LIST=3), HZ_HOST_SECTORS=1/3/4, HZ_NO_FAST_MATH=1; host_dense), rasteriser
SWITCHES = {
    "resolve_clears_0": (dict(resolve_clears=0), 0),
    "two_pass_near24":  (dict(rounds=2, near_cells=24), 2),
    "tiles":            (dict(tiles=1, rounds=2), 2),
    "tiles_list3":      (dict(tiles=1, rounds=2, tile_list=3), 2),
    "host_sectors_1":   (dict(host_sectors=1), 0),
    "host_sectors_3":   (dict(host_sectors=3), 0),
    "host_sectors_4":   (dict(host_sectors=4), 0),
    "no_fast_math":     (dict(fast_math=0), 2),
    "host_dense":       (dict(host_dense=1), 0),
}


def _three_calls(dev, entry, v, t, texels, W, what):
    """the one-call delivery, draw + resolve_to_host (or the reverse), then a sector"""
    want = _oracle_full(entry["id"])
    dev.set_texture(t, texels)
    for k in range(2):
        _same(dev.render(v), want, f"{entry['id']} {what} call {k}")
    _same(dev.render(v, W // 3, W - 5), _columns(want, W // 3, W - 5), f"{entry['id']} {what} sector")


@pytest.mark.parametrize("entry", FULL_CROSS, ids=lambda e: e["id"])
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_textured_draw_under_every_option_switch(switch, entry, contexts):
    """none of the switches changes a byte of a picture, textured included.  The options are set on the file's context
    (hz_hip_set_options: the fields the environment variables of the same names set when a context is made) and put back"""
    fields, raster = SWITCHES[switch]
    c, m, v, t, texels = _inputs(entry)
    with _context(contexts, c, m, raster) as dev:
        before, o = hzutil.hzlib.Options(), hzutil.hzlib.Options()
        assert dev.lib.hz_hip_get_options(dev.dev, C.byref(before)) == 0 and dev.lib.hz_hip_get_options(dev.dev, C.byref(o)) == 0
        for k, x in fields.items():
            setattr(o, k, x)
        assert dev.lib.hz_hip_set_options(dev.dev, C.byref(o)) == 0
        _three_calls(dev, entry, v, t, texels, c["W"], switch)
        assert dev.lib.hz_hip_set_options(dev.dev, C.byref(before)) == 0


@pytest.mark.parametrize("entry", FULL_CROSS, ids=lambda e: e["id"])
def test_textured_draw_with_queues_of_one_record(entry, monkeypatch):
    """HZ_QUEUE_CAPACITY=1 (read when a context is made: the queues exist from then on): every large triangle overflows
    its queue and is rasterised in place"""
    monkeypatch.setenv("HZ_QUEUE_CAPACITY", "1")
    c, m, v, t, texels = _inputs(entry)
    with hzutil.HipDev(m, c["W"], c["H"], raster=2) as dev:
        _three_calls(dev, entry, v, t, texels, c["W"], "HZ_QUEUE_CAPACITY=1")


# ---- f. through the API, elsewhere on Earth --------------------------------------------------------------

@pytest.mark.parametrize("place", sorted(hzutil.WORLD_CASES))
def test_render_texture_through_the_api_elsewhere_on_earth(place, tmp_path):
    """horizonator_init's tile range and horizonator_move's Taylor coefficients (hz_host.c) south of the equator, east
    of Greenwich, across both lines and at 70 N, over PNG tiles on disk: the layout, a whole panorama and one from a
    moved viewpoint against the oracle's textured draw"""
    import horizonator_amd
    c = hzutil.WORLD_CASES[place]
    d = hzutil.world_dem_dir(place)
    W, H = 640, 160
    od = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"])
    m = od.mosaic()
    t = od.texture(c["lat"], c["lon"])
    texels = hzutil.write_map_tiles(tmp_path, "mapnik", t.lowest_x, t.lowest_y, t.ntiles_x, t.ntiles_y, 21)
    h = horizonator_amd.horizonator(c["lat"], c["lon"], W, H, render_texture=True, dir_dems=d, dir_tiles=str(tmp_path),
                                    allow_downloads=False, render_radius_cells=c["R"])
    try:
        assert h.texture_layout() == (t.lowest_x, t.lowest_y, t.ntiles_x, t.ntiles_y)
        for lat, lon in ((c["lat"], c["lon"]), c["moved"]):
            kw = dict(znear=10.0, zfar=60000.0)
            tv = od.texture(c["lat"], c["lon"], viewer_lat=lat)
            want = oracle.render(m, od.view(lat, lon, W, H, -180.0, 180.0, **kw), W, H, tex=tv, texels=texels)
            assert 0.05 < (want["index"] >= 0).mean()
            image, ranges, index, z24 = h.render_full(-180.0, 180.0, lat=lat, lon=lon, **kw)
            _same(dict(bgr=image, ranges=ranges, index=index, z24=z24), want, f"{place} textured from ({lat},{lon})")
            plain = oracle.render(m, od.view(lat, lon, W, H, -180.0, 180.0, **kw), W, H, want=("bgr",))["bgr"]
            assert ((plain != want["bgr"]).any(-1)[want["index"] >= 0]).mean() >= 0.5
    finally:
        h.close()
