"""The HIP path on ground it was not developed on.  Every other GPU render test draws the smooth closed-form surface of
tools/demgen.c around one place; here the ground is hzutil.zoo_mosaic()'s - exactly flat, a 0 / 8000 m checkerboard, one-sample
spikes, a cliff, a blocky coast, the top of the int16 range, borders of -1, a bowl around the viewer, stairs - under views
chosen to move the transform's operands (latitudes 0 .. 80, both cell sizes, a viewer 5 mm above sea level, on, below and far
above the ground).  Each draw is compared with the CPU oracle bit for bit, and its full image hashes to what the reference's
own shaders drew on llvmpipe (tests/golden/zoo_checksums.json; tests/test_oracle_golden.py holds the oracle to the same
hashes, which is what entitles these tests to the oracle's index and ranges).  Then the same DEM reader and kernels through
tiles on disk at three places outside the N/W quadrant, with voids, negative heights, samples above 16383 and a missing tile."""
import hashlib
import json
import os

import numpy as np
import pytest

import hzutil
import oracle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ZOO = hzutil.zoo_cases()
BY_FAMILY = {f: [c for c in ZOO if c["family"] == f] for f in hzutil.ZOO_FAMILIES}
with open(os.path.join(GOLD, "zoo_checksums.json")) as _f:
    ZOO_GOLD = json.load(_f)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(c):
    return hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"])


_same = hzutil.same_render        # (NaN ranges in the same places count as equal: see there)


def _check(c, what, raster=0):
    """one fresh context: the case's sector against the oracle's, all four outputs"""
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    hip = hzutil.hip_render(m, v, W, H, c["c0"], c["c1"], raster=raster)
    _same(hip, oracle.render(m, v, W, H, c["c0"], c["c1"]), f"{c['name']} {what}")
    return m, v, hip


@pytest.mark.parametrize("raster", [1, 2])
@pytest.mark.parametrize("case", ZOO, ids=lambda c: c["name"])
def test_zoo_case_equals_the_oracle_and_the_reference_draw(case, raster):
    m, v, hip = _check(case, f"raster {raster}", raster=raster)
    W, H = case["W"], case["H"]
    if (case["c0"], case["c1"]) != (0, W):
        hip = hzutil.hip_render(m, v, W, H, raster=raster)
    g = ZOO_GOLD[case["name"]]
    assert _sha(m) == g["mosaic_sha256"]
    assert _sha(hip["bgr"]) == g["bgr_sha256"], "image differs from the reference's shaders' on llvmpipe"
    assert _sha(hip["z24"]) == g["z24_sha256"], "depth differs from the reference's shaders' on llvmpipe"
    terrain = hip["index"] >= 0
    assert float(terrain.mean()) == g["terrain_fraction"]
    assert np.array_equal((hip["ranges"] > 0) | np.isnan(hip["ranges"]), terrain) and hip["index"].max() < 2 * (case["N"] - 1) ** 2


def _sizes():
    return sorted({(c["N"], c["W"], c["H"]) for c in ZOO})


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "N%d_%dx%d" % s)
def test_zoo_cases_of_one_size_share_a_context(size):
    """the default rasteriser on ONE context per mosaic and image size, the mosaic replaced between draws and the families
    interleaved (a flat draw after a checkerboard draw on the same framebuffers: `touched` bytes and queue records of the
    draw before), twice round so that every framebuffer of the ring has held a different ground"""
    N, W, H = size
    mine = [c for c in ZOO if (c["N"], c["W"], c["H"]) == size]
    # full ground first, empty ground next: order by the reference's terrain fraction, then take from both ends in turn
    mine.sort(key=lambda c: ZOO_GOLD[c["name"]]["terrain_fraction"])
    order = []
    while mine:
        order.append(mine.pop())
        if mine:
            order.append(mine.pop(0))
    with hzutil.HipDev(hzutil.zoo_mosaic(order[0]["family"], N), W, H, raster=0) as dev:
        for rnd in range(2):
            for k, c in enumerate(order):
                m, v = _inputs(c)
                assert dev.lib.hz_hip_upload_mosaic(dev.dev, m.ctypes.data) == 0
                # second round: the other half of the cases get their sector
                c0, c1 = (c["c0"], c["c1"]) if rnd == 0 else (0, W) if (c["c0"], c["c1"]) != (0, W) else (W // 7, W - W // 9)
                got = dev.render(v, c0, c1)
                _same(got, oracle.render(m, v, W, H, c0, c1), f"round {rnd} draw {k}: {c['name']} [{c0},{c1})")


def _family_cases(families):
    return [c for f in families for c in BY_FAMILY[f]]


QUEUE_FAMILIES = ("checker", "spikes", "cliff")


@pytest.mark.parametrize("raster", [1, 2])
@pytest.mark.parametrize("capacity", [1, 50])
@pytest.mark.parametrize("family", QUEUE_FAMILIES)
def test_tall_thin_triangles_everywhere_with_full_queues(family, capacity, raster, monkeypatch):
    """every near and middle-distance triangle is large on the screen: the medium and large queues overflow from every
    strip, not only from those next to the viewer; the overflow is rasterised in place"""
    monkeypatch.setenv("HZ_QUEUE_CAPACITY", str(capacity))
    for c in BY_FAMILY[family]:
        _check(c, f"HZ_QUEUE_CAPACITY={capacity} raster {raster}", raster=raster)


@pytest.mark.parametrize("tile_list", [None, 3])
@pytest.mark.parametrize("family", QUEUE_FAMILIES)
def test_tall_thin_triangles_through_the_tile_lists(family, tile_list, monkeypatch):
    """HZ_TILES=1: first rounds by screen tile; HZ_TILE_LIST=3: lists so short that most tiles fall back"""
    monkeypatch.setenv("HZ_TILES", "1")
    monkeypatch.setenv("HZ_TWO_PASS", "1")
    if tile_list is not None:
        monkeypatch.setenv("HZ_TILE_LIST", str(tile_list))
    for c in BY_FAMILY[family]:
        _check(c, f"HZ_TILES=1 HZ_TILE_LIST={tile_list}", raster=2)


@pytest.mark.parametrize("hiz", ["0", "1"])
@pytest.mark.parametrize("near_cells", [24, 96])
@pytest.mark.parametrize("family", ["cliff", "bowl", "coast", "flat0"])
def test_early_depth_test_where_half_or_nothing_is_hidden(family, near_cells, hiz, monkeypatch):
    """two rounds with the early depth test of the second (and k_hiz's coarse depth): a wall that hides half the field, a
    bowl and a sea that hide nothing, flat runs with depth ties along every shared edge - same bytes as one round's"""
    monkeypatch.setenv("HZ_HIZ", hiz)
    for c in BY_FAMILY[family]:
        m, v = _inputs(c)
        W, H = c["W"], c["H"]
        monkeypatch.setenv("HZ_TWO_PASS", "1")
        monkeypatch.setenv("HZ_NEAR_CELLS", str(near_cells))
        two = hzutil.hip_render(m, v, W, H, c["c0"], c["c1"], raster=2)
        _same(two, oracle.render(m, v, W, H, c["c0"], c["c1"]),
                                  f"{c['name']} two rounds, reach {near_cells}, HZ_HIZ={hiz}")
        monkeypatch.setenv("HZ_TWO_PASS", "0")
        one = hzutil.hip_render(m, v, W, H, c["c0"], c["c1"], raster=2)
        _same(two, one, f"{c['name']} two rounds vs one")


def _transform_cases():
    # heights up to 32767, -1 next to 500, h > 0 for every vertex, cos(lat) 0.17 and 1.0, the 5 mm viewer, infinite extents
    picked = _family_cases(("max16", "border_minus1", "bowl")) + \
        [c for c in ZOO if c["lat"] in (80.0, 0.0) or c["recipe"] in ("z005", "inf_color", "inf_far")]
    seen, out = set(), []
    for c in picked:
        if c["name"] not in seen:
            seen.add(c["name"])
            out.append(c)
    return out


@pytest.mark.parametrize("case", _transform_cases(), ids=lambda c: c["name"])
def test_abridged_transform_equals_the_unabridged_one(case, monkeypatch):
    """hz_fast.h's sequences are taken per draw, strip and row where the operands are in range: with them (the default)
    and with hz_transform_en() alone (HZ_NO_FAST_MATH=1), each against the oracle and against each other"""
    m, v = _inputs(case)
    W, H = case["W"], case["H"]
    want = oracle.render(m, v, W, H)
    monkeypatch.delenv("HZ_NO_FAST_MATH", raising=False)
    fast = hzutil.hip_render(m, v, W, H, raster=2)
    monkeypatch.setenv("HZ_NO_FAST_MATH", "1")
    plain = hzutil.hip_render(m, v, W, H, raster=2)
    _same(plain, want, f"{case['name']} HZ_NO_FAST_MATH=1")
    _same(fast, want, f"{case['name']} default transform")
    _same(fast, plain, f"{case['name']} abridged vs unabridged")


@pytest.mark.parametrize("family", ["checker", "coast", "max16", "border_minus1", "stairs"])
def test_vertex_cache_on_a_caller_supplied_zoo_mosaic(family):
    """the Python API's context over a mosaic the caller supplies: the same view drawn twice (the second from the vertex
    cache), a third time with other azimuth extents, then from a moved viewpoint - each equal to the oracle's draw of the
    uniform values the context reports"""
    import horizonator_amd
    N, W, H = 128, 640, 160
    m = hzutil.zoo_mosaic(family, N)
    window = (1200, N // 2, 10, 45, 300, 417)          # cells per degree, radius, origin tile lon / lat, origin cell i / j
    lat, lon = 45.0 + (417 + N / 2 - 0.3) / 1200.0, 10.0 + (300 + N / 2 + 0.4) / 1200.0
    h = horizonator_amd.horizonator.from_mosaic(lat, lon, W, H, window, m)
    try:
        assert np.array_equal(h.mosaic(), m)
        h.set_options(vertex_cache=1)
        used = []
        for k, (az0, az1, where) in enumerate([(-180.0, 180.0, {}), (-180.0, 180.0, {}), (170.0, 530.0, {}), (20.0, 110.0, {}),
                                               (-180.0, 180.0, dict(lat=lat + 0.004, lon=lon - 0.007)),
                                               (-180.0, 180.0, dict(lat=lat + 0.004, lon=lon - 0.007))]):
            image, ranges, index, z24 = h.render_full(az0, az1, znear=10.0, zfar=30000.0, **where)
            v = oracle.make_view(**h.view())
            want = oracle.render(m, v, W, H)
            _same(dict(bgr=image, ranges=ranges, index=index, z24=z24), want, f"{family} draw {k}")
            assert (want["index"] >= 0).any()
            used.append(h.last_plan()["vertex_cache"])
        # per viewpoint: a cold draw, then from the cache (a call drawn in several sectors draws from the viewpoint several
        # times itself, so its first call may use the cache already: tests/test_gpu_api.py's vertex cache test)
        if h.options()["host_sectors"] in (0, 1):
            assert used == [False, True, True, True, False, True], used
        else:
            assert all(used[1:4]) and used[5], used
    finally:
        h.close()


@pytest.mark.parametrize("sectors", [1, 3, 4])
@pytest.mark.parametrize("name", ["coast-sky", "flat0-sky", "checker-sky"])
def test_host_delivery_in_sectors_of_very_different_terrain_share(name, sectors, monkeypatch):
    """hz_hip_render_to_host in 1, 3 and 4 azimuth sectors: from 9000 m the window is a patch whose share of each sector
    differs widely (blobs of very different sizes, tiles without any terrain)"""
    monkeypatch.setenv("HZ_HOST_SECTORS", str(sectors))
    c = next(c for c in ZOO if c["name"] == name)
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    want = oracle.render(m, v, W, H)
    with hzutil.HipDev(m, W, H) as dev:
        for k in range(3):                              # render_to_host, draw + resolve_to_host, render_to_host again
            _same(dev.render(v), want, f"{name} {sectors} sectors call {k}")
        part = dev.render(v, c["W"] // 3, c["W"] - 5)
        for key in part:
            assert np.array_equal(part[key], want[key][:, c["W"] // 3:c["W"] - 5]), key
    g = ZOO_GOLD[name]
    assert _sha(want["bgr"]) == g["bgr_sha256"] and _sha(want["z24"]) == g["z24_sha256"]


# ---- tiles on disk, elsewhere on Earth ---------------------------------------

WORLD = sorted(hzutil.WORLD_CASES)


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("place", WORLD)
def test_either_ingest_builds_the_oracles_mosaic_elsewhere_on_earth(place, how, monkeypatch):
    """S/E tile names, a window over the equator and the prime meridian, a missing tile, voids (-32768), negative
    heights and samples above 16383 in the tiles: the window of reference dem.c either way"""
    import horizonator_amd
    c = hzutil.WORLD_CASES[place]
    d = hzutil.world_dem_dir(place)
    monkeypatch.setenv("HORIZONATOR_INGEST", how)
    want = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"]).mosaic()
    assert want.min() == 0 and want.max() > 16383 and (want == 0).mean() > 0.2
    h = horizonator_amd.horizonator(c["lat"], c["lon"], 64, 16, dir_dems=d, render_radius_cells=c["R"])
    try:
        assert np.array_equal(h.mosaic(), want), (place, how)
    finally:
        h.close()


@pytest.mark.parametrize("place", WORLD)
def test_renders_elsewhere_on_earth_equal_the_oracle(place):
    """horizonator_init / move / pan_zoom / set_zextents away from the benchmark's viewpoint: render() and render_full()
    for the initial and for a moved viewpoint, whole panorama and a wrapped part of it"""
    import horizonator_amd
    c = hzutil.WORLD_CASES[place]
    d = hzutil.world_dem_dir(place)
    W, H = 801, 203
    od = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"])
    m = od.mosaic()
    h = horizonator_amd.horizonator(c["lat"], c["lon"], W, H, dir_dems=d, render_radius_cells=c["R"])
    try:
        for lat, lon in ((c["lat"], c["lon"]), c["moved"]):
            for az0, az1, kw in ((-180.0, 180.0, dict(znear=10.0, zfar=60000.0)),
                                 (250.0, 400.0, dict(znear=100.0, zfar=20000.0, znear_color=500.0, zfar_color=9000.0))):
                want = oracle.render(m, od.view(lat, lon, W, H, az0, az1, **kw), W, H)
                image, ranges, index, z24 = h.render_full(az0, az1, lat=lat, lon=lon, **kw)
                _same(dict(bgr=image, ranges=ranges, index=index, z24=z24), want, f"{place} ({lat},{lon}) az [{az0},{az1}]")
                image2, ranges2 = h.render(az0, az1, lat=lat, lon=lon, **kw)
                assert np.array_equal(image2, want["bgr"]) and np.array_equal(ranges2, want["ranges"])
                assert 0.05 < (want["index"] >= 0).mean()
            assert {k: np.float32(x) for k, x in h.view().items()} == \
                {k: np.float32(x) for k, x in od.view(lat, lon, W, H, az0, az1, **kw).as_dict().items()}
    finally:
        h.close()
