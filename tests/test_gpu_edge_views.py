"""The HIP draw path where it decides by the viewer's place relative to the grid and its 63-cell strips.  Every other render
test keeps the viewer well inside the grid; here (hzutil.edge_cases()) it stands on a strip's first and last vertex column, on a
segment's first and last row, on the border, a hair (2^-40 cells) off a vertex, just outside the grid, far outside it and beyond
zfar, with the image's seam pointing at the grid - on N = 128 (63 + 63 + 1 cells) - and the grids are 2 .. 191 samples wide,
around one, two and three whole strips.  What these reach in hz_k_march.h and hz_plan.cpp: fast_strip / fast_rows with offsets of
zero and below 2^-30, rcp_south / rcp_north with the viewer's row at a segment's end and with every strip on one side, the
sector cull's viewer_inside margins and its seam test, far_strips / far_dd with the whole grid beyond zfar, has_vertex / has_cell
on a last strip of 1 .. 63 cells, empty zones, clamped near boxes and the one-round fallback.  Each draw is compared with the CPU
oracle bit for bit and hashes to what the reference's shaders drew on llvmpipe (tests/golden/edge_checksums.json;
tests/test_oracle_golden.py holds the oracle to the same hashes, which entitles these tests to its index and ranges)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import hzutil
import oracle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EDGES = hzutil.edge_cases()
BY_ID = {c["id"]: c for c in EDGES}
with open(os.path.join(GOLD, "edge_checksums.json")) as _f:
    EDGE_GOLD = json.load(_f)
# the positions on N = 128
POSITIONS = [next(c for c in EDGES if c["pos"] == p[0] and c["N"] == hzutil.EDGE_N) for p in hzutil._EDGE_POSITIONS]

_same = hzutil.same_render


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(c):
    return hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"])


_WANT = {}


def _want(c):
    """the oracle's whole image of a case, computed once and never changed"""
    if c["id"] not in _WANT:
        m, v = _inputs(c)
        _WANT[c["id"]] = oracle.render(m, v, c["W"], c["H"])
        for a in _WANT[c["id"]].values():
            a.setflags(write=False)
    return _WANT[c["id"]]


def _cols(want, c0, c1):
    return {k: a[:, c0:c1] for k, a in want.items()}


def _outside(c):
    i, j = c["view"]["viewer_cell_i"], c["view"]["viewer_cell_j"]
    return not (0 <= i <= c["N"] - 1 and 0 <= j <= c["N"] - 1)


def _plan(dev):
    """hz_hip_last_plan: rounds, coarse depth, reach, work list, vertex cache"""
    out = (C.c_int * 5)()
    assert dev.lib.hz_hip_last_plan(dev.dev, out) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("raster", [1, 2])
@pytest.mark.parametrize("case", EDGES, ids=lambda c: c["id"])
def test_edge_case_equals_the_oracle_and_the_reference_draw(case, raster):
    """a fresh context per draw: the case's sector against the oracle's, the whole image against the llvmpipe hashes"""
    m, v = _inputs(case)
    W, H = case["W"], case["H"]
    want = _want(case)
    hip = hzutil.hip_render(m, v, W, H, case["c0"], case["c1"], raster=raster)
    _same(hip, _cols(want, case["c0"], case["c1"]), f"{case['id']} raster {raster} [{case['c0']},{case['c1']})")
    if (case["c0"], case["c1"]) != (0, W):
        hip = hzutil.hip_render(m, v, W, H, raster=raster)
    g = EDGE_GOLD[case["id"]]
    assert _sha(m) == g["mosaic_sha256"]
    assert _sha(hip["bgr"]) == g["bgr_sha256"], "image differs from the reference's shaders' on llvmpipe"
    assert _sha(hip["z24"]) == g["z24_sha256"], "depth differs from the reference's shaders' on llvmpipe"
    terrain = hip["index"] >= 0
    assert int(terrain.sum()) == g["terrain_pixels"] and bool(terrain.any()) != case["empty"]
    assert np.array_equal((hip["ranges"] > 0) | np.isnan(hip["ranges"]), terrain) and hip["index"].max() < 2 * (case["N"] - 1) ** 2


def _sizes():
    return sorted({(c["N"], c["W"], c["H"]) for c in EDGES})


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "N%d_%dx%d" % s)
def test_edge_cases_of_one_size_share_a_context(size):
    """the default rasteriser on ONE context per mosaic and image size, the mosaic replaced between draws, viewers inside and
    outside the grid in turn (work lists, zones, near boxes and `touched` bytes of a draw from the other side of the border),
    twice round; in the second round the other half of the cases get their sector"""
    N, W, H = size
    mine = [c for c in EDGES if (c["N"], c["W"], c["H"]) == size]
    inside, outside = [c for c in mine if not _outside(c)], [c for c in mine if _outside(c)]
    order = []
    while inside or outside:
        if inside:
            order.append(inside.pop(0))
        if outside:
            order.append(outside.pop(0))
    with hzutil.HipDev(hzutil.zoo_mosaic(order[0]["family"], N), W, H, raster=0) as dev:
        for rnd in range(2):
            for k, c in enumerate(order):
                m, v = _inputs(c)
                assert dev.lib.hz_hip_upload_mosaic(dev.dev, m.ctypes.data) == 0
                c0, c1 = (c["c0"], c["c1"]) if rnd == 0 else (0, W) if (c["c0"], c["c1"]) != (0, W) else (W // 7, W - W // 9)
                _same(dev.render(v, c0, c1), _cols(_want(c), c0, c1), f"round {rnd} draw {k}: {c['id']} [{c0},{c1})")


_ONE_ROUND = {}


def _one_round(c, monkeypatch):
    """the case's sector in one round on the marching rasteriser, drawn once"""
    if c["id"] not in _ONE_ROUND:
        m, v = _inputs(c)
        monkeypatch.setenv("HZ_TWO_PASS", "0")
        with hzutil.HipDev(m, c["W"], c["H"], raster=2) as dev:
            _ONE_ROUND[c["id"]] = dev.render(v, c["c0"], c["c1"])
            assert _plan(dev)[0] == 1
    return _ONE_ROUND[c["id"]]


def _near_box_rounds(c, near_cells):
    """hz_plan_rounds' strips next to the viewer, clamped on one side each: two rounds if any is left"""
    nsx = (c["N"] - 1 + hzutil.MR_COLS - 1) // hzutil.MR_COLS
    vi = np.float32(c["view"]["viewer_cell_i"])
    x0 = max(0, int(np.floor((vi - np.float32(near_cells)) / np.float32(hzutil.MR_COLS))))
    x1 = min(nsx - 1, int(np.floor((vi + np.float32(near_cells)) / np.float32(hzutil.MR_COLS))))
    return 2 if x1 >= x0 else 1


@pytest.mark.parametrize("near_cells,hiz", [(4, None), (24, None), (200, None), (24, "0"), (24, "1")])
def test_forced_two_rounds_where_the_near_box_is_inside_cut_or_off_the_grid(near_cells, hiz, monkeypatch):
    """HZ_TWO_PASS=1 with a first round of 4, 24 and 200 cells, at 24 also with coarse depth forced on and off: the box of strips next to the
    viewer lies inside the grid, is cut by its edge, or misses it (near_x1 < near_x0: hz_plan_rounds falls back to one round,
    which hz_hip_last_plan reports) - same bytes as the oracle's and as one round's"""
    fallbacks = 0
    for c in POSITIONS:
        m, v = _inputs(c)
        one = _one_round(c, monkeypatch)
        if hiz is not None:
            monkeypatch.setenv("HZ_HIZ", hiz)
        monkeypatch.setenv("HZ_TWO_PASS", "1")
        monkeypatch.setenv("HZ_NEAR_CELLS", str(near_cells))
        with hzutil.HipDev(m, c["W"], c["H"], raster=2) as dev:
            two = dev.render(v, c["c0"], c["c1"])
            rounds = _plan(dev)[0]
        monkeypatch.delenv("HZ_HIZ", raising=False)
        monkeypatch.delenv("HZ_NEAR_CELLS")
        what = f"{c['id']} two rounds, reach {near_cells}, HZ_HIZ={hiz}"
        _same(two, _cols(_want(c), c["c0"], c["c1"]), what)
        _same(two, one, what + " vs one round")
        assert rounds == _near_box_rounds(c, near_cells), (what, rounds)
        fallbacks += rounds == 1
    # the three far_w_* positions and beyond_zfar stand more than 200 cells west of the grid: no strip within any of the reaches
    assert fallbacks >= 4, fallbacks


@pytest.mark.parametrize("tile_list", [None, 3])
def test_edge_positions_through_the_tile_lists(tile_list, monkeypatch):
    """HZ_TILES=1: first rounds by screen tile; HZ_TILE_LIST=3: lists so short that most tiles fall back"""
    for c in POSITIONS:
        m, v = _inputs(c)
        one = _one_round(c, monkeypatch)
        monkeypatch.setenv("HZ_TILES", "1")
        monkeypatch.setenv("HZ_TWO_PASS", "1")
        if tile_list is not None:
            monkeypatch.setenv("HZ_TILE_LIST", str(tile_list))
        got = hzutil.hip_render(m, v, c["W"], c["H"], c["c0"], c["c1"], raster=2)
        monkeypatch.delenv("HZ_TILES")
        monkeypatch.delenv("HZ_TILE_LIST", raising=False)
        _same(got, _cols(_want(c), c["c0"], c["c1"]), f"{c['id']} HZ_TILES=1 HZ_TILE_LIST={tile_list}")
        _same(got, one, f"{c['id']} by tile vs one round")


def _transform_groups():
    """every case with a zero or tiny offset and every outside case, grouped by grid size and position"""
    groups = {}
    for c in EDGES:
        if c["kind"] in ("vertex", "tiny", "out") or (c["kind"] == "size" and c["pos"] in ("corner", "outside")):
            groups.setdefault("N%d-%s" % (c["N"], c["pos"]), []).append(c)
    return sorted(groups.items())


@pytest.mark.parametrize("group", _transform_groups(), ids=lambda g: g[0])
def test_abridged_transform_equals_the_unabridged_one_at_the_edges(group, monkeypatch):
    """hz_fast.h's sequences are dropped per strip and per row where an offset is zero or below 2^-30 (tests/test_oracle_golden.py
    asserts that these cases have such offsets): the default transform and hz_transform_en() alone (HZ_NO_FAST_MATH=1), each
    against the oracle and against each other"""
    for c in group[1]:
        m, v = _inputs(c)
        W, H = c["W"], c["H"]
        monkeypatch.delenv("HZ_NO_FAST_MATH", raising=False)
        fast = hzutil.hip_render(m, v, W, H, raster=2)
        monkeypatch.setenv("HZ_NO_FAST_MATH", "1")
        plain = hzutil.hip_render(m, v, W, H, raster=2)
        _same(plain, _want(c), f"{c['id']} HZ_NO_FAST_MATH=1")
        _same(fast, _want(c), f"{c['id']} default transform")
        _same(fast, plain, f"{c['id']} abridged vs unabridged")


def _size_case(N, pos):
    return next(c for c in EDGES if c["kind"] == "size" and (c["N"], c["pos"]) == (N, pos))


VCACHE_IDS = [c["id"] for c in POSITIONS if c["pos"] in ("i63", "i126_j126", "i126_j0", "i126_j127", "i62.5_j63", "sw_corner", "e_border",
                                                          "tiny_ij", "out_w", "out_ne", "far_n_360", "seam_from_n")] + \
    [_size_case(N, pos)["id"] for N, pos in ((2, "outside"), (64, "corner"), (65, "outside"), (127, "corner"), (190, "outside"))]


@pytest.mark.parametrize("cid", VCACHE_IDS)
def test_vertex_cache_at_the_edges(cid):
    """hz_hip_set_options(vertex_cache=1): the same viewpoint drawn twice (the second draw fills the cache and reads it:
    k_march's VCACHE instance), a third time with other azimuth extents - each equal to the oracle's draw; hz_hip_last_plan
    says which draws came from the cache"""
    c = BY_ID[cid]
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    turned = dict(c["view"])
    turned["az_deg0"], turned["az_deg1"] = float(np.float32(c["view"]["az_deg0"] + 100.0)), float(np.float32(c["view"]["az_deg0"] + 300.0))
    v3 = oracle.make_view(**turned)
    with hzutil.HipDev(m, W, H, raster=2) as dev:
        dev.set_options(vertex_cache=1)
        o = hzutil.hzlib.Options()
        assert dev.lib.hz_hip_get_options(dev.dev, C.byref(o)) == 0
        used = []
        for k, (view, want) in enumerate(((v, _want(c)), (v, _want(c)), (v3, oracle.render(m, v3, W, H)))):
            _same(dev.render(view), want, f"{cid} draw {k}")
            used.append(_plan(dev)[4])
        # (a call drawn in several sectors draws from the viewpoint several times itself: tests/test_gpu_api.py)
        assert used[1:] == [1, 1] and (used[0] == 0 or o.host_sectors not in (0, 1)), used


HOST_SECTOR_IDS = [_size_case(N, "outside")["id"] for N in (5, 65, 129, 191)]


@pytest.mark.parametrize("sectors", [1, 3, 4])
@pytest.mark.parametrize("cid", HOST_SECTOR_IDS)
def test_host_delivery_in_sectors_of_which_one_holds_the_grid(cid, sectors, monkeypatch):
    """hz_hip_render_to_host in 1, 3 and 4 azimuth sectors from outside the grid: all of the terrain lies in one of them
    (judged on the oracle's draw), the others are sky - empty work lists, blobs without a pixel"""
    monkeypatch.setenv("HZ_HOST_SECTORS", str(sectors))
    c = BY_ID[cid]
    m, v = _inputs(c)
    W, H = c["W"], c["H"]
    want = _want(c)
    cols = np.flatnonzero((want["index"] >= 0).any(0))
    assert len(cols) and all(cols[0] * n // W == cols[-1] * n // W for n in (3, 4))
    with hzutil.HipDev(m, W, H) as dev:
        for k in range(3):                              # render_to_host, draw + resolve_to_host, render_to_host again
            _same(dev.render(v), want, f"{cid} {sectors} sectors call {k}")
        _same(dev.render(v, W // 3, W - 5), _cols(want, W // 3, W - 5), f"{cid} {sectors} sectors, part")


# ---- the public API on tiles on disk: viewpoints on, just outside and three cells outside the window -------------------

def _latlon_at(origin_tile, origin_cell, cpd, cell):
    """the float32 latitude or longitude whose window cell, formed as horizonator_move forms it (float32), is nearest `cell`"""
    f32 = np.float32
    x = f32(origin_tile + (origin_cell + cell) / cpd)
    best = None
    for _ in range(64):
        x = np.nextafter(x, f32(-1e9))
    for _ in range(129):
        got = (x - f32(origin_tile)) * f32(cpd) - f32(origin_cell)
        if best is None or abs(float(got) - cell) < best[0]:
            best = (abs(float(got) - cell), float(x))
        x = np.nextafter(x, f32(1e9))
    return best[1]


def _api_viewpoints(N):
    mid = N // 2 + 0.3
    return (("first column", 0.0, mid), ("last column", N - 1.0, mid), ("first row", mid, 0.0), ("last row", mid, N - 1.0),
            ("corner", 0.0, N - 1.0), ("half a cell west", -0.5, mid), ("half a cell north", mid, N - 0.5),
            ("three cells south-west", -3.0, -3.0), ("three cells east", N + 2.0, mid))


@pytest.mark.parametrize("explicit_z", [False, True], ids=["auto_z", "explicit_z"])
@pytest.mark.parametrize("place", ["equator_greenwich", "arctic_gap"])
def test_render_api_from_the_windows_border_and_beyond(place, explicit_z):
    """horizonator_move to viewpoints on the window's first and last sample rows and columns (as near as a float32 degree
    gets: 1e-5 cells at the equator, 5e-3 at 70 degrees north), half a cell and three cells outside it, with the automatic viewer height
    (the four samples around the viewer: beyond the window the tiles' own samples, -1 west and south of the first tile - the
    same in reference dem.c, through oracle.Dem) and with an explicit one: the view reported equals oracle.Dem.view() value
    for value, render_full() and render() equal the oracle's draw.  oracle.Dem refuses none of these viewpoints"""
    import horizonator_amd
    c = hzutil.WORLD_CASES[place]
    d = hzutil.world_dem_dir(place)
    W, H = 640, 160
    od = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"])
    m = od.mosaic()
    N, cpd = od.N, od.d.cells_per_deg
    h = horizonator_amd.horizonator(c["lat"], c["lon"], W, H, dir_dems=d, render_radius_cells=c["R"])
    try:
        shown = 0
        for k, (what, ci, cj) in enumerate(_api_viewpoints(N)):
            lon = _latlon_at(od.d.origin_tile[0], od.d.origin_cell[0], cpd, ci)
            lat = _latlon_at(od.d.origin_tile[1], od.d.origin_cell[1], cpd, cj)
            az0, az1, kw = ((-180.0, 180.0, dict(znear=10.0, zfar=60000.0)), (250.0, 400.0, dict(znear=100.0, zfar=20000.0)))[k % 2]
            vz = 1800.0 if explicit_z else -1.0
            ov = od.view(lat, lon, W, H, az0, az1, viewer_z=vz, **kw)
            assert abs(ov.viewer_cell_i - ci) < 6e-3 and abs(ov.viewer_cell_j - cj) < 6e-3, (what, ov.viewer_cell_i, ov.viewer_cell_j)
            want = oracle.render(m, ov, W, H)
            if explicit_z:
                z = C.c_float(vz)
                assert h._lib.horizonator_move(C.byref(h._ctx), C.byref(z), lat, lon)
                where = {}
            else:
                where = dict(lat=lat, lon=lon)
            image, ranges, index, z24 = h.render_full(az0, az1, **where, **kw)
            assert {n: np.float32(x) for n, x in h.view().items()} == {n: np.float32(x) for n, x in ov.as_dict().items()}, what
            _same(dict(bgr=image, ranges=ranges, index=index, z24=z24), want, f"{place} {what} render_full")
            image2, ranges2 = h.render(az0, az1, **where, **kw)
            assert np.array_equal(image2, want["bgr"]) and np.array_equal(ranges2, want["ranges"]), f"{place} {what} render"
            shown += bool((want["index"] >= 0).any())
        assert shown >= 6
    finally:
        h.close()
