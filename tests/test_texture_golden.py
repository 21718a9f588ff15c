"""Texture path ("next" row N4): the oracle against what the reference's own shaders did
on Mesa llvmpipe (fixtures made by oracle/make_golden.py texture).  Textures are
hzutil.hash_texture(): the fixtures hold size and seed only."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import hzutil
import oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEXTURED = sorted(os.path.basename(p)[10:-4] for p in glob.glob(os.path.join(GOLD, "texrender_*.npz")))


def tex_of(g):
    """oracle.OrcTex from the t_* entries of a fixture"""
    t = oracle.OrcTex()
    for ours, theirs in (("viewer_lat_rad", "viewer_lat_rad"), ("origin_cell_lon_deg", "origin_cell_lon_deg"),
                         ("origin_cell_lat_deg", "origin_cell_lat_deg"), ("lon0", "texturemap_lon0"),
                         ("lon1", "texturemap_lon1"), ("dlat0", "texturemap_dlat0"), ("dlat1", "texturemap_dlat1"),
                         ("dlat2", "texturemap_dlat2")):
        setattr(t, ours, float(g["t_" + theirs]))
    t.ntiles_x, t.ntiles_y = int(g["t_NtilesX"]), int(g["t_NtilesY"])
    t.lowest_x, t.lowest_y = int(g["t_osmtile_lowestX"]), int(g["t_osmtile_lowestY"])
    t.tex_w, t.tex_h = t.ntiles_x * 256, t.ntiles_y * 256
    return t


def test_texture_coordinates_are_bit_identical_to_the_reference_shader():
    g = np.load(os.path.join(GOLD, "tex_vertex.npz"))
    t = tex_of(g)
    lib = oracle.load()
    N = int(g["N"])
    st = np.empty((N, N, 2), np.float32)
    buf = (C.c_float * 2)()
    for j in range(N):
        for i in range(N):
            lib.orc_vertex_tex(C.byref(t), float(g["u_deg_per_cell"]), i, j, C.byref(buf))
            st[j, i] = buf[:]
    assert np.array_equal(st.view(np.uint32), g["tex_st"].view(np.uint32))
    assert 0.0 < st.min() and st.max() < 1.0            # the DEM window lies inside the tile mosaic


def test_host_side_texture_parameters():
    """tile range, grid origin and Taylor coefficients (reference horizonator-lib.c:225-246,372-389,
    577-582,707-759,801): restated from the reference's host code, which cannot be built here;
    this pins the restatement against drift and checks it against the tile formula itself"""
    g = np.load(os.path.join(GOLD, "tex_vertex.npz"))
    d = hzutil.dem_dir_for(float(g["init_lat"]), float(g["init_lon"]), 48)
    od = oracle.Dem(float(g["init_lat"]), float(g["init_lon"]), d, radius_cells=48)
    t, want = od.texture(float(g["init_lat"]), float(g["init_lon"]), viewer_lat=float(g["viewer_lat"])), tex_of(g)
    for name, _ in oracle.OrcTex._fields_[:-1]:
        assert getattr(t, name) == getattr(want, name), name
    # slippy-map tile of a point, double precision: https://wiki.openstreetmap.org/wiki/Slippy_map_tilenames
    lat, lon = np.radians(float(g["init_lat"])), float(g["init_lon"])
    n = 2 ** 12
    x = int((lon + 180.0) / 360.0 * n)
    y = int((1.0 - np.arcsinh(np.tan(lat)) / np.pi) / 2.0 * n)
    assert t.lowest_x <= x < t.lowest_x + t.ntiles_x and t.lowest_y <= y < t.lowest_y + t.ntiles_y
    # the quadratic in dlat reproduces the exact tile y of the viewer's latitude at dlat = 0
    assert abs(t.dlat0 - (1.0 - np.arcsinh(np.tan(np.radians(float(g["viewer_lat"])))) / np.pi) / 2.0 * n) < 2e-3


def test_sampler_and_blend_on_probe_triangles():
    """GL_LINEAR/GL_REPEAT sampling of RGB8 textures (power-of-two and not, coordinates beyond
    [0,1]) and fragment.glsl's blend, drawn by llvmpipe through the reference's fragment shader"""
    g = np.load(os.path.join(GOLD, "tex_probe.npz"))
    W, H = int(g["W"]), int(g["H"])
    for k in range(int(g["n"])):
        th, tw, seed, blocky = (int(x) for x in g[f"tex{k}"])
        o = oracle.draw_triangles(g[f"tris{k}"], W, H, hzutil.hash_texture(th, tw, seed=seed, blocky=blocky))
        assert np.array_equal(o["bgr"], g[f"bgr{k}"]), (k, th, tw)


@pytest.mark.parametrize("name", TEXTURED)
def test_textured_draw_is_identical_to_the_reference_on_llvmpipe(name):
    g = np.load(os.path.join(GOLD, f"texrender_{name}.npz"))
    W, H = int(g["W"]), int(g["H"])
    v = oracle.make_view(**{k: float(g["u_" + k]) for k in oracle.VIEW_FIELDS})
    texels = hzutil.hash_texture(int(g["tex_h"]), int(g["tex_w"]), seed=int(g["tex_seed"]), blocky=int(g["tex_blocky"]))
    o = oracle.render(g["mosaic"], v, W, H, tex=tex_of(g), texels=texels, want=("bgr", "z24"))
    assert np.array_equal(o["z24"], g["z24"])
    assert np.array_equal(o["bgr"], g["bgr"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", TEXTURED)
def test_hip_textured_draw_is_identical_to_the_reference_on_llvmpipe(name):
    g = np.load(os.path.join(GOLD, f"texrender_{name}.npz"))
    W, H = int(g["W"]), int(g["H"])
    v = oracle.make_view(**{k: float(g["u_" + k]) for k in oracle.VIEW_FIELDS})
    texels = hzutil.hash_texture(int(g["tex_h"]), int(g["tex_w"]), seed=int(g["tex_seed"]), blocky=int(g["tex_blocky"]))
    hip = hzutil.hip_render(g["mosaic"], v, W, H, tex=tex_of(g), texels=texels)
    assert np.array_equal(hip["z24"], g["z24"])
    assert np.array_equal(hip["bgr"], g["bgr"])


# ---- the textured zoo (hzutil.zoo_tex_cases; tests/golden/zoo_tex_checksums.json holds what the reference's shaders drew) ----

ZOO = {c["name"]: c for c in hzutil.zoo_cases()}
ZOO_TEX = hzutil.zoo_tex_cases()


def _zoo_tex_gold():
    import json
    with open(os.path.join(GOLD, "zoo_tex_checksums.json")) as f:
        return json.load(f)


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _zoo_inputs(e):
    c = ZOO[e["name"]]
    t, texels = hzutil.zoo_tex_inputs(e, c)
    return c, hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"]), hzutil.orc_tex(t), texels


def test_zoo_tex_case_list_and_fixture_describe_the_same_cases():
    gold = _zoo_tex_gold()
    assert [e["id"] for e in ZOO_TEX] == list(gold)
    for e in ZOO_TEX:
        g = gold[e["id"]]
        assert (g["name"], g["placement"], g["ntiles_x"], g["ntiles_y"], g["tex_seed"], g["tex_blocky"]) == \
            (e["name"], e["placement"], *e["ntiles"], e["seed"], e["blocky"])
    # every zoo case once at least, every placement on eight cases or more, three cases under all seven
    assert {e["name"] for e in ZOO_TEX} == set(ZOO)
    for p in hzutil.ZOO_TEX_PLACEMENTS:
        assert sum(e["placement"] == p for e in ZOO_TEX) >= 8, p
    for name in hzutil.ZOO_TEX_FULL_CROSS:
        assert {e["placement"] for e in ZOO_TEX if e["name"] == name} == set(hzutil.ZOO_TEX_PLACEMENTS)
    # texture sizes: a power of two and not, on either axis
    assert {e["ntiles"] for e in ZOO_TEX} == set(hzutil.ZOO_TEX_TILES) and {e["blocky"] for e in ZOO_TEX} == {1, 4, 8}


def test_zoo_tex_placements_put_the_coordinates_where_they_say():
    """the window's corner vertices through the oracle's vertex stage: s and t as ZOO_TEX_PLACEMENTS lists them (t over
    one window height of latitude around the viewer's, who stands 0.3 of it north of the southern edge)"""
    c = ZOO["coast-arctic90"]
    N = c["N"]
    lib = oracle.load()
    buf = (C.c_float * 2)()
    for p, ((s_lo, s_hi), (t_lo, t_hi), curve) in hzutil.ZOO_TEX_PLACEMENTS.items():
        t = hzutil.orc_tex(hzutil.zoo_tex(c, p, (3, 2)))
        st = {}
        for i, j in ((0, 0), (N, N)):
            lib.orc_vertex_tex(C.byref(t), c["view"]["deg_per_cell"], i, j, C.byref(buf))
            st[i, j] = tuple(buf)
        # exact: s_lo + (s_hi-s_lo)*x, t_lo + (t_hi-t_lo)*(d - curve*d*d) with d = y - 0.3; float32 through offsets of 700 and 1600 tiles
        tol = 2e-3
        want_t = [t_lo + (t_hi - t_lo) * (d + curve * d * d) for d in (-0.3, 0.7)]
        assert abs(st[0, 0][0] - s_lo) < tol and abs(st[N, N][0] - s_hi) < tol, (p, st)
        assert abs(st[0, 0][1] - want_t[0]) < tol and abs(st[N, N][1] - want_t[1]) < tol, (p, st, want_t)


@pytest.mark.parametrize("entry", ZOO_TEX, ids=lambda e: e["id"])
def test_zoo_tex_oracle_draw_is_the_reference_draw(entry):
    """the oracle's textured draw of hand-made ground, under placements that wrap (GL_REPEAT on power-of-two and other
    sizes), minify, magnify, flip and straddle the seam: image and depth hash to what the reference's shaders drew"""
    g = _zoo_tex_gold()[entry["id"]]
    c, m, v, t, texels = _zoo_inputs(entry)
    o = oracle.render(m, v, c["W"], c["H"], tex=t, texels=texels, want=("bgr", "z24", "index"))
    assert _sha(o["bgr"]) == g["bgr_sha256"]
    assert _sha(o["z24"]) == g["z24_sha256"]
    terrain = o["index"] >= 0
    assert float(terrain.mean()) == g["terrain_fraction"]
    # the texture really is in the picture
    plain = oracle.render(m, v, c["W"], c["H"], want=("bgr",))["bgr"]
    assert np.array_equal(plain[~terrain], o["bgr"][~terrain])
    if not c["degenerate"]:
        differs = (plain != o["bgr"]).any(-1)[terrain].mean()
        print(f"{entry['id']}: textured differs from untextured on {100 * differs:.1f}% of the terrain pixels")
        assert differs >= 0.5
        if entry["placement"] != "magnified":                           # (a few texels over the whole window may hold no green)
            assert (o["bgr"][..., 1][terrain] > 0).any()                # green only comes from the texture


def clipped_runs_per_chunk(index, clipped_tri):
    """what k_shade_tex meets in a sector whose index image is `index` (top row first): per 256-pixel chunk of the
    sector's row-major pixel order, the number of runs (maximal stretches of equal triangle id, restarted with every
    chunk) that belong to a triangle the clipper cuts"""
    flat = index.reshape(-1).astype(np.int64)
    n = len(flat)
    k = np.arange(n)
    start = (flat >= 0) & ((k % 256 == 0) | (flat != np.concatenate([[-2], flat[:-1]])))
    hit = start & clipped_tri[np.maximum(flat, 0)]
    return np.bincount(k[hit] // 256, minlength=(n + 255) // 256)


def clipped_triangles(m, v):
    """bool per triangle id: one of its vertices lies outside the clip volume (|x|, |y| or |z| > 1); vertices of
    triangle p as hz_prim_cverts (hz_k_tex.h) takes them: cell p>>1, t = p&1"""
    N = m.shape[0]
    out = (np.abs(oracle.vertices(m, v)[..., :3]) > 1.0).any(-1)          # [j, i]
    a, b0, c0 = out[:-1, :-1], out[1:, 1:], out[1:, :-1]                 # t = 0: (i,j) (i+1,j+1) (i,j+1)
    b1, c1 = out[:-1, 1:], out[1:, 1:]                                    # t = 1: (i,j) (i+1,j)   (i+1,j+1)
    return np.stack([a | b0 | c0, a | b1 | c1], -1).reshape(-1)            # id = 2*(j*(N-1) + i) + t


@pytest.fixture(scope="module")
def zoo_runs():
    """index image and clipped-triangle table of the cases of hzutil.zoo_tex_sectors() and of plateau-near360"""
    out = {}
    for name in sorted({s[0] for s in hzutil.zoo_tex_sectors()} | {"plateau-near360"}):
        c = ZOO[name]
        m, v = hzutil.zoo_mosaic(c["family"], c["N"]), oracle.make_view(**c["view"])
        out[name] = oracle.render(m, v, c["W"], c["H"], want=("index",))["index"], clipped_triangles(m, v)
    return out


@pytest.mark.parametrize("sector", hzutil.zoo_tex_sectors(), ids=lambda s: "%s-%d-%d" % s)
def test_narrow_sectors_run_out_of_slots_for_clipped_triangles(sector, zoo_runs):
    """the sectors tests/test_gpu_texture_zoo.py draws do visit k_shade_tex's per-pixel fallback: a chunk with more
    clipped runs than the TX_MAXCLIP = 4 slots (judged on the oracle's index image, never on the code under test).
    The one-column sector is exempt: its whole image is one chunk or less, in which one triangle next to the viewer
    makes one run; it is drawn for its shape (every pixel a row of its own), and counted here all the same"""
    name, c0, c1 = sector
    index, clipped = zoo_runs[name]
    runs = clipped_runs_per_chunk(np.ascontiguousarray(index[:, c0:c1]), clipped)
    print(f"{name} [{c0},{c1}): {(runs > 4).sum()} of {len(runs)} chunks with more than 4 clipped runs, at most {runs.max()}")
    assert (runs > 4).any() or c1 - c0 == 1


def test_plateau_visits_both_the_slots_and_the_fallback(zoo_runs):
    index, clipped = zoo_runs["plateau-near360"]
    runs = clipped_runs_per_chunk(index, clipped)
    share = clipped[index[index >= 0]].mean()
    print(f"plateau-near360: {100 * share:.0f}% of the terrain pixels on clipped triangles; chunks with 1..4 clipped runs: "
          f"{((runs >= 1) & (runs <= 4)).sum()}, with more: {(runs > 4).sum()}, of {len(runs)}")
    assert ((runs >= 1) & (runs <= 4)).any() and (runs > 4).any()


# ---- host-side texture parameters elsewhere on Earth ----------------------------------------

def _tile_xy(lat_deg, lon_deg):
    """slippy-map tile coordinates at zoom 12, double precision"""
    n = 2 ** 12
    return (lon_deg + 180.0) / 360.0 * n, (1.0 - np.arcsinh(np.tan(np.radians(lat_deg))) / np.pi) / 2.0 * n


@pytest.mark.parametrize("place", sorted(hzutil.WORLD_CASES))
def test_host_side_texture_parameters_elsewhere_on_earth(place):
    """test_host_side_texture_parameters' two conditions south of the equator, east of Greenwich, across both lines and
    at 70 N: the tile of every corner of the window lies in the tile range, and the quadratic's constant is the exact
    tile y of the viewer's latitude"""
    c = hzutil.WORLD_CASES[place]
    od = oracle.Dem(c["lat"], c["lon"], hzutil.world_dem_dir(place), radius_cells=c["R"])
    r = c["R"] / 1200.0
    for viewer_lat in (c["lat"], c["moved"][0]):
        t = od.texture(c["lat"], c["lon"], viewer_lat=viewer_lat)
        assert (t.tex_w, t.tex_h) == (256 * t.ntiles_x, 256 * t.ntiles_y) and t.ntiles_x >= 1 and t.ntiles_y >= 1
        for lat in (c["lat"] - r, c["lat"] + r):
            for lon in (c["lon"] - r, c["lon"] + r):
                x, y = _tile_xy(lat, lon)
                assert t.lowest_x <= int(x) < t.lowest_x + t.ntiles_x and t.lowest_y <= int(y) < t.lowest_y + t.ntiles_y, (lat, lon)
        err = abs(t.dlat0 - _tile_xy(float(np.float32(viewer_lat)), 0.0)[1])
        print(f"{place} viewer latitude {viewer_lat}: dlat0 {t.dlat0} is {err:.2e} from the exact tile y")
        assert err < 2e-3
