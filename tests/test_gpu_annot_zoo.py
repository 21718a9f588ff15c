"""The consumers of the framebuffer - k_link_cells, k_poi, hz_hip_read_depth and their host halves (horizonator_pick,
horizonator_amd_link_cells, horizonator_amd_poi_visibility) - on the terrain zoo.

(a) the kernels alone, through the C-ABI, on ten zoo draws (tests/annot_cases.py) and a not-quite-360 degree variant of each
    full-circle view: link cells of four sizes under three cut-offs, the crafted and the projected points of interest under
    five cut-offs and in counts around the 256-thread block, the depth of some 200 pixels; the refusals; a sector; a textured
    context.
(b) call order: the readers after every call that consumes, replaces or keeps the framebuffer, with and without the
    conversions' fused clear, and on a context that has drawn nothing.
(c) the host halves through the Python API on the synthetic DEM.

Every expectation is tests/naive_annot.py applied to the ORACLE's render of the same uniforms, never to the device's own
output, and every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import annot_cases as ac
import hzutil
import naive_annot as na
import oracle

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(12345.0)


class Ctx:
    """one device context per input, made once for the module's tests of that input"""

    def __init__(self, key):
        self.key, self.c = key, ac.INPUTS[key]
        self.W, self.H = self.c["W"], self.c["H"]
        self.view = oracle.make_view(**self.c["view"])
        self.dev = hzutil.HipDev(ac.mosaic(key), self.W, self.H)
        self.cos_lat = ac.cos_lat(key)

    def link(self, cw, ch, cut, tables=None, **kw):
        c = self.c
        nx, ny, s, co, e = tables or na.link_tables(self.W, self.H, c["view"]["az_deg0"], c["view"]["az_deg1"], cw, ch, cut)
        return self.dev.link_cells(self.view, s, co, e, c["lat"], self.cos_lat, c["lon"], cw, ch, nx, ny, **kw)

    def check_link(self, cw, ch, cut, what=""):
        rc, la, lo = self.link(cw, ch, cut)
        assert rc == 0, self.dev.last_error()
        wla, wlo = ac.want_link(self.key, cw, ch, cut)
        assert la.shape == wla.shape
        for got, want, name in ((la, wla, "lat"), (lo, wlo, "lon")):
            if not np.array_equal(got, want, equal_nan=True):
                bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
                raise AssertionError(f"{self.key} {what} cells {cw}x{ch} cut {cut}: {name} differs in {len(bad)} cells, first "
                                     f"{bad[0]}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")

    def check_poi(self, cut, n=None, what=""):
        p = ac.proj_list(self.key)
        n = len(p) if n is None else n
        rc, vis, x, y = self.dev.poi(self.view, p[:n], cut)
        assert rc == 0, self.dev.last_error()
        wvis, wx, wy, tags = ac.want_poi(self.key, cut)
        for got, want, name in ((vis, wvis[:n], "visible"), (x, wx[:n], "label_x"), (y, wy[:n], "label_y")):
            if not np.array_equal(got, want):
                k = int(np.flatnonzero(got != want)[0])
                raise AssertionError(f"{self.key} {what} cut {cut}, {n} points: {name} differs at {(got != want).sum()} points, first {k} "
                                     f"{p[k].tolist()} {sorted(tags[k])}: {got[k]!r} for {want[k]!r}")

    def check_depth(self, pixels, c0=0, what=""):
        z = ac.want_render(self.key)["z24"]
        for x, y in pixels:
            rc, got = self.dev.read_depth(x, y)
            assert rc == 0 and got == int(z[y, x]), f"{self.key} {what} depth at ({x},{y}): rc {rc}, {got:#x} for {int(z[y, x]):#x}"

    def check_readers(self, what, npix=25):
        self.check_link(14, 14, 0, what)
        self.check_poi(20, None, what)
        self.check_depth(ac.depth_pixels(self.key, n=npix), what=what)


@pytest.fixture(scope="module", params=ac.KEYS)
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.dev.close()


# ---- (a) the kernels alone ------------------------------------------------------------------------------------------------

def test_link_cells_of_every_size_and_cut(ctx):
    ctx.dev.draw(ctx.view)
    ran = 0
    for cw, ch, cut in ac.cells_and_cuts(ctx.W, ctx.H):
        nx, ny = na.link_tables(ctx.W, ctx.H, 0.0, 1.0, cw, ch, cut)[:2]
        if nx > 0 and ny > 0:
            ctx.check_link(cw, ch, cut)
            ran += 1
        else:
            rc, la, lo = ctx.link(cw, ch, cut)
            assert rc == -1 and ctx.dev.last_error() and (la == SENTINEL).all() and (lo == SENTINEL).all(), (cw, ch, cut, nx, ny)
    assert ran >= 8


def test_link_cells_refusals_write_nothing(ctx):
    ctx.dev.draw(ctx.view)
    nx, ny, s, co, e = na.link_tables(ctx.W, ctx.H, ctx.c["view"]["az_deg0"], ctx.c["view"]["az_deg1"], 14, 14, 0)
    for tables in ((0, ny, s, co, e), (nx, 0, s, co, e), (-3, ny, s, co, e), (nx, -1, s, co, e),
                   (nx, ny, None, co, e), (nx, ny, s, None, e), (nx, ny, s, co, None)):
        rc, la, lo = ctx.link(14, 14, 0, tables=tables)
        assert rc == -1 and "hz_hip_link_cells" in ctx.dev.last_error(), tables[:2]
        assert (la == SENTINEL).all() and (lo == SENTINEL).all()
    ctx.check_link(14, 14, 0, "after the refusals")


def test_points_of_interest_under_every_cut_and_count(ctx):
    ctx.dev.draw(ctx.view)
    cuts = ac.cuts_poi(ctx.H)
    for cut in cuts:
        ctx.check_poi(cut)
    for k, n in enumerate(ac.COUNTS):
        ctx.check_poi(cuts[k % len(cuts)], n)
        ctx.check_poi(0, n)
    assert len(ac.proj_list(ctx.key)) > 1000


def test_read_depth_is_the_oracles_z24(ctx):
    ctx.dev.draw(ctx.view)
    px = ac.depth_pixels(ctx.key)
    assert len(px) >= 200
    ctx.check_depth(px)
    for x, y in ((-1, 0), (ctx.W, 0), (0, -1), (0, ctx.H)):
        rc, z = ctx.dev.read_depth(x, y)
        assert rc == -1 and z == 0xDEADBEEF and "hz_hip_read_depth" in ctx.dev.last_error()


def test_sector_context_refuses_the_passes_and_reads_depth_with_its_own_stride(ctx):
    c0, c1 = ctx.c["zoo"]["c0"], ctx.c["zoo"]["c1"]
    if (c0, c1) == (0, ctx.W):
        c0, c1 = ctx.W // 5 + 3, ctx.W // 5 + 3 + ctx.W // 3
    ctx.dev.draw(ctx.view, c0, c1)
    try:
        rc, la, lo = ctx.link(14, 14, 0)
        assert rc == -1 and "full-width" in ctx.dev.last_error() and (la == SENTINEL).all() and (lo == SENTINEL).all()
        rc, vis, x, y = ctx.dev.poi(ctx.view, ac.proj_list(ctx.key)[:300], 0)
        assert rc == -1 and "full-width" in ctx.dev.last_error() and (vis == 77).all() and (x == 77).all() and (y == 77).all()
        ctx.check_depth(ac.depth_pixels(ctx.key, c0, c1), what=f"sector [{c0},{c1})")
        for x, y in ((c0 - 1, 5), (c1, 5), (c0, -1), (c0, ctx.H), (c1 - 1, ctx.H)):
            rc, z = ctx.dev.read_depth(x, y)
            assert rc == -1 and z == 0xDEADBEEF, (x, y)
    finally:
        ctx.dev.draw(ctx.view)
    ctx.check_readers("full width again")


def test_textured_context_gives_the_same_answers():
    """the low bits of the framebuffer word hold what the textured resolve needs: no reader may look at them"""
    key = "cliff-near360~"
    e = hzutil.zoo_tex_entry("cliff-near360")
    t, texels = hzutil.zoo_tex_inputs(e)
    c = Ctx(key)
    try:
        c.dev.set_texture(t, texels)
        c.dev.draw(c.view)
        c.check_readers("textured, after a draw", npix=200)
        for cw, ch, cut in ((1, 1, 0), (7, 31, 37)):
            c.check_link(cw, ch, cut, "textured")
        for k in range(2):                                  # render_to_host, then draw + resolve_to_host, textured
            got = c.dev.render(c.view)
            assert np.array_equal(got["z24"], ac.want_render(key)["z24"])
            assert not np.array_equal(got["bgr"], ac.want_render(key)["bgr"])       # (it IS textured)
            c.check_readers(f"textured, after conversion {k}")
        c.dev.texture_off()
        c.check_readers("texture switched off")
    finally:
        c.dev.close()


# ---- (b) call order -------------------------------------------------------------------------------------------------------

def _to_host(c, how):
    """hz_hip_render_to_host / hz_hip_draw + hz_hip_resolve_to_host of the whole image: dict(bgr, ranges, index, z24)"""
    lib, dev, W, H = c.dev.lib, c.dev.dev, c.W, c.H
    v, tanel = c.dev._view_tanel(c.view)
    out = {"bgr": np.empty((H, W, 3), np.uint8), "ranges": np.empty((H, W), np.float32),
           "index": np.empty((H, W), np.int32), "z24": np.empty((H, W), np.uint32)}
    ptrs = [out[k].ctypes.data for k in ("bgr", "ranges", "index", "z24")]
    if how == "render_to_host":
        rc = lib.hz_hip_render_to_host(dev, C.byref(v), tanel.ctypes.data, *ptrs)
    else:
        assert lib.hz_hip_draw(dev, C.byref(v)) == 0, c.dev.last_error()
        rc = lib.hz_hip_resolve_to_host(dev, C.byref(v), tanel.ctypes.data, *ptrs)
    assert rc == 0, c.dev.last_error()
    return out


def _same_render(got, want, what):
    hzutil.assert_same_render({k: np.nan_to_num(a, nan=-7.0) if k == "ranges" else a for k, a in got.items()},
                              {k: np.nan_to_num(a, nan=-7.0) if k == "ranges" else a for k, a in want.items()}, what)


@pytest.mark.parametrize("clears", [1, 0])
@pytest.mark.parametrize("key", ["cliff-near360", "cliff-near360~"])
def test_readers_after_every_kind_of_call(key, clears):
    """hz_fb_refill: a reader that finds the framebuffer consumed by the conversion before it (or replaced by the last
    sector of a delivery in sectors) repeats the draw; one that finds it whole must not.  After each call the three readers
    answer as after a plain draw, twice in a row, and the render after them is still the oracle's"""
    import torch
    c = Ctx(key)
    W, H = c.W, c.H
    want = ac.want_render(key)
    ms = (W + 31) // 32
    d_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    d_sparse = torch.zeros(1 + H + H * ms + H * W, dtype=torch.int32, device="cuda:0")
    lib, dev = c.dev.lib, c.dev.dev

    def pack():
        assert lib.hz_hip_pack(dev, d_packed.data_ptr()) == 0, c.dev.last_error()

    def pack_sparse():
        assert lib.hz_hip_pack_sparse(dev, d_sparse.data_ptr(), ms) == 0, c.dev.last_error()

    def sectors(n):
        c.dev.set_options(host_sectors=n)

    steps = [
        ("render_to_host", lambda: _same_render(_to_host(c, "render_to_host"), want, "render_to_host")),
        ("render_to_host in 3 sectors", lambda: (sectors(3), _same_render(_to_host(c, "render_to_host"), want, "3 sectors"), sectors(0))),
        ("draw + resolve_to_host", lambda: _same_render(_to_host(c, "draw_resolve"), want, "draw + resolve_to_host")),
        ("draw alone", lambda: c.dev.draw(c.view)),
        ("pack", lambda: (c.dev.draw(c.view), pack())),
        ("pack twice", lambda: (pack(), pack())),
        ("pack_sparse", lambda: (c.dev.draw(c.view), pack_sparse())),
        ("pack_sparse after the readers alone", pack_sparse),
        ("3 sectors, then pack", lambda: (sectors(3), _to_host(c, "render_to_host"), sectors(0), pack())),
    ]
    try:
        c.dev.set_options(resolve_clears=clears)
        for what, step in steps:
            step()
            c.check_readers(f"after {what} (resolve_clears={clears})")
            c.check_readers(f"after {what} and the readers (resolve_clears={clears})", npix=8)
            c.check_link(1, 1, 0, what)
            _same_render(_to_host(c, "render_to_host"), want, f"the render after the readers after {what}")
        # the strips a reader's refill leaves behind are the draw's
        c.dev.draw(c.view); pack(); c.check_depth(ac.depth_pixels(key, n=8)); pack()
        torch.cuda.synchronize()
        words = d_packed.cpu().numpy().view(np.uint32)
        terrain = want["z24"] != 0xFFFFFF
        assert np.array_equal(words >> 8, want["z24"]) and np.array_equal((words & 0xFF)[terrain], want["bgr"][..., 2][terrain])
    finally:
        c.dev.close()


def test_context_that_has_drawn_nothing_answers_all_sky():
    """no draw yet: the framebuffer is as hz_hip_create cleared it and nothing is marked consumed, so the readers read it -
    every cell NaN, nothing visible, depth 0xFFFFFF.  Never data"""
    key = "cliff-near360~"
    c = Ctx(key)
    try:
        assert c.dev.lib.hz_hip_sync(c.dev.dev) == 0
        rc, la, lo = c.link(14, 14, 0)
        assert rc == 0 and np.isnan(la).all() and np.isnan(lo).all()
        rc, vis, x, y = c.dev.poi(c.view, ac.proj_list(key), 0)
        assert rc == 0 and not vis.any() and not x.any() and not y.any()
        for px in ac.depth_pixels(key, n=12):
            assert c.dev.read_depth(*px) == (0, 0xFFFFFF)
        # ... and the first draw after them is the oracle's
        _same_render(_to_host(c, "render_to_host"), ac.want_render(key), "first render of a context whose readers ran first")
        c.check_readers("after that render")
    finally:
        c.dev.close()


# ---- (c) the host halves, through the Python API --------------------------------------------------------------------------

# 354..366 looks over the synthetic DEM's terrain into the sky (every cell NaN, nothing visible, no pick): 474..486 is as narrow
# and wrapped, and two thirds terrain
API_VIEWS = [(-179.9, 179.95, False), (354.0, 366.0, False), (474.0, 486.0, False), (0.0, 90.0, False), (-120.0, 75.0, True)]


@pytest.fixture(scope="module")
def api():
    import horizonator_amd
    R, W, H = 100, 640, 160
    lat, lon = hzutil.VIEW_LAT, hzutil.VIEW_LON
    d = hzutil.dem_dir_for(lat, lon, R)
    h = horizonator_amd.horizonator(lat, lon, W, H, dir_dems=d, render_radius_cells=R)
    m = oracle.Dem(lat, lon, d, radius_cells=R).mosaic()
    yield h, m, W, H
    h.close()


@pytest.mark.parametrize("az0,az1,centers", API_VIEWS, ids=lambda v: str(v))
def test_host_halves_against_the_naive_restatement(api, az0, az1, centers):
    """horizonator_amd_link_cells' tables, horizonator_amd_poi_visibility's projections and horizonator_pick's arithmetic
    (hz_host.c) against naive_annot on the oracle's render of the uniforms the context reports"""
    h, m, W, H = api
    lat32, lon32 = float(np.float32(hzutil.VIEW_LAT)), float(np.float32(hzutil.VIEW_LON))
    _, ranges = h.render(az0, az1, az_extents_use_pixel_centers=centers, zfar=30000.0)
    v = h.view()
    want = oracle.render(m, oracle.make_view(**v), W, H)
    all_sky = (az0, az1) == (354.0, 366.0)
    assert np.array_equal(ranges, want["ranges"]) and (not (want["ranges"] > 0).any() if all_sky else 0.05 < (want["ranges"] > 0).mean() < 0.95)
    a0, a1, R = float(v["az_deg0"]), float(v["az_deg1"]), want["ranges"]
    if centers:
        assert (a0, a1) != (az0, az1)

    for cw, ch, cut in ((14, 14, 0), (14, 14, 37), (1, 1, 0), (7, 31, 5), (W - 1, H - 1, 0)):
        la, lo = h.link_cells(cw, ch, cut)
        wla, wlo = na.link_cells(R, cut, cw, ch, lat32, lon32, a0, a1)
        assert la.shape == wla.shape and la.size > 0
        assert np.array_equal(la, wla, equal_nan=True) and np.array_equal(lo, wlo, equal_nan=True), (cw, ch, cut)
    # no cell column, no cell row: empty results, no error (hz_host.c: horizonator_amd_link_cells)
    for cw, ch, cut, shape in ((W, 14, 0, (len(range(0, H - 14, 14)), 0)), (W + 7, 14, 0, (len(range(0, H - 14, 14)), 0)),
                               (14, 14, H, (0, len(range(0, W - 14, 14)))), (14, 14, H + 9, (0, len(range(0, W - 14, 14)))),
                               (14, H, 0, (0, len(range(0, W - 14, 14))))):
        la, lo = h.link_cells(cw, ch, cut)
        assert la.shape == lo.shape == shape, (cw, ch, cut, la.shape)

    N = m.shape[0]
    rng = np.random.default_rng(3)
    jj, ii = np.meshgrid(np.arange(2, N - 2, 3), np.arange(2, N - 2, 3), indexing="ij")
    glat = hzutil.VIEW_LAT + (jj - v["viewer_cell_j"]) / 1200.0
    glon = hzutil.VIEW_LON + (ii - v["viewer_cell_i"]) / 1200.0
    gele = m[jj, ii].astype(np.float64)
    pois = np.concatenate([np.stack([glat.ravel(), glon.ravel(), gele.ravel() + dz], 1) for dz in (0.0, -400.0, 2000.0)] +
                          [np.stack([hzutil.VIEW_LAT + rng.uniform(-0.1, 0.1, 300), hzutil.VIEW_LON + rng.uniform(-0.1, 0.1, 300),
                                     rng.uniform(0, 3000, 300)], 1)]).astype(np.float32)
    for cut in (0, 20, H - 3, H + 5, -4):
        vis, x, y = h.poi_visibility(pois, cut_off_bottom_px=cut)
        wvis, wx, wy = na.poi_visibility(R, pois, cut, lat32, lon32, a0, a1, float(v["viewer_z"]))
        assert np.array_equal(vis, wvis) and np.array_equal(x, wx) and np.array_equal(y, wy), cut
        if cut == 0 and not all_sky:
            assert 10 < wvis.sum() < len(pois) - 10
    assert h.poi_visibility(np.zeros((0, 3), np.float32))[0].shape == (0,)

    z = want["z24"]
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(96)]
    sky = 0
    for x, y in px:
        got, w = h.pick(x, y), na.pick(z, x, y, v, lat32, lon32)
        if w is None:
            assert got is None, (x, y, got)
            sky += 1
        else:
            assert got is not None and (np.float32(got[0]), np.float32(got[1])) == w, (x, y, got, w)
    assert sky == 100 if all_sky else 5 < sky < 95
    for x, y in ((-1, 0), (W, 0), (0, -1), (0, H)):
        assert h.pick(x, y) is None
