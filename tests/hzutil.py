"""shared helpers for the tests: synthetic DEM tiles, views, comparisons"""
import os
import tempfile

import numpy as np

from horizonator_amd import _lib as hzlib

# the survey's generic viewpoint: not on a grid sample
VIEW_LAT, VIEW_LON = 34.4137, -117.5621

_DEM_ROOT = os.environ.get("HZ_TEST_DEM_DIR", os.path.join(tempfile.gettempdir(), "hz_synth_dems"))


def dem_dir(lat_lo, lat_hi, lon_lo, lon_hi, srtm1=False, rough=False):
    """directory holding synthetic tiles covering the given integer lat/lon box
    (tiles are generated on first use and cached across test runs)"""
    name = ("srtm1" if srtm1 else "srtm3") + ("_rough" if rough else "")
    d = os.path.join(_DEM_ROOT, name)
    os.makedirs(d, exist_ok=True)
    gen = hzlib.load_demgen()
    rc = gen.hz_demgen_write_region(d.encode(), lat_lo, lat_hi, lon_lo, lon_hi, int(srtm1), int(rough))
    if rc < 0:
        raise RuntimeError(f"demgen failed ({rc})")
    return d


def load_render_fixture(path):
    """tests/golden/render_*.npz as a dict.  A fixture whose DEM window is too large to commit along with it
    (render_G3_cfg1: 1200x1200 samples) holds the SHA-256 of that int16 mosaic and its radius instead; the mosaic is
    then rebuilt from the synthetic tiles it was cut from (oracle/make_golden.py: render_fixture) and must hash the same"""
    import hashlib
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    if "mosaic" not in g:
        import oracle
        R = int(g["mosaic_R"])
        m = oracle.Dem(VIEW_LAT, VIEW_LON, dem_dir_for(VIEW_LAT, VIEW_LON, R), radius_cells=R).mosaic()
        if hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() != str(g["mosaic_sha256"]):
            raise AssertionError(f"{os.path.basename(path)}: the synthetic DEM generator produced different tiles on this "
                                 "machine (libm?): the fixture's mosaic cannot be rebuilt")
        g["mosaic"] = m
    return g


def tiles_for(lat, lon, radius_cells, srtm1=False):
    """integer lat/lon box a window of radius_cells around (lat,lon) can touch"""
    cpd = 3600 if srtm1 else 1200
    r = radius_cells / cpd + 0.01
    return (int(np.floor(lat - r)), int(np.floor(lat + r)),
            int(np.floor(lon - r)), int(np.floor(lon + r)))


def dem_dir_for(lat, lon, radius_cells, srtm1=False, rough=False):
    return dem_dir(*tiles_for(lat, lon, radius_cells, srtm1), srtm1=srtm1, rough=rough)


def viewpoint_lattice(lat=VIEW_LAT, lon=VIEW_LON, side=16, half_span_deg=0.2):
    """the batch of side*side viewpoints of BASELINE.json configs[3],
    a lattice of +-half_span_deg around (lat,lon); viewpoint v = row*side + column,
    rows south to north, columns west to east; float32 as the API takes them"""
    off = (np.arange(side, dtype=np.float64) / (side - 1) - 0.5) * 2.0 * half_span_deg
    lats = np.repeat(lat + off, side).astype(np.float32)
    lons = np.tile(lon + off, side).astype(np.float32)
    return lats, lons


def random_view_case(seed):
    """seeded random render configuration shared by the parity tests and by oracle/make_golden.py
    (tests/golden/random_checksums.json holds what the reference's shaders drew for each):
    viewpoint, azimuth extents (narrow, wide, wrapped, exactly 360), image size, depth/colour
    extents, viewer height, sector"""
    rng = np.random.default_rng(1000 + seed)
    c = {}
    c["R"] = int(rng.choice([24, 40, 75, 130, 200]))
    c["W"] = int(rng.integers(17, 900))
    c["H"] = int(rng.integers(9, 400))
    c["rough"] = bool(seed % 3 == 0)
    span = float(rng.choice([360.0, rng.uniform(0.5, 20.0), rng.uniform(20.0, 359.0)]))
    c["az0"] = float(rng.uniform(-720.0, 720.0))
    c["az1"] = c["az0"] + span
    frac = c["R"] / 1200.0 * 0.8
    c["lat"] = VIEW_LAT + float(rng.uniform(-frac, frac))
    c["lon"] = VIEW_LON + float(rng.uniform(-frac, frac))
    zfar = float(rng.choice([2000.0, 9000.0, 40000.0, 300000.0]))
    znear = float(rng.choice([100.0, 1.0, 500.0]))
    kw = dict(znear=znear, zfar=zfar)
    if seed % 4 == 1:
        kw.update(znear_color=float(rng.uniform(10.0, 3000.0)), zfar_color=float(rng.uniform(3500.0, 30000.0)))
    if seed % 5 == 2:
        kw.update(viewer_z=float(rng.uniform(0.0, 9000.0)))
    c["kw"] = kw
    c["c0"] = int(rng.integers(0, c["W"] - 1)) if seed % 2 else 0
    c["c1"] = int(rng.integers(c["c0"] + 1, c["W"] + 1)) if seed % 2 else c["W"]
    return c


def hash_texture(th, tw, seed=0, blocky=1):
    """a deterministic map-like texture without any RNG (integer hash of the texel index, so that
    fixtures only need to store its size and seed): uint8[th,tw,3], B,G,R, row 0 = southern edge.
    blocky > 1 repeats each value over blocky x blocky texels (flat areas with sharp borders)."""
    y, x = np.mgrid[0:th, 0:tw].astype(np.uint64)
    y //= np.uint64(blocky); x //= np.uint64(blocky)
    out = np.empty((th, tw, 3), np.uint8)
    for c in range(3):
        h = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ np.uint64((c + 1) * 83492791 + seed * 2654435761)
        h = (h ^ (h >> np.uint64(13))) * np.uint64(0x9E3779B97F4A7C15)
        out[..., c] = ((h >> np.uint64(40)) & np.uint64(255)).astype(np.uint8)
    return out


def write_map_tiles(root, name, lowest_x, lowest_y, nx, ny, seed):
    """zoom-12 map tiles as PNG files in the layout the reference reads
    (dir_tiles/tiles_name/12/X/Y.png), in the PNG flavours tile servers emit; returns the
    mosaic as the reference builds it: uint8[ny*256, nx*256, 3] B,G,R, southern row first"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    mosaic = np.zeros((ny * 256, nx * 256, 3), np.uint8)
    highest_y = lowest_y + ny - 1
    k = 0
    for ty in range(lowest_y, lowest_y + ny):
        for tx in range(lowest_x, lowest_x + nx):
            yy, xx = np.mgrid[0:256, 0:256]
            rgb = np.stack([(xx * 3 + tx * 40) % 256, (yy * 5 + ty * 17) % 256, (xx + yy + 31 * k) % 256], -1).astype(np.uint8)
            rgb = (rgb.astype(int) + rng.integers(-20, 21, rgb.shape)).clip(0, 255).astype(np.uint8)
            img = Image.fromarray(rgb, "RGB")
            flavour = k % 4
            if flavour == 1:            # palettised, as OSM's own tiles are (reference :339-352)
                img = img.quantize(colors=200)
                rgb = np.asarray(img.convert("RGB"))
            elif flavour == 2:          # with an alpha channel, which is dropped
                img = img.convert("RGBA")
            elif flavour == 3:          # grey
                img = img.convert("L")
                rgb = np.repeat(np.asarray(img)[..., None], 3, -1)
            d = root / name / "12" / str(tx)
            d.mkdir(parents=True, exist_ok=True)
            img.save(d / f"{ty}.png")
            x0, y0 = (tx - lowest_x) * 256, (highest_y - ty) * 256
            mosaic[y0:y0 + 256, x0:x0 + 256] = rgb[::-1, :, ::-1]      # bottom-up rows, B,G,R
            k += 1
    return mosaic


# ---- driving the HIP path through its C-ABI (include/hz_hip.h) ---------------

def hip_available():
    try:
        return hzlib.load().hz_hip_device_count() > 0
    except Exception:
        return False


class HipDev:
    """one device context of the C-ABI shim (include/hz_hip.h), reusable for several draws:
    hz_hip_create / upload_mosaic, then render(view, col0, col1) = set_sector / render_to_host
    (or draw / resolve_to_host) as often as wanted"""

    def __init__(self, mosaic, W, H, raster=0):
        self.lib = hzlib.load()
        mosaic = np.ascontiguousarray(mosaic, np.int16)
        self.W, self.H = W, H
        self.dev = self.lib.hz_hip_create(0, mosaic.shape[0], W, H)
        if not self.dev:
            raise RuntimeError("hz_hip_create failed: " + self.lib.hz_hip_last_error().decode())
        try:
            assert self.lib.hz_hip_upload_mosaic(self.dev, mosaic.ctypes.data) == 0
            assert self.lib.hz_hip_set_raster(self.dev, raster) == 0
        except Exception:
            self.close()
            raise

    def close(self):
        if self.dev:
            self.lib.hz_hip_destroy(self.dev)
            self.dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_texture(self, tex, texels):
        """texture path: `tex` is anything with the hz_texparams_t field names (e.g. oracle.OrcTex)"""
        import ctypes as C
        tp = hzlib.TexParams()
        for name, _ in hzlib.TexParams._fields_:
            setattr(tp, name, getattr(tex, name))
        texels = np.ascontiguousarray(texels, np.uint8)
        assert texels.shape == (tp.tex_h, tp.tex_w, 3)
        assert self.lib.hz_hip_set_texture(self.dev, C.byref(tp), texels.ctypes.data) == 0, self.lib.hz_hip_last_error()

    def texture_off(self):
        assert self.lib.hz_hip_set_texture(self.dev, None, None) == 0

    def set_texparams(self, tex):
        """the parameters alone, for a resident texture of the same size: the C-ABI's return code (0, or -1 with
        hz_hip_last_error() set)"""
        import ctypes as C
        tp = hzlib.TexParams()
        for name, _ in hzlib.TexParams._fields_:
            setattr(tp, name, getattr(tex, name))
        return self.lib.hz_hip_set_texture(self.dev, C.byref(tp), None)

    # ---- the draw and the readers of its framebuffer on their own: thin wrappers, return codes handed back -------------

    def _view_tanel(self, view):
        import oracle
        v = hzlib.View()
        for name, _ in hzlib.View._fields_:
            setattr(v, name, getattr(view, name))
        return v, np.ascontiguousarray(oracle.tanel(self.W, self.H, v.az_deg0, v.az_deg1), np.float32)

    def last_error(self):
        return self.lib.hz_hip_last_error().decode()

    def set_options(self, **kw):
        """hz_hip_set_options with some fields replaced, e.g. set_options(host_sectors=3, resolve_clears=0)"""
        import ctypes as C
        o = hzlib.Options()
        assert self.lib.hz_hip_get_options(self.dev, C.byref(o)) == 0
        for k, x in kw.items():
            assert k in dict(hzlib.Options._fields_), k
            setattr(o, k, int(x))
        assert self.lib.hz_hip_set_options(self.dev, C.byref(o)) == 0, self.last_error()

    def draw(self, view, col0=0, col1=None):
        """hz_hip_set_sector + hz_hip_draw: the framebuffer the readers below read"""
        import ctypes as C
        assert self.lib.hz_hip_set_sector(self.dev, col0, self.W if col1 is None else col1) == 0, self.last_error()
        v, _ = self._view_tanel(view)
        assert self.lib.hz_hip_draw(self.dev, C.byref(v)) == 0, self.last_error()

    def link_cells(self, view, sin_az, cos_az, cos_el, viewer_lat, cos_viewer_lat, viewer_lon, cell_w, cell_h, nx, ny, fill=12345.0):
        """hz_hip_link_cells: (return code, lat, lon); the outputs are float32[max(ny,0), max(nx,0)] (one element where that
        is empty) prefilled with `fill`, so that a refused call shows that it wrote nothing.  A table may be None"""
        import ctypes as C
        v, tanel = self._view_tanel(view)
        shape = (ny, nx) if nx > 0 and ny > 0 else (1, 1)
        lat, lon = np.full(shape, fill, np.float32), np.full(shape, fill, np.float32)
        tabs = [None if t is None else np.ascontiguousarray(t, dt) for t, dt in ((sin_az, np.float32), (cos_az, np.float32), (cos_el, np.float64))]
        rc = self.lib.hz_hip_link_cells(self.dev, C.byref(v), tanel.ctypes.data, *[None if t is None else t.ctypes.data for t in tabs],
                                        viewer_lat, cos_viewer_lat, viewer_lon, cell_w, cell_h, nx, ny, lat.ctypes.data, lon.ctypes.data)
        return rc, lat, lon

    def poi(self, view, proj, cut_off_bottom_px, fill=77):
        """hz_hip_poi_visibility on projected points float64[n,3] (x, y, range): (return code, visible, label_x, label_y),
        the outputs prefilled with `fill`"""
        import ctypes as C
        v, tanel = self._view_tanel(view)
        proj = np.ascontiguousarray(proj, np.float64).reshape(-1, 3)
        n = len(proj)
        vis, x, y = np.full(max(n, 1), fill, np.uint8), np.full(max(n, 1), fill, np.float32), np.full(max(n, 1), fill, np.float32)
        rc = self.lib.hz_hip_poi_visibility(self.dev, C.byref(v), tanel.ctypes.data, cut_off_bottom_px, proj.ctypes.data, n,
                                            vis.ctypes.data, x.ctypes.data, y.ctypes.data)
        return rc, vis[:n], x[:n], y[:n]

    def read_depth(self, x, y):
        """hz_hip_read_depth: (return code, z24)"""
        import ctypes as C
        z = C.c_uint32(0xDEADBEEF)
        rc = self.lib.hz_hip_read_depth(self.dev, int(x), int(y), C.byref(z))
        return rc, z.value

    def render(self, view, col0=0, col1=None, tanel=None, want=("bgr", "ranges", "index", "z24")):
        """`view` is anything with the hz_view_t field names as attributes (e.g. oracle.OrcView);
        `want`: the outputs asked for (NULL goes in for the others), returned as a dict of those"""
        import ctypes as C
        lib, W, H = self.lib, self.W, self.H
        if col1 is None:
            col1 = W
        SW = col1 - col0
        assert lib.hz_hip_set_sector(self.dev, col0, col1) == 0
        v = hzlib.View()
        for name, _ in hzlib.View._fields_:
            setattr(v, name, getattr(view, name))
        if tanel is None:
            # tan(elevation) per GL row exactly as hz_host.c / the reference derive it
            import oracle
            tanel = oracle.tanel(W, H, v.az_deg0, v.az_deg1)
        tanel = np.ascontiguousarray(tanel, np.float32)
        assert want and set(want) <= {"bgr", "ranges", "index", "z24"}
        out = {"bgr": np.empty((H, SW, 3), np.uint8), "ranges": np.empty((H, SW), np.float32),
               "index": np.empty((H, SW), np.int32), "z24": np.empty((H, SW), np.uint32)}
        out = {k: a for k, a in out.items() if k in want}

        def ptr(k):
            return out[k].ctypes.data if k in out else None
        # draw + delivery into host memory as one call (hz_hostpath.cpp: in azimuth sectors where the image is large or the
        # context's host_sectors option says so); every other call the two-step form, hz_hip_draw then hz_hip_resolve_to_host
        self.calls = getattr(self, "calls", 0) + 1
        if self.calls % 2:
            rc = lib.hz_hip_render_to_host(self.dev, C.byref(v), tanel.ctypes.data, ptr("bgr"), ptr("ranges"), ptr("index"), ptr("z24"))
        else:
            assert lib.hz_hip_draw(self.dev, C.byref(v)) == 0, lib.hz_hip_last_error()
            rc = lib.hz_hip_resolve_to_host(self.dev, C.byref(v), tanel.ctypes.data, ptr("bgr"), ptr("ranges"), ptr("index"), ptr("z24"))
        assert rc == 0, lib.hz_hip_last_error()
        return out


def hip_render(mosaic, view, W, H, col0=0, col1=None, raster=0, tanel=None, tex=None, texels=None):
    """mosaic int16[N,N] + uniform values -> dict(bgr, ranges, index, z24) via
    hz_hip_create / upload_mosaic / draw / resolve_to_host on a fresh context"""
    with HipDev(mosaic, W, H, raster=raster) as dev:
        if tex is not None:
            dev.set_texture(tex, texels)
        return dev.render(view, col0, col1, tanel=tanel)


def assert_same_render(a, b, what=""):
    for k in ("index", "z24", "bgr", "ranges"):
        if k in a and k in b:
            if not np.array_equal(a[k], b[k]):
                bad = np.argwhere(a[k] != b[k])
                raise AssertionError(f"{what}: {k} differs at {len(bad)} places, first {bad[0]}: "
                                     f"{a[k][tuple(bad[0])]} vs {b[k][tuple(bad[0])]}")


def same_render(a, b, what=""):
    """assert_same_render, with ranges that are NaN in the same places counted as equal: without a far clip
    (zfar = inf) the reference's own range formula gives 0 * inf on terrain"""
    if "ranges" in a and "ranges" in b:
        assert np.array_equal(np.isnan(a["ranges"]), np.isnan(b["ranges"])), f"{what}: ranges are NaN in different places"
    assert_same_render({k: np.nan_to_num(x, nan=-7.0) if k == "ranges" else x for k, x in a.items()},
                       {k: np.nan_to_num(x, nan=-7.0) if k == "ranges" else x for k, x in b.items()}, what)


# ---- the terrain zoo: hand-made ground, integer arithmetic only --------------

def _zoo_hash(i, j, seed):
    """64-bit integer hash of a sample position (the hash_texture mix): uint64, same bytes on every machine"""
    i = np.asarray(i).astype(np.uint64); j = np.asarray(j).astype(np.uint64)
    h = (i * np.uint64(73856093)) ^ (j * np.uint64(19349663)) ^ np.uint64(83492791 + seed * 2654435761)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(0x9E3779B97F4A7C15)
    return (h ^ (h >> np.uint64(29))) >> np.uint64(20)


def _isqrt(a):
    """floor(sqrt(a)) of a non-negative int64 array, corrected with integer compares"""
    r = np.sqrt(a.astype(np.float64)).astype(np.int64)
    r -= (r * r > a)
    r += ((r + 1) * (r + 1) <= a)
    return r


ZOO_FAMILIES = ("flat0", "plateau", "checker", "spikes", "cliff", "coast", "max16", "border_minus1", "bowl", "stairs")


def zoo_mosaic(name, N):
    """hand-made DEM windows for tests/test_gpu_terrain_zoo.py: int16[N,N], row j = north index, column i = east index.
    No libm, no RNG: fixtures store the name and N, not the samples."""
    j, i = np.mgrid[0:N, 0:N].astype(np.int64)
    if name == "flat0":                 # sea level everywhere: what the DEM reader gives for voids and missing tiles
        m = np.zeros((N, N), np.int64)
    elif name == "plateau":
        m = np.full((N, N), 1234, np.int64)
    elif name == "checker":             # every triangle tall and thin
        m = np.where((i + j) & 1, 8000, 0)
    elif name == "spikes":              # isolated one-sample summits
        m = np.where(_zoo_hash(i, j, 1) % np.uint64(97) == 0, 6000, 200)
    elif name == "cliff":               # one wall along a meridian three cells east of the centre
        m = np.where(i < N // 2 + 3, 0, 3000)
    elif name == "coast":               # half sea level, half blocky land
        m = np.maximum(0, (_zoo_hash(i // 8, j // 8, 2) % np.uint64(900)).astype(np.int64) - 450)
    elif name == "max16":               # top bits of the int16
        m = np.where(_zoo_hash(i, j, 3) & np.uint64(1), 32767, 32000)
    elif name == "border_minus1":       # the -1 that sampling outside the window returns, next to positive heights
        m = np.full((N, N), 500, np.int64)
        m[:2, :] = -1; m[-1, :] = -1; m[:, 0] = -1; m[:, -2:] = -1
    elif name == "bowl":                # viewer at the bottom: everything above the horizon, nothing hidden
        c = N // 2
        m = np.minimum(8000, 60 * _isqrt((i - c) ** 2 + (j - c) ** 2))
    elif name == "stairs":              # long exactly collinear edges on a slope
        m = 100 * (j // 16)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(m.astype(np.int16))


# cos(latitude) as float32 constants, so that no case depends on a libm: latitude -> cos_viewer_lat
_ZOO_COS = {0.0: 1.0, 34.4: 0.8251135, -43.6: 0.7241719, 69.6: 0.3485720, 80.0: 0.1736482}

# view recipes: N, W, H, viewer position ("off" = a fraction of a cell off the centre, "vertex" = exactly on the centre
# sample, "corner" = a few cells from the window's south-west corner), viewer height (a number, or "above" = 10 m above the
# highest of the four samples around the viewer), latitude, cells per degree, azimuth extents, depth extents, colour extents
_ZOO_VIEWS = {
    "near360":   dict(N=64,  W=640,  H=160, pos="off",    vz="above", lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(100.0, 40000.0)),
    "high_wrap": dict(N=200, W=640,  H=160, pos="off",    vz=2500.0,  lat=-43.6, cpd=1200, az=(170.0, 530.0),  z=(10.0, 300000.0)),
    "arctic90":  dict(N=128, W=801,  H=203, pos="off",    vz="above", lat=69.6,  cpd=3600, az=(-45.0, 45.0),   z=(1.0, 2000.0)),
    "sky":       dict(N=400, W=1024, H=256, pos="off",    vz=9000.0,  lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(100.0, 100000.0),
                      zc=(2000.0, 30000.0)),
    "zoom12":    dict(N=96,  W=333,  H=111, pos="vertex", vz="above", lat=80.0,  cpd=1200, az=(354.0, 366.0),   z=(10.0, 20000.0)),
    "corner90":  dict(N=400, W=1024, H=256, pos="corner", vz=2500.0,  lat=0.0,   cpd=1200, az=(0.0, 90.0),     z=(100.0, 300000.0)),
    "z005":      dict(N=64,  W=512,  H=128, pos="off",    vz=0.005,   lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(1.0, 9000.0)),
    # depth steps of 30 m: overlapping triangles tie in z24 and the lower triangle id must win
    "coarse_z":  dict(N=64,  W=640,  H=160, pos="off",    vz="above", lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(100.0, 5e8),
                      zc=(100.0, 40000.0)),
    # "no far limit" as a caller may write it: every quotient by the colour span is exactly 0
    "inf_color": dict(N=64,  W=640,  H=160, pos="off",    vz="above", lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(100.0, 40000.0),
                      zc=(100.0, float("inf"))),
    # ... and no far clip: every vertex has depth exactly -1, all of the terrain ties at z24 = 0 and the lowest triangle id wins
    # everywhere; the abridged quotient by the depth span would be NaN (hzf_draw_ok refuses the draw).  The reference's own
    # range formula gives 0 * inf = NaN on terrain here
    "inf_far":   dict(N=64,  W=640,  H=160, pos="off",    vz="above", lat=34.4,  cpd=1200, az=(-180.0, 180.0), z=(100.0, float("inf")),
                      zc=(100.0, 40000.0)),
    "vertex360": dict(N=64,  W=512,  H=128, pos="vertex", vz="above", lat=-43.6, cpd=3600, az=(-180.0, 180.0), z=(10.0, 8000.0),
                      zc=(50.0, 1500.0)),
}

# family -> (recipe, overrides) ...: the cross of ground and view, written out so that a reader sees every case
_ZOO_PLAN = {
    "flat0":         [("near360", {}), ("high_wrap", {}), ("sky", {}), ("zoom12", {}), ("corner90", {}),
                      ("z005", dict(degenerate=True))],                                        # 5 mm above sea level: a line
    "plateau":       [("near360", dict(vz=1300.0)), ("high_wrap", {}), ("arctic90", {}), ("sky", {}),
                      ("vertex360", dict(vz=1234.0, degenerate=True))],                       # edge-on: viewer AT the plateau's height
    "checker":       [("near360", {}), ("high_wrap", dict(vz=8500.0)), ("arctic90", {}), ("sky", {}), ("vertex360", dict(vz=4000.0)),
                      ("coarse_z", {}), ("zoom12", dict(vz=4000.0, degenerate=True))],                           # from inside the checkerboard: all terrain
    "spikes":        [("near360", {}), ("high_wrap", {}), ("arctic90", {}), ("corner90", {}), ("vertex360", dict(vz=100.0)), ("zoom12", {}),
                      ("coarse_z", {}), ("inf_color", {}), ("inf_far", {})],
    "cliff":         [("near360", {}), ("high_wrap", {}), ("arctic90", {}), ("z005", {}), ("sky", {}), ("inf_color", {})],
    "coast":         [("near360", {}), ("high_wrap", {}), ("arctic90", {}), ("sky", {}), ("corner90", {}), ("zoom12", {}), ("coarse_z", {}),
                      ("inf_far", {})],
    "max16":         [("near360", {}), ("arctic90", {}), ("vertex360", {}), ("sky", dict(vz=34000.0))],
    "border_minus1": [("near360", {}), ("high_wrap", {}), ("corner90", dict(vz=700.0)), ("sky", {}), ("vertex360", {})],
    "bowl":          [("near360", {}), ("high_wrap", {}), ("z005", {}), ("arctic90", {}), ("vertex360", {})],
    "stairs":        [("near360", {}), ("high_wrap", {}), ("corner90", {}), ("vertex360", dict(vz=150.0)), ("zoom12", {})],
}


def zoo_view_json(view):
    """a case's uniform values as strict JSON takes them: finite floats as they are, an infinite extent as the string "inf"""
    return {k: (x if np.isfinite(x) else {float("inf"): "inf", float("-inf"): "-inf"}[x]) for k, x in view.items()}


def zoo_cases():
    """the terrain zoo's case list, deterministic: dicts with name, family, N, W, H, view (the twelve uniform values as
    float32-representable floats), c0, c1 (a sector on every other case) and degenerate (the reference draws nothing or
    everything: wanted, but exempt from the terrain-fraction condition)"""
    f32 = np.float32
    cases = []
    for family in ZOO_FAMILIES:
        for recipe, over in _ZOO_PLAN[family]:
            r = dict(_ZOO_VIEWS[recipe]); r.update(over)
            N, W, H = r["N"], r["W"], r["H"]
            k = len(cases)
            if r["pos"] == "off":
                ci, cj = f32(N // 2) + f32(0.37), f32(N // 2) - f32(0.29)
            elif r["pos"] == "vertex":
                ci, cj = f32(N // 2), f32(N // 2)
            else:
                ci, cj = f32(5.3), f32(7.6)
            vz = r["vz"]
            if vz == "above":
                m = zoo_mosaic(family, N)
                i0, j0 = int(np.floor(ci)), int(np.floor(cj))
                vz = float(m[j0:j0 + 2, i0:i0 + 2].max()) + 10.0
            zc = r.get("zc", r["z"])
            view = dict(viewer_cell_i=ci, viewer_cell_j=cj, viewer_z=f32(vz), cos_viewer_lat=f32(_ZOO_COS[r["lat"]]),
                        deg_per_cell=f32(1.0) / f32(r["cpd"]), az_deg0=f32(r["az"][0]), az_deg1=f32(r["az"][1]),
                        aspect=f32(W) / f32(H), znear=f32(r["z"][0]), zfar=f32(r["z"][1]),
                        znear_color=f32(zc[0]), zfar_color=f32(zc[1]))
            c0, c1 = (W // 5 + k, W // 5 + k + W // 3) if k % 2 else (0, W)
            cases.append(dict(name=f"{family}-{recipe}", family=family, recipe=recipe, lat=r["lat"], N=N, W=W, H=H,
                              view={n: float(x) for n, x in view.items()}, c0=c0, c1=c1,
                              degenerate=bool(r.get("degenerate", False))))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# ---- image shapes at the kernels' size boundaries: zoo grounds and views at other W x H --------------------

# tiny images: narrower than the short cull's 64 columns, than one `touched` segment (256), than a tile of the coarse depth
# (8 x 4, 32 x 16) or of the tile bins (64 x 64), lower than the host path's four bands of rows, narrower than its eight sectors
SHAPES_TINY = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (4, 4), (5, 3), (15, 4), (16, 9), (63, 17), (64, 16), (65, 33),
               (255, 3), (256, 4), (257, 5), (9, 300), (3, 2000), (16384, 4), (4, 16384))
SHAPES_TINY_GROUNDS = ("coast-near360", "checker-near360", "spikes-zoom12", "cliff-arctic90")
# ... the boundaries that list misses: one row of a whole segment, the coarse-depth tiles (32 x 16) from both sides, the
# tile bins (64 x 64), two segments in fewer rows than bands, a host blob's 2048 columns from both sides
SHAPES_EDGE = ((64, 1), (31, 15), (32, 16), (33, 17), (65, 65), (512, 2), (2047, 5), (2048, 5), (2049, 5))
# wide images: the packed 16-bit pixel boxes of the short cull end at 65535 columns, hz_hip_pack_sparse at 65536
SHAPES_WIDE = ((65535, 8), (65536, 8), (65537, 9), (70001, 7))
SHAPES_WIDE_GROUNDS = ("coast-near360", "spikes-near360", "cliff-near360", "bowl-near360", "stairs-near360", "checker-vertex360",
                       "spikes-high_wrap")
# tall images: a blob's 16-bit row field ends at 65535 rows; the terrain lies around row H/2: 32768 at H = 65536, the sign
# bit of a 16-bit row, and beyond 65535 itself at H = 140001.  The azimuth extents are replaced: in a span as narrow as the
# aspect asks for every cell crosses a quarter of the image
SHAPES_TALL = ((8, 65536), (7, 70001), (33, 65535), (8, 140001))
SHAPES_TALL_GROUNDS = ("spikes-corner90", "coast-corner90", "stairs-corner90", "cliff-sky", "checker-sky", "spikes-high_wrap",
                       "bowl-high_wrap")
SHAPES_TALL_AZ = (10.0, 14.0)
# The short cull itself (mr_simple_cull: rows whose 64 vertices all lie inside the view volume) never runs on the shapes above:
# seven rows of a 70001-column panorama are 0.04 degrees of elevation, and four degrees of azimuth hold no whole strip.
# 4 Mpix images that give it rows to run on, on both sides of its limits.  Wide: a viewer two metres above level ground
# (the zoo case's viewer_z replaced), so that the ground beyond 650 m lies within the 0.35 degrees of 64 rows.  Tall: the
# zoo cases' own 360 degrees in 64 columns - every vertex is inside, the terrain lies in a few rows around row 32768
SHAPES_CULL_WIDE = ((65535, 64), (65536, 64), (65537, 63))
SHAPES_CULL_WIDE_GROUNDS = (("flat0-near360", 2.0), ("plateau-near360", 1236.0), ("stairs-near360", 202.0))
SHAPES_CULL_TALL = ((64, 65535), (64, 65536), (63, 66000))
SHAPES_CULL_TALL_GROUNDS = ("coast-near360", "spikes-near360", "bowl-near360")
SHAPE_LLVMPIPE_MAX = 16384              # llvmpipe draws no more pixels a side: larger shapes are held to the oracle alone


def _shape_sector(W, k):
    """the sector of the k-th case of a shape: in turn one column at column 0, the last column alone, a width that is no
    multiple of 4 from a start that is one, a start that is no multiple of 4; from 65537 columns on also six columns
    across column 65536 and the last three.  Images of fewer than four columns: the whole image"""
    if W < 4:
        return 0, W
    c_odd = min(W - 2, (W // 5) | 1)
    kinds = [(0, 1), (W - 1, W), (W // 3 // 4 * 4, W // 3 // 4 * 4 + max(1, min(W - W // 3 // 4 * 4, (W // 2) | 1))),
             (c_odd, min(W, c_odd + max(4, W // 2 // 4 * 4)))]
    if W >= 65537:
        kinds = [(65533, min(W, 65539)), (W - 3, W)] + kinds
    c0, c1 = kinds[k % len(kinds)]
    assert 0 <= c0 < c1 <= W
    return c0, c1


def shape_cases():
    """zoo grounds and views at image shapes next to the size rules of the kernels, deterministic: dicts with id, name (the
    zoo case's), family, N, W, H, view (the zoo case's with aspect = float32(W)/float32(H); for the tall shapes with the
    azimuth extents of SHAPES_TALL_AZ, for the wide shapes of the short cull with another viewer_z), az (those extents, or
    None), c0, c1 (a sector: _shape_sector) and kind"""
    f32 = np.float32
    zoo = {c["name"]: c for c in zoo_cases()}
    cases = []
    for kind, shapes, grounds, az in (("tiny", SHAPES_TINY, SHAPES_TINY_GROUNDS, None), ("edge", SHAPES_EDGE, SHAPES_TINY_GROUNDS, None),
                                      ("wide", SHAPES_WIDE, SHAPES_WIDE_GROUNDS, None), ("tall", SHAPES_TALL, SHAPES_TALL_GROUNDS, SHAPES_TALL_AZ),
                                      ("cull", SHAPES_CULL_WIDE, SHAPES_CULL_WIDE_GROUNDS, None),
                                      ("cull", SHAPES_CULL_TALL, SHAPES_CULL_TALL_GROUNDS, None)):
        for W, H in shapes:
            for k, ground in enumerate(grounds):
                name, vz = ground if isinstance(ground, tuple) else (ground, None)
                z = zoo[name]
                view = dict(z["view"])
                view["aspect"] = float(f32(W) / f32(H))
                if az is not None:
                    view["az_deg0"], view["az_deg1"] = float(f32(az[0])), float(f32(az[1]))
                if vz is not None:
                    view["viewer_z"] = float(f32(vz))
                c0, c1 = _shape_sector(W, k)
                cases.append(dict(id=f"{W}x{H}-{name}" + ("" if vz is None else "-vz%g" % vz), name=name, family=z["family"], N=z["N"],
                                  W=W, H=H, view=view, az=None if az is None else [float(az[0]), float(az[1])], c0=c0, c1=c1, kind=kind))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


# the textured resolve on five of the shapes: (shape case, texture seed); the texture is zoo_tex(case, "wrap", (3, 2))
# over hash_texture(512, 768, seed)
SHAPE_TEX_CASES = (("1x1-spikes-zoom12", 21), ("7x1-coast-near360", 22), ("255x3-coast-near360", 23), ("257x5-spikes-zoom12", 24),
                   ("70001x7-checker-vertex360", 25))


def shape_tex_inputs(case, seed):
    """(texture parameters, texels) of a textured shape case"""
    t = zoo_tex(case, "wrap", (3, 2))
    return t, hash_texture(t.tex_h, t.tex_w, seed=seed)


# ---- viewer positions at the grid's edges and odd DEM sizes: zoo grounds, zoo views with the viewer moved ----------------

EDGE_GROUNDS = ("coast", "spikes", "checker", "stairs", "border_minus1", "bowl")
EDGE_N, EDGE_W, EDGE_H = 128, 640, 160          # 127 cells: strips end at vertex columns 63 and 126, the last strip has one cell
MR_COLS = 63                                    # (hz_types.h: cells of a strip)
_P17, _P36, _P40 = 2.0 ** -17, 2.0 ** -36, 2.0 ** -40
# metres per cell as the transform forms it (hz_num.h: hz_north; hz_east times cos(latitude)): 20015088 / cells per degree / 180
EDGE_M_PER_CELL = {1200: 92.66244, 3600: 30.88748}
# (tag, i, j, kind, recipe, overrides of the recipe).  kind: "vertex" = a zero east or north offset at some vertex, "tiny" =
# an offset below hz_fast.h's HZF_LO = 2^-30 that is not zero, "in" = neither, "out" = the viewer outside the grid.
# 2^-40 cells are 92.66 * 2^-40 = 8.4e-11 m north (6.9e-11 m east at 34.4 degrees); 2^-36 cells of 1/3600 degree are
# 30.89 * 2^-36 = 4.5e-10 m north - with 1/1200 degree they would be 1.35e-9 m, above 2^-30 = 9.3e-10: that position is
# drawn with vertex360's cells.  tests/test_oracle_golden.py asserts the products
_EDGE_POSITIONS = (
    # on a strip boundary
    ("i63", 63.0, 40.37, "vertex", "near360", {}),
    ("i63-", 63.0 - _P17, 40.37, "in", "near360", {}),
    ("i63+", 63.0 + _P17, 40.37, "in", "near360", {}),
    ("i63_2500m", 63.0, 40.37, "vertex", "high_wrap", {}),
    ("i126_j126", 126.0, 126.0, "vertex", "near360", {}),
    ("i126_j0", 126.0, 0.0, "vertex", "near360", {}),          # row0[0..3] = 0: the viewer's row is a segment's first
    ("i126_j127", 126.0, 127.0, "vertex", "near360", {}),      # row0[4..7] = 127: ... its last
    ("i126_j4", 126.0, 4.0, "vertex", "near360", {}),          # row0[3] = 0, two rows a segment: last of [2,4], first of [4,6]
    ("i62.5_j63", 62.5, 63.0, "vertex", "near360", {}),        # n = 0 only
    # on the border, in the last and the first cell
    ("sw_corner", 0.0, 0.0, "vertex", "near360", {}),
    ("w_border", 0.0, 64.29, "vertex", "near360", {}),
    ("s_border", 64.37, 0.0, "vertex", "near360", {}),
    ("ne_corner", 127.0, 127.0, "vertex", "near360", {}),
    ("e_border", 127.0, 30.5, "vertex", "near360", {}),
    ("last_cell", 126.5, 126.5, "in", "near360", {}),
    ("first_cell", 0.5, 0.5, "in", "near360", {}),
    # tiny offsets
    ("tiny_ij", _P40, _P40, "tiny", "near360", {}),
    ("tiny_i", _P40, 64.29, "tiny", "near360", {}),
    ("tiny_j", 64.37, _P36, "tiny", "vertex360", {}),
    # just outside
    ("out_w", -0.5, 64.29, "out", "near360", {}),
    ("out_sw1", -1.0, -1.0, "out", "near360", {}),
    ("out_sw", -3.7, -2.2, "out", "near360", {}),
    ("out_sw_2500m", -3.7, -2.2, "out", "high_wrap", {}),
    ("out_e", 130.25, 64.6, "out", "near360", {}),
    ("out_n", 64.4, 131.0, "out", "near360", {}),
    ("out_ne", 128.0, 128.0, "out", "near360", {}),
    # well outside, the grid within zfar: 360 degrees, 90 degrees at the grid, 90 degrees away from it (empty by design)
    ("far_w_360", -200.3, 64.29, "out", "near360", dict(z=(100.0, 60000.0))),
    ("far_w_at", -200.3, 64.29, "out", "near360", dict(z=(100.0, 60000.0), az=(45.0, 135.0))),
    ("far_w_away", -200.3, 64.29, "out", "near360", dict(z=(100.0, 60000.0), az=(225.0, 315.0), empty=True)),
    ("far_n_360", 64.37, 400.2, "out", "near360", dict(z=(100.0, 60000.0))),
    ("far_n_at", 64.37, 400.2, "out", "near360", dict(z=(100.0, 60000.0), az=(135.0, 225.0))),
    ("far_n_away", 64.37, 400.2, "out", "near360", dict(z=(100.0, 60000.0), az=(-45.0, 45.0), empty=True)),
    # the whole grid beyond zfar
    ("beyond_zfar", -2000.0, -2000.0, "out", "near360", dict(empty=True)),
    # extents (170, 530) put the image's seam at azimuth 170: seen from the south the grid lies around azimuth 0, in the
    # middle of the image; seen from the north it lies around azimuth 180 and straddles the seam
    ("seam_from_s", 60.2, -30.4, "out", "near360", dict(az=(170.0, 530.0))),
    ("seam_from_n", 70.3, 160.6, "out", "near360", dict(az=(170.0, 530.0))),
)
EDGE_SIZES = (2, 3, 4, 5, 63, 64, 65, 66, 126, 127, 128, 129, 190, 191)
EDGE_SIZE_GROUNDS = ("spikes", "checker", "plateau")
EDGE_SIZE_W, EDGE_SIZE_H = 320, 80


# Dropped from the list: the one case on which the oracle's draw differs from llvmpipe's, in one pixel.  Triangle 11005 there is
# a sliver 68 pixels tall whose area is positive in the snapped 1/256-pixel positions (5544/65536 px^2: llvmpipe's rasteriser
# and the oracle draw it) and negative in the unsnapped float positions.  Mesa's draw module culls by the float area, but only
# the triangles of a batch that holds a clipped vertex: drawn alone, or with an unclipped triangle, llvmpipe fills the pixel;
# with a triangle across the image border in the same call it does not.  GL leaves the precision of the facing test to the
# implementation, and which triangles share a batch is nothing the oracle can restate
EDGE_DROPPED = ("i126_j127-checker",)


def _edge_above(m, ci, cj):
    """10 m above the highest of the four samples around the viewer, as the zoo's "above"; samples outside the window count
    as -1 (what the DEM reader returns there)"""
    N = m.shape[0]
    i0, j0 = int(np.floor(ci)), int(np.floor(cj))
    z = [int(m[j, i]) if 0 <= i < N and 0 <= j < N else -1 for j in (j0, j0 + 1) for i in (i0, i0 + 1)]
    return float(max(z)) + 10.0


def _edge_case(cid, family, recipe, over, N, W, H, ci, cj, kind, k):
    f32 = np.float32
    r = dict(_ZOO_VIEWS[recipe]); r.update(over)
    ci, cj = f32(ci), f32(cj)
    vz = r["vz"]
    if vz == "above":
        vz = _edge_above(zoo_mosaic(family, N), ci, cj)
    zc = r.get("zc", r["z"])
    view = dict(viewer_cell_i=ci, viewer_cell_j=cj, viewer_z=f32(vz), cos_viewer_lat=f32(_ZOO_COS[r["lat"]]),
                deg_per_cell=f32(1.0) / f32(r["cpd"]), az_deg0=f32(r["az"][0]), az_deg1=f32(r["az"][1]),
                aspect=f32(W) / f32(H), znear=f32(r["z"][0]), zfar=f32(r["z"][1]),
                znear_color=f32(zc[0]), zfar_color=f32(zc[1]))
    c0, c1 = (W // 5 + k % 97, W // 5 + k % 97 + W // 3) if k % 2 else (0, W)
    return dict(id=cid, family=family, recipe=recipe, lat=r["lat"], cpd=r["cpd"], N=N, W=W, H=H, kind=kind,
                view={n: float(x) for n, x in view.items()}, c0=c0, c1=c1, empty=bool(r.get("empty", False)))


def edge_cases():
    """viewer positions at the edges of the grid and of its 63-cell strips, and DEM sizes around whole strips, deterministic:
    dicts with id, family, recipe, N, W, H, view (float32-representable floats), kind (see _EDGE_POSITIONS; the sizes: "size"),
    pos (the position's tag), c0, c1 (a sector on every other case) and empty (no terrain by design).  Every position on
    N = 128 under one of EDGE_GROUNDS in rotation; every N of EDGE_SIZES from three places, each under one of EDGE_SIZE_GROUNDS in rotation"""
    f32 = np.float32
    cases = []
    for n, (tag, ci, cj, kind, recipe, over) in enumerate(_EDGE_POSITIONS):
        # (one ground per position, in rotation: under three each - the cross the list began with - the GPU tests on this list
        # took a third of the suite's time before them; the decisions these positions are for depend on where the viewer
        # stands, not on the heights)
        grounds = [EDGE_GROUNDS[(n + t) % len(EDGE_GROUNDS)] for t in range(2)]
        grounds = [g for g in grounds if f"{tag}-{g}" not in EDGE_DROPPED][:1]
        for family in grounds:
            if family == "stairs" and cj > EDGE_N - 1:          # (the stairs climb northwards: from the north, 10 m up, only their back)
                family = "coast"
            c = _edge_case(f"{tag}-{family}", family, recipe, over, EDGE_N, EDGE_W, EDGE_H, ci, cj, kind, len(cases))
            c["pos"] = tag
            cases.append(c)
    for N in EDGE_SIZES:
        lo, hi = f32(0), f32(N - 1)
        places = (("mid", min(max(f32(N // 2) + f32(0.37), lo), hi), min(max(f32(N // 2) - f32(0.29), lo), hi)),
                  ("corner", f32(0), f32(0)), ("outside", f32(-1.5), f32(N) + f32(0.5)))
        for p, (tag, ci, cj) in enumerate(places):
            for family in (EDGE_SIZE_GROUNDS[(EDGE_SIZES.index(N) + p) % len(EDGE_SIZE_GROUNDS)],):     # (one ground per place, in rotation)
                # (from outside: above the highest sample of the grid - 10 m above the -1 around it is below the ground)
                over = dict(vz=float(zoo_mosaic(family, N).max()) + 10.0) if tag == "outside" else {}
                if N <= 5:                                      # (the whole grid lies within near360's near clip of 100 m)
                    over["z"] = (1.0, 40000.0)
                if N == 2 and tag != "outside":                 # (seen from inside it, the one cell spans a quarter of the image or more:
                    over["empty"] = True                        #  the reference drops both triangles)
                c = _edge_case(f"N{N}_{tag}-{family}", family, "near360", over, N, EDGE_SIZE_W, EDGE_SIZE_H, ci, cj, "size", len(cases))
                c["pos"] = tag
                cases.append(c)
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


def edge_offsets(c):
    """the east and north offsets of every vertex column and row of an edge case from the viewer, in metres, as float32
    arithmetic forms them (hz_num.h: hz_east, hz_north): what hz_fast.h's range test sees"""
    f32 = np.float32
    v = c["view"]
    k = f32(20015088.0)
    fi = np.arange(c["N"], dtype=f32)
    e = (fi - f32(v["viewer_cell_i"])) * k * f32(v["deg_per_cell"]) / f32(180.0) * f32(v["cos_viewer_lat"])
    n = (fi - f32(v["viewer_cell_j"])) * k * f32(v["deg_per_cell"]) / f32(180.0)
    return e.astype(f32), n.astype(f32)


# ---- texture placements for the zoo: where the DEM window lies on the mosaic of map tiles -----------------

# placement -> s at the window's west and east edge, t over one window height of latitude, and the curvature
# dlat2 as a multiple of dlat1/span.  `inside` is what every earlier textured test had; the others put coordinates
# beyond [0,1] (GL_REPEAT), many texels per pixel, a few texels over the whole window, decreasing s, and the wrap
# seam itself under the viewer
ZOO_TEX_PLACEMENTS = {
    "inside":    ((0.05, 0.95), (0.1, 0.9), 0.0),
    "wrap":      ((-0.3, 1.4), (-0.2, 1.1), 0.2),
    "far_out":   ((37.2, 38.9), (-12.6, -11.3), 0.2),
    "minified":  ((0.0, 40.0), (0.0, 25.0), -0.3),
    "magnified": ((0.5, 0.5 + 3.0 / 768.0), (0.25, 0.25 + 2.0 / 512.0), 0.0),
    "flipped":   ((1.2, -0.1), (0.9, 0.1), 0.5),
    "seam":      ((0.999, 1.001), (-0.001, 0.001), 0.0),
}
ZOO_TEX_TILES = ((3, 2), (2, 3), (1, 1), (5, 1), (1, 4))        # 768, 512, 256, 1280, 1024 texels: power of two and not
ZOO_TEX_BLOCKY = (1, 8, 4)
ZOO_TEX_FULL_CROSS = ("checker-zoom12", "cliff-z005", "coast-arctic90")


def zoo_tex(case, placement, ntiles):
    """texture parameters (hzlib.TexParams: the hz_texparams_t / oracle.OrcTex field names) that lay zoo case `case`'s
    DEM window on a mosaic of ntiles = (x, y) map tiles as ZOO_TEX_PLACEMENTS[placement] says.  float32 multiplies,
    divisions and additions only, so that fixtures store names and not numbers"""
    f32 = np.float32
    (s_lo, s_hi), (t_lo, t_hi), curve = ZOO_TEX_PLACEMENTS[placement]
    ntx, nty = ntiles
    span = f32(case["N"]) * f32(case["view"]["deg_per_cell"]) * f32(0.017453292)         # the window's extent in radians
    t = hzlib.TexParams()
    t.viewer_lat_rad = f32(0.3) * span
    t.origin_cell_lon_deg = t.origin_cell_lat_deg = 0.0
    t.ntiles_x, t.ntiles_y, t.lowest_x, t.lowest_y = ntx, nty, 700, 1600
    t.tex_w, t.tex_h = 256 * ntx, 256 * nty
    t.lon0 = f32(700) + f32(s_lo) * f32(ntx)
    t.lon1 = (f32(s_hi) - f32(s_lo)) * f32(ntx) / span
    t.dlat0 = f32(1600) + f32(nty) * (f32(1) - f32(t_lo))
    dlat1 = -(f32(t_hi) - f32(t_lo)) * f32(nty) / span
    t.dlat1 = dlat1
    t.dlat2 = f32(curve) * (dlat1 / span)
    return t


def orc_tex(t):
    """oracle.OrcTex with the values of anything that has its field names"""
    import oracle
    o = oracle.OrcTex()
    for name, _ in hzlib.TexParams._fields_:
        setattr(o, name, getattr(t, name))
    return o


def zoo_tex_cases():
    """the textured zoo's list, deterministic: every zoo case under one placement in rotation, the three of
    ZOO_TEX_FULL_CROSS under all seven; tile counts, texture seed and blockiness rotate with the entry's number.
    dicts with id, name (the zoo case's), placement, ntiles, seed, blocky"""
    names = list(ZOO_TEX_PLACEMENTS)
    pairs = []
    for k, c in enumerate(zoo_cases()):
        mine = [names[k % len(names)]]
        if c["name"] in ZOO_TEX_FULL_CROSS:
            mine += [p for p in names if p != mine[0]]
        pairs += [(c["name"], p) for p in mine]
    return [dict(id=f"{name}-{p}", name=name, placement=p, ntiles=ZOO_TEX_TILES[n % len(ZOO_TEX_TILES)], seed=n,
                 blocky=ZOO_TEX_BLOCKY[n % len(ZOO_TEX_BLOCKY)]) for n, (name, p) in enumerate(pairs)]


def zoo_tex_sectors():
    """narrow and odd sectors of the cases whose near ground the clipper cuts: (case name, first column, one past the
    last).  In a sector a few columns wide a chunk of 256 pixels spans many rows, and a clipped triangle starts a run
    on every one of them"""
    zoo = {c["name"]: c for c in zoo_cases()}
    out = []
    for name in ("checker-zoom12", "checker-vertex360", "checker-near360", "max16-near360", "bowl-vertex360"):
        W = zoo[name]["W"]
        out += [(name, W // 2, W // 2 + 1), (name, W // 3, W // 3 + 17), (name, 5, 68), (name, 0, 64), (name, W - 65, W)]
    out.append(("cliff-z005", 447, 512))
    return out


def zoo_tex_entry(name, placement="wrap"):
    """the entry of zoo_tex_cases() for a zoo case: under `placement` where it has that one, else the one it has"""
    mine = [e for e in zoo_tex_cases() if e["name"] == name]
    return next((e for e in mine if e["placement"] == placement), mine[0])


def zoo_tex_inputs(e, case=None):
    """(texture parameters, texels) of an entry of zoo_tex_cases()"""
    if case is None:
        case = next(c for c in zoo_cases() if c["name"] == e["name"])
    t = zoo_tex(case, e["placement"], e["ntiles"])
    return t, hash_texture(t.tex_h, t.tex_w, seed=e["seed"], blocky=e["blocky"])


# ---- .hgt tiles anywhere on Earth, with what real SRTM holds and tools/demgen.c does not write ----------------

def hgt_tile_name(lat, lon):
    """file name of the tile whose south-west corner is (lat, lon), integers: N/S + 2 digits, E/W + 3 digits"""
    return "%s%02d%s%03d.hgt" % ("S" if lat < 0 else "N", abs(lat), "W" if lon < 0 else "E", abs(lon))


def hgt_tile_values(lat, lon, cpd=1200):
    """int16[cpd+1,cpd+1], row 0 = northern edge: integer-hash terrain keyed on the absolute sample position (tiles
    agree along shared edges), blocky hills with sea-level flats, and sprinkled over them negative heights,
    -32768 voids and heights above 16383"""
    row, col = np.mgrid[0:cpd + 1, 0:cpd + 1].astype(np.int64)
    gi = (lon + 400) * cpd + col                 # absolute east index, offset to stay positive
    gj = (lat + 400) * cpd + (cpd - row)         # absolute north index
    z = np.maximum(0, (_zoo_hash(gi // 12, gj // 12, 11) % np.uint64(2400)).astype(np.int64) - 800)
    z = np.where(z > 0, z + (_zoo_hash(gi, gj, 12) % np.uint64(40)).astype(np.int64), 0)
    h = _zoo_hash(gi, gj, 13)
    z = np.where(h % np.uint64(31) == 0, -32768, z)
    z = np.where(h % np.uint64(29) == 1, -1 - (h % np.uint64(400)).astype(np.int64), z)
    z = np.where(h % np.uint64(37) == 2, 16384 + (h % np.uint64(16000)).astype(np.int64), z)
    return z.astype(np.int16)


def write_hgt_tiles(directory, lat_lo, lat_hi, lon_lo, lon_hi, cpd=1200, missing=()):
    """big-endian int16 tiles covering the integer box, except those named in `missing`"""
    os.makedirs(directory, exist_ok=True)
    for lat in range(lat_lo, lat_hi + 1):
        for lon in range(lon_lo, lon_hi + 1):
            name = hgt_tile_name(lat, lon)
            path = os.path.join(directory, name)
            if name[:-4] in missing or os.path.exists(path) and os.path.getsize(path) == 2 * (cpd + 1) ** 2:
                continue
            tmp = path + ".%d.tmp" % os.getpid()
            hgt_tile_values(lat, lon, cpd).astype(">i2").tofile(tmp)
            os.replace(tmp, path)
    return directory


# places away from the N/W quadrant: name -> viewpoint, window radius, the tiles the window touches, the tile left out,
# a second viewpoint inside the window
WORLD_CASES = {
    "equator_greenwich": dict(lat=0.0137, lon=-0.0121, R=100, tiles=("S01W001", "S01E000", "N00W001", "N00E000"), missing=(),
                              moved=(-0.021, 0.033)),
    "south_east":        dict(lat=-43.6, lon=170.1, R=150, tiles=("S44E169", "S44E170"), missing=(), moved=(-43.63, 170.02)),
    "arctic_gap":        dict(lat=69.98, lon=20.03, R=120, tiles=("N69E019", "N69E020", "N70E019", "N70E020"),
                              missing=("N70E020",), moved=(70.01, 19.97)),
}


def world_dem_dir(name):
    """directory with the tiles of WORLD_CASES[name] (generated on first use, cached)"""
    c = WORLD_CASES[name]
    return write_hgt_tiles(os.path.join(_DEM_ROOT, "world_" + name), *tiles_for(c["lat"], c["lon"], c["R"]), missing=c["missing"])
