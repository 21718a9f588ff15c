"""The inputs tests/test_gpu_annot_zoo.py hands to the annotator kernels, and what they must answer: ten draws of the terrain
zoo (with a not-quite-360 degree variant of each full-circle view), the oracle's render of each, a list of projected points
of interest crafted from that render so that every exit of the search is taken (tests/test_naive_annot.py holds the list to
that), and tests/naive_annot.py's answers.  TEST CODE, CPU only: the GPU tests compare the device with what this module
computes, never with the device's own output."""
import functools

import numpy as np

import hzutil
import naive_annot as na
import oracle

NAMES = ("cliff-near360", "spikes-arctic90", "checker-sky", "coast-zoom12", "stairs-corner90", "flat0-high_wrap",
         "spikes-inf_far", "flat0-z005", "checker-zoom12", "border_minus1-vertex360")
VIEWER_LON = 7.25                       # the zoo's views have no longitude: any will do
CELLS = ((14, 14), (1, 1), (7, 31), None)               # None: (W-1) x (H-1), one cell per image
COUNTS = (0, 1, 255, 256, 257)


def _inputs():
    zoo = {c["name"]: c for c in hzutil.zoo_cases()}
    out = {}
    for name in NAMES:
        c = zoo[name]
        variants = [(name, c["view"])]
        if float(c["view"]["az_deg1"]) - float(c["view"]["az_deg0"]) == 360.0:
            # an exact 360 degree span refuses every projection (reference horizonator_x_from_az): the view the
            # reference's CLI asks for instead
            variants.append((name + "~", dict(c["view"], az_deg0=float(np.float32(-179.9)), az_deg1=float(np.float32(179.95)))))
        for key, view in variants:
            out[key] = dict(key=key, name=name, family=c["family"], N=c["N"], W=c["W"], H=c["H"], view=view, lat=float(c["lat"]),
                            lon=VIEWER_LON, ele=float(view["viewer_z"]), degenerate=c["degenerate"], zoo=c)
    return out


INPUTS = _inputs()
KEYS = tuple(INPUTS)


def cuts_poi(H):
    return (0, 20, H - 3, H + 5, -4)


def cells_and_cuts(W, H):
    """every (cell_w, cell_h, cut) of the link-cell checks: cuts 0, 37 and the largest that leaves one row of cells"""
    out = []
    for cell in CELLS:
        cw, ch = cell if cell else (W - 1, H - 1)
        for cut in (0, 37, H - ch - 1):
            if cut >= 0 and (cw, ch, cut) not in out:
                out.append((cw, ch, cut))
    return out


@functools.lru_cache(maxsize=None)
def mosaic(key):
    c = INPUTS[key]
    return hzutil.zoo_mosaic(c["family"], c["N"])


@functools.lru_cache(maxsize=None)
def want_render(key):
    """the oracle's render of the input: dict(bgr, ranges, index, z24).  Shared: nobody writes into it"""
    c = INPUTS[key]
    out = oracle.render(mosaic(key), oracle.make_view(**c["view"]), c["W"], c["H"])
    for a in out.values():
        a.setflags(write=False)
    return out


def _shift_rows(R, k):
    """S[r] = R[r+k], rows from outside the image as sky"""
    S = np.full_like(R, -1.0)
    if k == 0:
        S[:] = R
    elif k < 0:
        S[-k:] = R[:k]
    else:
        S[:-k] = R[k:]
    return S


def crafted_proj(ranges, seed=0):
    """projected points (x, y, range) float64[n,3] made from a range image so that the search around them takes every way
    out it has: the distance window's two ends hit exactly and missed narrowly, crosshairs whose round() lands on column W,
    column -1, row H, crosshairs above the image and with fraction exactly .5 (also below -0.5, where round() and
    floor(y + .5) part), windows cut by the top row, by height_out and by the image's bottom, the skyline (sky skipped, then
    terrain), columns whose range does not fall monotonically (the `else break` decides), two rows equally far from the
    wanted range, NaN ranges, the first and the last row of the window as the answer"""
    R = np.asarray(ranges, np.float32)
    H, W = R.shape
    rng = np.random.default_rng(seed)
    P = [(0.0, 0.0, -1.0), (W / 2.0, H / 2.0, -0.5)]

    def add(x, y, r):
        P.append((float(x), float(y), float(r)))

    def some(mask, n):
        yy, xx = np.nonzero(mask)
        if len(yy) == 0:
            return []
        pick = rng.choice(len(yy), size=min(n, len(yy)), replace=False)
        return [(int(yy[k]), int(xx[k])) for k in sorted(pick)]

    def val(r, x, default=1000.0):
        v = float(R[r, x]) if 0 <= r < H and 0 <= x < W else -1.0
        return v if v > 0 else default

    def inwin(v):
        return min(max(v, 500.0), 100000.0)

    with np.errstate(invalid="ignore"):
        sky = R <= 0
    nan = np.isnan(R)
    T = ~sky & ~nan
    pixels = some(T, 40) + some(np.ones_like(T), 10)
    for r, x in pixels:
        v = val(r, x)
        add(x, r, v); add(x + 0.3, r - 0.4, v); add(x, r + 0.5, inwin(v)); add(x - 0.5, r - 3.5, inwin(v))
        add(x, r, 499.99); add(x, r, 100000.01); add(x, r, 500.0); add(x, r, 100000.0)
        add(x, r, inwin(v) + 2000.0); add(x, r, inwin(v) + 499.9)
        add(x, r + 6, inwin(v)); add(x, r - 5, inwin(v)); add(x, r + 5, inwin(v)); add(x, r - 6, inwin(v))
    # the image's edges
    for r, x in some(np.ones_like(T), 12) + some(T, 12):
        v = inwin(val(r, x))
        add(W - 0.5, r, inwin(val(r, W - 1))); add(-0.5, r, inwin(val(r, 0))); add(W - 0.51, r, inwin(val(r, W - 1)))
        add(-0.49, r, inwin(val(r, 0))); add(W + 3.0, r, v); add(-7.2, r, v)
        for y in (-0.5, -1.5, -2.5, -5.5, -6.0, -7.0, 0.0, 2.0, 0.49):
            add(x, y, inwin(val(1, x)))
        for y in (H - 0.5, H - 1.0, H - 1.5, H - 3.0, H - 5.5, H + 2.0, H + 5.0, H + 6.5):
            add(x, y, inwin(val(H - 1, x))); add(x, y, inwin(val(H - 2, x)))
    # the skyline: sky at r, terrain at r+1
    for r, x in some(sky[:-1] & T[1:], 25):
        add(x, r + 3, inwin(val(r + 1, x))); add(x, r - 2.5, inwin(val(r + 1, x))); add(x, r + 6.2, inwin(val(r + 2, x)))
    # sky holes: terrain at r, sky at r+1
    for r, x in some(T[:-1] & sky[1:], 25):
        add(x, r + 2, inwin(val(r, x))); add(x, r - 3, inwin(val(r + 3, x, val(r, x))))
    # ties: the mean of two neighbouring rows' ranges is exactly as far from both
    for r, x in some(T[:-1] & T[1:], 25):
        a, b = float(R[r, x]), float(R[r + 1, x])
        add(x, r + 6, inwin((a + b) / 2.0)); add(x, r + 2.5, inwin((a + b) / 2.0))
    for r, x in some(nan, 12):
        add(x, r, 1000.0); add(x, r + 6, 1000.0); add(x + 0.4, r - 5.3, 70000.0)
    # crosshair at row r - 5 wanting the range of row r, the window's last: the scan gets there only while every row on the
    # way is nearer than the one before; where it does not, the `else break` decides and the full-window minimum is row r
    base = T & (R >= 500.0) & (R <= 100000.0)
    base[:11] = False
    R64 = R.astype(np.float64)
    best = np.full(R.shape, np.inf)
    alive = np.ones(R.shape, bool)
    with np.errstate(invalid="ignore"):
        for k in range(12):
            S = _shift_rows(R, k - 11).astype(np.float64)
            valid = ~(S <= 0)
            err = np.abs(R64 - S)
            upd = alive & valid & (err < best)
            alive &= ~(valid & ~upd)
            best = np.where(upd, err, best)
    for r, x in some(base & ~alive, 20) + some(base & alive, 20):
        add(x, r - 5, float(R[r, x])); add(x + 0.25, r - 5.25, float(R[r, x]))
    return np.array(P, np.float64)


def ground_pois(key):
    """every third mosaic cell's ground point, the same points 400 m below and 2 km above: float32[n,3] lat, lon, ele"""
    c = INPUTS[key]
    m, v = mosaic(key), c["view"]
    jj, ii = np.meshgrid(np.arange(0, c["N"], 3), np.arange(0, c["N"], 3), indexing="ij")
    glat = c["lat"] + (jj - float(v["viewer_cell_j"])) * float(v["deg_per_cell"])
    glon = c["lon"] + (ii - float(v["viewer_cell_i"])) * float(v["deg_per_cell"])
    gele = m[jj, ii].astype(np.float64)
    return np.concatenate([np.stack([glat.ravel(), glon.ravel(), gele.ravel() + dz], 1) for dz in (0.0, -400.0, 2000.0)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def proj_list(key):
    """the projected points of an input: the crafted ones, then naive_annot's projection of the ground points"""
    c = INPUTS[key]
    v = c["view"]
    p = np.concatenate([crafted_proj(want_render(key)["ranges"], seed=len(key)),
                        na.project_pois(ground_pois(key), c["lat"], c["lon"], c["ele"], v["az_deg0"], v["az_deg1"], c["W"], c["H"])])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def want_poi(key, cut):
    """naive_annot.poi_search on the oracle's range image: (visible, label_x, label_y, tags)"""
    return na.poi_search(want_render(key)["ranges"], INPUTS[key]["H"] - cut, proj_list(key))


def cos_lat(key):
    return float(na.cos(np.float64(INPUTS[key]["lat"]) * np.float64(na.M_PI) / np.float64(180.0)))


@functools.lru_cache(maxsize=None)
def want_link(key, cw, ch, cut):
    c = INPUTS[key]
    return na.link_cells(want_render(key)["ranges"], cut, cw, ch, c["lat"], c["lon"], c["view"]["az_deg0"], c["view"]["az_deg1"])


def depth_pixels(key, c0=0, c1=None, n=200):
    """about n pixels (x, y) of columns [c0, c1): the four corners, both sides of the skyline, the rest seeded"""
    c = INPUTS[key]
    W, H = c["W"], c["H"]
    c1 = W if c1 is None else c1
    z = want_render(key)["z24"]
    rng = np.random.default_rng(7)
    pts = [(c0, 0), (c1 - 1, 0), (c0, H - 1), (c1 - 1, H - 1)]
    terrain = z[:, c0:c1] != 0xFFFFFF
    yy, xx = np.nonzero(~terrain[:-1] & terrain[1:])
    for k in rng.permutation(len(yy))[:40]:
        pts += [(c0 + int(xx[k]), int(yy[k])), (c0 + int(xx[k]), int(yy[k]) + 1)]
    while len(pts) < n:
        pts.append((int(rng.integers(c0, c1)), int(rng.integers(0, H))))
    return pts
