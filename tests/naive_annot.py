"""A second, deliberately naive restatement of the annotator arithmetic: the reference's horizonator_project /
horizonator_unproject (reference horizonator-lib.c:1053-1213), the two passes its annotator makes over the range image
(annotator.c:228-264 and :297-347) and horizonator_pick (horizonator-lib.c:1267-1295).

TEST CODE.  Written from the reference's text alone, statement by statement; it shares no code with oracle/ (the C
restatement, oracle_annot.c) nor with horizonator_amd/csrc/hz_host.c and the kernels (the product), so that a misreading
the two have in common would show here (tests/test_naive_annot.py, tests/test_gpu_annot_zoo.py).  The only things it
borrows are glibc's own sinf / cosf / cos / atan2 / sqrt / round through ctypes - the functions the reference itself calls;
NumPy's float32 sine is not glibc's.

C semantics spelled out: a `double` is a Python float or a NumPy float64, a `float` a NumPy float32, and each rounds after
every operation; an expression with a double in it (M_PI, 2., 180., a double argument) is evaluated in double from that
operand on and rounded when it is assigned to a float.  The double-only functions (project, the search) run on Python
floats, one point at a time; unproject takes scalars or arrays, element by element - the same IEEE operations either way -
so that an image of 1x1 link cells does not take minutes.
"""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
M_PI = 3.14159265358979323846
DBL_MAX = 1.7976931348623157e308

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
for _n in ("cos", "sqrt", "round"):
    getattr(_libm, _n).restype = ctypes.c_double
    getattr(_libm, _n).argtypes = [ctypes.c_double]
_libm.atan2.restype = ctypes.c_double
_libm.atan2.argtypes = [ctypes.c_double, ctypes.c_double]


def _each(fn, dtype, bits):
    """glibc's fn on a scalar or on every element of an array (once per distinct bit pattern)"""
    def call(x):
        x = np.asarray(x, dtype)
        if x.ndim == 0:
            return dtype(fn(float(x)))
        u, inv = np.unique(np.ascontiguousarray(x).view(bits).ravel(), return_inverse=True)
        r = np.array([fn(float(v)) for v in u.view(dtype)], dtype)
        return r[inv.ravel()].reshape(x.shape)
    return call


sinf = _each(_libm.sinf, f32, np.uint32)
cosf = _each(_libm.cosf, f32, np.uint32)
cos = _each(_libm.cos, f64, np.uint64)
c_atan2, c_sqrt, c_round = _libm.atan2, _libm.sqrt, _libm.round


# ---- reference horizonator-lib.c:1053-1155, all in double -------------------------------------------------------------

def unwrap_near_rad(x, near):
    """:1055-1060"""
    d = (x - near) / (2. * M_PI)
    return (d - c_round(d)) * 2. * M_PI + near


def x_from_az(az_rad, az_rad0, az_rad1, width):
    """:1062-1095: (x, az_ndc_per_rad), or None where the azimuth is outside the view"""
    az_rad1 = unwrap_near_rad(az_rad1 - az_rad0, M_PI) + az_rad0
    az_rad_center = (az_rad0 + az_rad1) / 2.
    az_rad = unwrap_near_rad(az_rad, az_rad_center)
    try:
        az_ndc_per_rad = 2.0 / (az_rad1 - az_rad0)
    except ZeroDivisionError:                       # C: 2.0 / 0.0 = +inf (an exact 360 degree span collapses to this)
        az_ndc_per_rad = float("inf")
    az_ndc = (az_rad - az_rad_center) * az_ndc_per_rad
    if not (-1. <= az_ndc and az_ndc <= 1.):
        return None
    return (az_ndc + 1.) / 2. * width - 0.5, az_ndc_per_rad


def project(lat_viewer, cos_lat_viewer, lon_viewer, ele_viewer, lat, lon, ele, az_rad0, az_rad1, width, height):
    """:1097-1155: (x, y, range), or None where the reference returns false"""
    lat_viewer, cos_lat_viewer, lon_viewer, ele_viewer = float(lat_viewer), float(cos_lat_viewer), float(lon_viewer), float(ele_viewer)
    lat, lon, ele, az_rad0, az_rad1 = float(lat), float(lon), float(ele), float(az_rad0), float(az_rad1)
    Rearth = float(f32(6371000.0))
    dlat = (lat - lat_viewer) * M_PI / 180.
    dlon = (lon - lon_viewer) * M_PI / 180.
    east = dlon * Rearth * cos_lat_viewer
    north = dlat * Rearth
    distance_sq_ne = east * east + north * north
    xk = x_from_az(c_atan2(east, north), az_rad0, az_rad1, width)
    if xk is None:
        return None
    x, az_ndc_per_rad = xk
    h = ele - ele_viewer
    distance_ne = c_sqrt(distance_sq_ne)
    rng = c_sqrt(distance_sq_ne + h * h)
    aspect = float(width) / float(height)
    el_ndc = c_atan2(h, distance_ne) * aspect * az_ndc_per_rad
    if not (-1. <= el_ndc and el_ndc <= 1.):
        return None
    y = (-el_ndc + 1.) / 2. * height - 0.5
    return x, y, rng


# ---- reference horizonator-lib.c:1157-1213: the float/double mix as the reference has it ------------------------------

def unproject(x, y, range_enh, range_en, lat_viewer, cos_lat_viewer, lon_viewer, az_deg0, az_deg1, width, height):
    """(ok, lat, lon): ok is what the reference returns; lat / lon float32, meaningless where not ok.
    x, y ints and range_enh, range_en doubles, scalars or arrays of one shape; the rest double scalars"""
    lat_viewer, cos_lat_viewer, lon_viewer = f64(lat_viewer), f64(cos_lat_viewer), f64(lon_viewer)
    az_deg0, az_deg1 = f64(az_deg0), f64(az_deg1)
    range_enh, range_en = np.asarray(range_enh, f64), np.asarray(range_en, f64)
    with np.errstate(all="ignore"):
        ok = 1 == (range_enh > 0.).astype(int) + (range_en > 0.).astype(int)
        Rearth = f32(6371000.0)
        az_ndc = (np.asarray(x).astype(f32) + f32(0.5)) / f32(width) * f32(2.) - f32(1.)
        # az_ndc * (double) / 2.f + (double)/2.f, that * M_PI / 180.0f: double throughout, rounded by the assignment
        az = ((az_ndc.astype(f64) * (az_deg1 - az_deg0) / f64(2.) + (az_deg1 + az_deg0) / f64(2.)) * f64(M_PI) / f64(180.)).astype(f32)
        # if(range_en <= 0): have range_enh, need range_en
        aspect = f64(width) / f64(height)
        el_ndc = (np.asarray(y).astype(f64) + f64(0.5)) / f64(height) * f64(2.) - f64(1.)
        el = el_ndc * (az_deg1 - az_deg0) / f64(2.) / aspect * f64(M_PI) / f64(180.)
        range_en = np.where(range_en <= 0, cos(el) * range_enh, range_en)
        e = (range_en * sinf(az).astype(f64)).astype(f32)
        n = (range_en * cosf(az).astype(f64)).astype(f32)
        # e / Rearth is a float quotient; / M_PI takes it to double
        lon = (lon_viewer + (e / Rearth).astype(f64) / f64(M_PI) * f64(180.) / cos_lat_viewer).astype(f32)
        lat = (lat_viewer + (n / Rearth).astype(f64) / f64(M_PI) * f64(180.)).astype(f32)
    return ok, lat, lon


# ---- reference annotator.c:228-264 ------------------------------------------------------------------------------------

def _cells(width, height, cell_w, cell_h, cut):
    """the trip values of the reference's two loops (:230, :232)"""
    height_out = height - cut
    return list(range(0, width - cell_w, cell_w)), list(range(0, height_out - cell_h, cell_h))


def link_tables(W, H, az_deg0, az_deg1, cell_w, cell_h, cut):
    """include/hz_hip.h:189-203: nx, ny and what hz_hip_link_cells wants from its caller - sinf / cosf of the azimuth of
    the centre column of each cell column (float32[nx]), cos of the elevation of the centre row of each cell row
    (float64[ny]) - evaluated as horizonator_unproject does (:1183-1184, :1199-1203)"""
    xs, ys = _cells(W, H, cell_w, cell_h, cut)
    az_deg0, az_deg1 = f64(az_deg0), f64(az_deg1)
    sin_az, cos_az, cos_el = np.empty(len(xs), f32), np.empty(len(xs), f32), np.empty(len(ys), f64)
    for cx, x0 in enumerate(xs):
        x = x0 + cell_w // 2
        az_ndc = (f32(x) + f32(0.5)) / f32(W) * f32(2.) - f32(1.)
        az = f32((f64(az_ndc) * (az_deg1 - az_deg0) / f64(2.) + (az_deg1 + az_deg0) / f64(2.)) * f64(M_PI) / f64(180.))
        sin_az[cx], cos_az[cx] = sinf(az), cosf(az)
    for cy, y0 in enumerate(ys):
        y = y0 + cell_h // 2
        aspect = f64(W) / f64(H)
        el_ndc = (f64(y) + f64(0.5)) / f64(H) * f64(2.) - f64(1.)
        el = el_ndc * (az_deg1 - az_deg0) / f64(2.) / aspect * f64(M_PI) / f64(180.)
        cos_el[cy] = cos(el)
    return len(xs), len(ys), sin_az, cos_az, cos_el


def link_cells(ranges, cut, cell_w, cell_h, lat, lon, az_deg0, az_deg1):
    """:228-264 on a range image float32[H,W]: (lat, lon) float32[ny,nx] of the cells the reference makes a link for,
    NaN for those it skips.  The two loops are stated as index grids: every cell goes through the same statements"""
    ranges = np.asarray(ranges, f32)
    H, W = ranges.shape
    xs, ys = _cells(W, H, cell_w, cell_h, cut)
    la = np.full((len(ys), len(xs)), np.nan, f32)
    lo = np.full((len(ys), len(xs)), np.nan, f32)
    if not xs or not ys:
        return la, lo
    cos_lat = cos(f64(lat) * f64(M_PI) / f64(180.))                             # :207
    y, x = np.meshgrid(np.array(ys), np.array(xs), indexing="ij")
    rng = ranges[y, x]
    with np.errstate(invalid="ignore"):
        skipped = rng <= f32(0.0)                                               # :236 "no render data here"
    ok, lat_cell, lon_cell = unproject(x + cell_w // 2, y + cell_h // 2, rng.astype(f64), -1.,
                                       lat, cos_lat, lon, az_deg0, az_deg1, W, H)
    made = ~skipped & ok
    la[made], lo[made] = lat_cell[made], lon_cell[made]
    return la, lo


# ---- reference annotator.c:297-347 ------------------------------------------------------------------------------------

MAX_MARKER_DIST, MIN_MARKER_DIST, FUZZ_RANGE, FUZZ_PIXEL_Y = 100000.0, 500.0, 500., 6

# what poi_search says about the way a point took through the search (tests/test_naive_annot.py: coverage conditions)
TAGS = ("refused", "near", "far", "at_min", "at_max", "clip_top", "height_out", "col_outside", "row_outside",
        "sky_then_terrain", "break_decided", "tie", "nan", "rejected", "fuzz-6", "fuzz+5", "y_half")


def poi_search(ranges, height_out, proj):
    """:297-347 for points already projected: proj float64[n,3] = crosshair x, y and range, range < 0 where
    horizonator_project refused the point.  Returns (visible uint8[n], label_x float32[n], label_y float32[n], tags):
    tags[k] is the set of TAGS naming the exits and branches point k met"""
    ranges = np.asarray(ranges, f32)
    H, W = ranges.shape
    img = ranges.astype(f64).tolist()                   # float -> double: exact
    proj = np.asarray(proj, f64).reshape(-1, 3)
    n = len(proj)
    visible, label_x, label_y, tags = np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, f32), []
    for k, (crosshair_x, crosshair_y, range_have) in enumerate(proj.tolist()):
        t = set()
        tags.append(t)
        if not (range_have >= 0.0):
            t.add("refused")
            continue
        if range_have < MIN_MARKER_DIST or range_have > MAX_MARKER_DIST:
            t.add("near" if range_have < MIN_MARKER_DIST else "far")
            continue
        if range_have == MIN_MARKER_DIST:
            t.add("at_min")
        if range_have == MAX_MARKER_DIST:
            t.add("at_max")
        if crosshair_y - np.floor(crosshair_y) == 0.5:
            t.add("y_half")
        fuzz_nearest = 0
        err_nearest = DBL_MAX
        broke = False
        sky_before = False
        yi, xi = int(c_round(crosshair_y)), int(c_round(crosshair_x))
        for fuzz in range(-FUZZ_PIXEL_Y, FUZZ_PIXEL_Y):
            if crosshair_y + float(fuzz) < 0:
                t.add("clip_top")
                continue
            if crosshair_y + float(fuzz) >= height_out:
                t.add("height_out")
                break
            yy = yi + fuzz
            # THIS PROJECT'S DECISION, not the reference's: the reference indexes range_image[width*yy + xi] without a
            # check and reads outside the image here; rows and columns outside it are skipped
            if xi < 0 or xi >= W:
                t.add("col_outside")
                continue
            if yy < 0 or yy >= H:
                t.add("row_outside")
                continue
            rng = img[yy][xi]
            if rng <= 0.0:
                sky_before = True
                continue
            if rng != rng:
                t.add("nan")
            err = abs(range_have - rng)
            if err < err_nearest:
                err_nearest = err
                fuzz_nearest = fuzz
                if sky_before:
                    t.add("sky_then_terrain")
            else:
                broke = True
                if err == err_nearest:
                    t.add("tie")
                break
        if broke:
            # for the tag alone: would the minimum over the whole window have been another row?
            for fuzz in range(-FUZZ_PIXEL_Y, FUZZ_PIXEL_Y):
                yy = yi + fuzz
                if 0 <= crosshair_y + float(fuzz) < height_out and 0 <= yy < H and 0 <= xi < W and img[yy][xi] > 0.0 \
                        and abs(range_have - img[yy][xi]) < err_nearest:
                    t.add("break_decided")
        if err_nearest < FUZZ_RANGE:
            visible[k] = 1
            label_x[k] = f32(crosshair_x)
            label_y[k] = f32(crosshair_y + float(f32(fuzz_nearest)))
            if fuzz_nearest == -FUZZ_PIXEL_Y:
                t.add("fuzz-6")
            if fuzz_nearest == FUZZ_PIXEL_Y - 1:
                t.add("fuzz+5")
        else:
            t.add("rejected")
    return visible, label_x, label_y, tags


def project_pois(pois, lat, lon, ele_m, az_deg0, az_deg1, W, H):
    """:284-295 for pois [n,3] = lat, lon, ele_m: float64[n,3] crosshair x, y, range; 0, 0, -1 where refused"""
    cos_lat = float(cos(f64(lat) * f64(M_PI) / f64(180.)))
    az_rad0, az_rad1 = float(az_deg0) * M_PI / 180., float(az_deg1) * M_PI / 180.
    out = np.empty((len(pois), 3), f64)
    for k, (plat, plon, pele) in enumerate(np.asarray(pois, f64).reshape(-1, 3).tolist()):
        p = project(lat, cos_lat, lon, ele_m, plat, plon, pele, az_rad0, az_rad1, W, H)
        out[k] = (0.0, 0.0, -1.0) if p is None else p
    return out


def poi_visibility(ranges, pois, cut, lat, lon, az_deg0, az_deg1, ele_m):
    """:280-348: project + poi_search, without the tags"""
    H, W = np.asarray(ranges).shape
    return poi_search(ranges, H - cut, project_pois(pois, lat, lon, ele_m, az_deg0, az_deg1, W, H))[:3]


# ---- reference horizonator-lib.c:1267-1295 ----------------------------------------------------------------------------

def pick(z24, x, y, view, viewer_lat, viewer_lon):
    """horizonator_pick on the depth image uint32[H,W] (top row first, as glReadPixels(x, height-1-y) addresses it; a
    24-bit depth buffer read as GL_FLOAT is float(z24 / (2^24 - 1)), tests/naive_host_math.py).  view: the uniform values
    (znear, zfar, az_deg0, az_deg1, cos_viewer_lat: floats); viewer_lat / viewer_lon: the context's floats.
    (lat, lon) float32, or None where the reference returns false"""
    H, W = z24.shape
    depth = f32(f64(z24[y, x]) / f64(16777215.0))
    if depth >= f32(1.0):
        return None
    znear, zfar = f32(view["znear"]), f32(view["zfar"])
    with np.errstate(all="ignore"):
        range_en = f64(depth * (zfar - znear) + znear)              # float arithmetic, assigned to a double
    ok, lat, lon = unproject(x, y, -1., range_en, f64(f32(viewer_lat)), f64(f32(view["cos_viewer_lat"])), f64(f32(viewer_lon)),
                             f64(f32(view["az_deg0"])), f64(f32(view["az_deg1"])), W, H)
    return (f32(lat), f32(lon)) if ok else None
