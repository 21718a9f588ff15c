"""tests/naive_annot.py (NumPy scalars, from the reference's text) against oracle/oracle_annot.c (C, from the same text) and
against the library's own host functions (hz_host.c): three statements of reference horizonator-lib.c:1053-1213 and
annotator.c:228-347 must agree bit for bit.  Then the conditions the GPU tests' inputs (tests/annot_cases.py) have to
meet: every exit and branch of the search is taken by at least one point.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import annot_cases as ac
import hzutil
import naive_annot as na
import oracle
from horizonator_amd import _lib

LAT, LON, ELE = hzutil.VIEW_LAT, hzutil.VIEW_LON, 1000.0
COSL = float(na.cos(np.float64(LAT) * np.float64(na.M_PI) / np.float64(180.0)))
# azimuth extents in degrees: the CLI's, both exact 360 degree spans, a zoom across north, a quadrant
VIEWS = ((-179.9, 179.95), (-180.0, 180.0), (170.0, 530.0), (354.0, 366.0), (0.0, 90.0))
SIZES = ((4000, 1000), (333, 111), (64, 64), (128, 64), (64, 128))


def _three_projects(lat, lon, ele, az0, az1, W, H, ele_viewer=ELE):
    """(naive, oracle, library): each None or (x, y, range)"""
    lib, orc = _lib.load(), oracle.load()
    r0, r1 = az0 * na.M_PI / 180., az1 * na.M_PI / 180.
    out = [na.project(LAT, COSL, LON, ele_viewer, lat, lon, ele, r0, r1, W, H)]
    for fn in (orc.orc_project, lib.horizonator_project):
        v = [C.c_double() for _ in range(3)]
        ok = fn(*[C.byref(a) for a in v], LAT, COSL, LON, ele_viewer, lat, lon, ele, r0, r1, W, H)
        out.append(tuple(a.value for a in v) if ok else None)
    return out


def _project_points(az0, az1, rng):
    pts = [(LAT + rng.uniform(-0.5, 0.5), LON + rng.uniform(-0.5, 0.5), rng.uniform(0, 3000)) for _ in range(150)]
    pts += [(LAT, LON, ELE), (LAT, LON, ELE + 1000.0), (LAT, LON, ELE - 1000.0)]        # atan2(0, 0); straight above, below
    pts += [(LAT + 0.1, LON, 1500.0), (LAT - 0.1, LON, 1500.0), (LAT, LON + 0.1, 900.0), (LAT, LON - 0.1, 900.0)]   # az 0, 180, 90, 270 exactly
    for az in (az0, az1):                       # along the view's two ends, and a hair to either side
        for d in (-1e-9, 0.0, 1e-9, -1e-4, 1e-4):
            a = np.deg2rad(az) + d
            pts.append((LAT + 0.05 * np.cos(a), LON + 0.05 * np.sin(a) / COSL, 1200.0))
    return pts


@pytest.mark.parametrize("az", VIEWS, ids=lambda a: "%g..%g" % a)
def test_project_is_the_oracles_and_the_librarys(az):
    rng = np.random.default_rng(11)
    accepted = 0
    for W, H in SIZES[:2]:
        for p in _project_points(az[0], az[1], rng):
            a, b, c = _three_projects(*p, az[0], az[1], W, H)
            assert a == b == c, (p, az, W, H, a, b, c)
            accepted += a is not None
    if az[1] - az[0] == 360.0:
        # reference horizonator_x_from_az: an exact 2 pi span unwraps to zero and refuses every point
        assert accepted == 0
    if az == (-179.9, 179.95):
        assert accepted > 200


def test_project_at_elevation_ndc_exactly_plus_and_minus_one():
    """a point due north as high above (below) the viewer as it is far: atan2 = pi/4; with aspect * 2 / span = 4 / pi the
    elevation lands on the image's edge, el_ndc = +-1 exactly where the rounding allows - accepted, y = -0.5 / H - 0.5 -
    and a hair beyond it elsewhere - refused.  All three statements agree on every candidate"""
    hits = {-0.5: 0, 1.0: 0}
    for W, H, span in ((64, 64, 90.0), (128, 64, 180.0), (64, 128, 45.0)):
        for az0 in np.arange(-40.0, -1.0, 1.5):
            for dlat_deg in (0.01, 0.013, 0.02, 0.05):
                north = ((LAT + dlat_deg) - LAT) * na.M_PI / 180. * float(np.float32(6371000.0))
                for sign in (1.0, -1.0):
                    a, b, c = _three_projects(LAT + dlat_deg, LON, sign * north, az0, az0 + span, W, H, ele_viewer=0.0)
                    assert a == b == c
                    if a is not None and a[1] == -0.5:
                        hits[-0.5] += 1
                    if a is not None and a[1] == H - 0.5:
                        hits[1.0] += 1
    assert hits[-0.5] > 0 and hits[1.0] > 0, hits


@pytest.mark.parametrize("az", VIEWS, ids=lambda a: "%g..%g" % a)
def test_unproject_is_the_oracles_and_the_librarys(az):
    lib, orc = _lib.load(), oracle.load()
    rng = np.random.default_rng(12)
    for W, H in SIZES[:3]:
        px = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(60)] + \
             [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (-1, -1), (W, H)]
        for x, y in px:
            r = float(rng.uniform(200, 50000))
            for enh, en in ((r, -1.0), (-1.0, r), (r, r), (-1.0, -1.0), (0.0, r), (r, 0.0), (float("nan"), r), (r, float("nan")),
                            (float(np.float32(r)), -1.0)):
                ok, la, lo = na.unproject(x, y, enh, en, LAT, COSL, LON, az[0], az[1], W, H)
                for fn in (orc.orc_unproject, lib.horizonator_unproject):
                    fla, flo = C.c_float(), C.c_float()
                    fok = fn(C.byref(fla), C.byref(flo), x, y, enh, en, LAT, COSL, LON, az[0], az[1], W, H)
                    assert bool(fok) == bool(ok), (x, y, enh, en)
                    if ok:
                        assert np.array_equal(np.array([la, lo], np.float32), np.array([fla.value, flo.value], np.float32),
                                              equal_nan=True), (x, y, enh, en, az, W, H)
    # arrays go through the same statements as scalars
    xs, ys = np.arange(W), np.arange(W) % H
    rr = rng.uniform(200, 50000, W)
    ok, la, lo = na.unproject(xs, ys, rr, -1.0, LAT, COSL, LON, az[0], az[1], W, H)
    for k in (0, 1, W // 3, W - 1):
        ok1, la1, lo1 = na.unproject(int(xs[k]), int(ys[k]), float(rr[k]), -1.0, LAT, COSL, LON, az[0], az[1], W, H)
        assert ok[k] == ok1 and la[k].tobytes() == la1.tobytes() and lo[k].tobytes() == lo1.tobytes()


def _same_poi(a, b, what):
    for k, name in enumerate(("visible", "label_x", "label_y")):
        assert np.array_equal(a[k], b[k]), f"{what}: {name} differs at {np.flatnonzero(a[k] != b[k])[:5]}"


def _same_link(a, b, what):
    assert a[0].shape == b[0].shape, what
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True), what


@pytest.mark.parametrize("key", ac.KEYS)
def test_passes_are_the_oracles_on_the_zoo(key):
    """link_cells and poi_visibility on the oracle's range image of every input the GPU tests use"""
    c = ac.INPUTS[key]
    v, R = c["view"], ac.want_render(key)["ranges"]
    for cw, ch, cut in ac.cells_and_cuts(c["W"], c["H"]):
        _same_link(ac.want_link(key, cw, ch, cut),
                   oracle.link_cells(R, cw, ch, cut, c["lat"], c["lon"], v["az_deg0"], v["az_deg1"]), f"{key} {cw}x{ch} cut {cut}")
    pois = ac.ground_pois(key)[::7]
    rng = np.random.default_rng(5)
    span = c["N"] * float(v["deg_per_cell"])
    pois = np.concatenate([pois, np.stack([c["lat"] + rng.uniform(-span, span, 300), c["lon"] + rng.uniform(-span, span, 300),
                                           rng.uniform(0, 9000, 300)], 1).astype(np.float32)])
    for cut in ac.cuts_poi(c["H"]):
        _same_poi(na.poi_visibility(R, pois, cut, c["lat"], c["lon"], v["az_deg0"], v["az_deg1"], c["ele"]),
                  oracle.poi_visibility(R, pois, cut, c["lat"], c["lon"], v["az_deg0"], v["az_deg1"], c["ele"]), f"{key} cut {cut}")


def test_link_tables_are_what_unproject_evaluates():
    """the tables hz_hip_link_cells takes from its caller hold exactly the sinf / cosf / cos that horizonator_unproject
    would evaluate for the cell's centre pixel"""
    W, H = 333, 111
    for az0, az1 in VIEWS:
        nx, ny, s, c, e = na.link_tables(W, H, az0, az1, 7, 31, 5)
        assert (nx, ny) == (len(range(0, W - 7, 7)), len(range(0, H - 5 - 31, 31))) and s.dtype == np.float32 and e.dtype == np.float64
        # range_en = 1: n is cosf(az), e is sinf(az), and lat - lat_viewer is n / Rearth / pi * 180
        ok, la, lo = na.unproject(np.arange(nx) * 7 + 3, 0, -1.0, 1.0, 0.0, 1.0, 0.0, az0, az1, W, H)
        R = np.float32(6371000.0)
        assert np.array_equal(la, ((c / R).astype(np.float64) / np.float64(na.M_PI) * np.float64(180.)).astype(np.float32))
        assert np.array_equal(lo, ((s / R).astype(np.float64) / np.float64(na.M_PI) * np.float64(180.)).astype(np.float32))


def _hand_image():
    """40 x 30: eight rows of sky, below them ground whose range falls by 900 m a row; column 5 has a sky hole, column 10
    one row farther than the row above it, column 15 a NaN, column 20 is plain"""
    R = np.full((30, 40), -1.0, np.float32)
    base = (30000.0 - 900.0 * np.arange(30)).astype(np.float32)
    R[8:] = base[8:, None]
    R[14:16, 5] = -1.0
    R[13, 10] = base[11]
    R[16, 15] = np.nan
    return R, base


def test_search_on_a_hand_made_image():
    R, base = _hand_image()
    proj = np.array([
        (5.0, 13.0, base[16]),                          # rows 7..18: sky, falling errors, the hole skipped, row 16 exact
        (10.0, 12.0, base[15]),                         # row 13 is worse than row 12: given up, though row 15 is exact
        (15.0, 13.0, base[16]),                         # row 16 is NaN: given up at row 15, 900 m off
        (15.0, 13.0, base[15]),                         # row 15 exact, found before the NaN
        (20.0, 18.0, (float(base[12]) + float(base[13])) / 2),     # rows 12 and 13 both 450 m off: the first stays
        (20.0, 2.0, base[8]),                           # window rows -4..7 all sky or above the image
        (20.0, 28.5, base[29]),                         # round(28.5) = 29: rows 23..29, row 29 exact at fuzz 0, row 30 outside, then height_out
        (39.5, 20.0, base[20]),                         # round(39.5) = 40 = W
    ], np.float64)
    vis, x, y, tags = na.poi_search(R, 30, proj)
    assert vis.tolist() == [1, 0, 0, 1, 1, 0, 1, 0]
    assert y.tolist() == [16.0, 0.0, 0.0, 15.0, 12.0, 0.0, 28.5, 0.0] and x.tolist() == [5.0, 0.0, 0.0, 15.0, 20.0, 0.0, 20.0, 0.0]
    assert {"sky_then_terrain"} <= tags[0] and {"break_decided", "rejected"} <= tags[1] and {"nan", "rejected"} <= tags[2]
    assert "nan" in tags[3] and {"tie", "fuzz-6"} <= tags[4] and {"clip_top", "rejected"} <= tags[5]
    assert {"y_half", "row_outside", "height_out"} <= tags[6] and {"col_outside", "rejected"} <= tags[7]
    # a cut-off of 4 rows takes row 26 and below out of reach of a crosshair at 28.5
    assert na.poi_search(R, 26, proj)[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0]


def test_passes_are_the_oracles_on_the_hand_made_image():
    R, _ = _hand_image()
    H, W = R.shape
    rng = np.random.default_rng(8)
    n = 4000
    # points at the ranges the image holds, straight ahead of a viewer looking north through a 40 degree window
    dist = rng.uniform(300, 31000, n)
    az = np.deg2rad(rng.uniform(-25, 25, n))
    pois = np.stack([LAT + dist * np.cos(az) / 111194.9, LON + dist * np.sin(az) / 111194.9 / COSL, ELE + dist * rng.uniform(-0.12, 0.12, n)], 1)
    for cut in (0, 4, 27, 35, -4):
        got = na.poi_visibility(R, pois.astype(np.float32), cut, LAT, LON, -20.0, 20.0, ELE)
        _same_poi(got, oracle.poi_visibility(R, pois.astype(np.float32), cut, LAT, LON, -20.0, 20.0, ELE), f"cut {cut}")
        if cut == 0:
            assert 50 < got[0].sum() < n - 50
    for cw, ch, cut in ((1, 1, 0), (3, 2, 0), (7, 5, 3), (39, 29, 0), (40, 5, 0), (5, 30, 0), (14, 14, 37)):
        _same_link(na.link_cells(R, cut, cw, ch, LAT, LON, -20.0, 20.0), oracle.link_cells(R, cw, ch, cut, LAT, LON, -20.0, 20.0), (cw, ch, cut))
    la, _ = na.link_cells(R, 0, 1, 1, LAT, LON, -20.0, 20.0)
    assert la.shape == (29, 39) and np.isnan(la[:8]).all() and np.isnan(la[14:16, 5]).all() and np.isnan(la[16, 15])
    assert not np.isnan(np.delete(la[8:], [5, 15], axis=1)).any()


# ---- the conditions the GPU tests' inputs have to meet ------------------------------------------------------------------

def test_crafted_points_take_every_way_through_the_search():
    """over the exact inputs of tests/test_gpu_annot_zoo.py - every input, every cut-off, the whole list of points - each
    tag of naive_annot.TAGS is met, and `y_half` also by a crosshair below -0.5 that is searched (where round() and
    floor(y + .5) give different rows)"""
    seen = set()
    half_below = 0
    for key in ac.KEYS:
        p = ac.proj_list(key)
        for cut in ac.cuts_poi(ac.INPUTS[key]["H"]):
            vis, _, _, tags = ac.want_poi(key, cut)
            for t in tags:
                seen |= t
            half_below += sum(1 for k in np.flatnonzero(vis) if p[k, 1] < -0.5 and "y_half" in tags[k])
    assert seen == set(na.TAGS), set(na.TAGS) - seen
    assert half_below > 0


# neither sky nor ground to tell apart: no terrain at all, terrain everywhere, terrain whose every range is NaN (zfar = inf)
LINK_EXEMPT = ("flat0-z005", "checker-zoom12", "spikes-inf_far")


@pytest.mark.parametrize("key", ac.KEYS)
def test_link_cells_inputs_have_both_sky_and_ground(key):
    c = ac.INPUTS[key]
    for cw, ch in ((14, 14), (1, 1), (7, 31)):
        la, lo = ac.want_link(key, cw, ch, 0)
        assert la.size > 1 and np.array_equal(np.isnan(la), np.isnan(lo))
        if c["name"] in LINK_EXEMPT:
            assert np.isnan(la).all() or not np.isnan(la).any()
        else:
            assert np.isnan(la).any() and (~np.isnan(la)).any(), (key, cw, ch)
