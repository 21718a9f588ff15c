"""Full-size scenes against the reference: tests/golden/render_checksums.json
holds the SHA-256 of what the reference's own shaders drew on Mesa llvmpipe for
BASELINE's 3x3-tile / 8000x2000 and 7x7-tile / 16000x4000 panoramas and for other views at those
sizes (a 45 degree zoom, a viewer 4.5 km up, a moved viewpoint with a 240 degree span; made by
oracle/make_golden.py; the images themselves are too large to commit).  Equal
hashes = every byte of the BGR image and of the 24-bit depth is the reference's."""
import hashlib
import json
import os

import numpy as np
import pytest

import hzutil
import oracle

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "render_checksums.json")))
# BASELINE.json configs[3]: sixteen of the 256 viewpoints over the 5x5-tile window, same provenance
BATCH = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "batch_checksums.json")))


def _dem_differs():
    """The hashes pin reference renders of ONE synthetic DEM.  tools/demgen.c rounds sums of
    libm sines to integers, so another libm could in principle move a sample: the committed
    hashes then say nothing.  Where the HIP path is under test (a GPU is present) that must
    not pass silently: it fails; on a CPU-only machine the oracle tests skip."""
    msg = "the synthetic DEM generator produced different tiles on this machine (libm?): the reference hashes cannot be used"
    if hzutil.hip_available():
        pytest.fail(msg)
    pytest.skip(msg)


def _inputs(c):
    d = hzutil.dem_dir_for(c["lat"], c["lon"], c["R"])
    od = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"])
    m = od.mosaic()
    if hashlib.sha256(m.tobytes()).hexdigest() != c["mosaic_sha256"]:
        _dem_differs()
    v = od.view(c.get("view_lat", c["lat"]), c.get("view_lon", c["lon"]), c["W"], c["H"], c["az_deg0"], c["az_deg1"],
                **dict(dict(znear=c["znear"], zfar=c["zfar"]), **c.get("kw", {})))
    assert {k: float(np.float32(x)) for k, x in v.as_dict().items()} == c["view"]
    return m, v


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", ["cfg2_3x3_8000x2000", "cfg2_3x3_8000x2000_moved_wide"])
def test_oracle_cfg2_is_the_reference_render(name):
    c = GOLD[name]
    m, v = _inputs(c)
    o = oracle.render(m, v, c["W"], c["H"], want=("bgr", "z24"))
    assert _sha(o["bgr"]) == c["bgr_sha256"]
    assert _sha(o["z24"]) == c["z24_sha256"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLD))
def test_hip_full_size_is_the_reference_render(name):
    """the benchmark workload itself: HIP output == reference-on-llvmpipe, byte for byte"""
    c = GOLD[name]
    m, v = _inputs(c)
    hip = hzutil.hip_render(m, v, c["W"], c["H"])
    assert _sha(hip["bgr"]) == c["bgr_sha256"]
    assert _sha(hip["z24"]) == c["z24_sha256"]
    assert abs(float((hip["index"] >= 0).mean()) - c["terrain_fraction"]) < 1e-12


@pytest.mark.gpu
def test_hip_cfg3_equals_oracle_on_every_output():
    """16000x4000 over the 7x7 mosaic: index map and ranges too (the reference
    has no index map; ranges are its CPU conversion of the depth)"""
    c = GOLD["cfg3_7x7_16000x4000"]
    m, v = _inputs(c)
    hip = hzutil.hip_render(m, v, c["W"], c["H"])
    orc = oracle.render(m, v, c["W"], c["H"])
    hzutil.assert_same_render(hip, orc, "cfg3 full size")


def _batch_inputs():
    c = BATCH
    d = hzutil.dem_dir_for(c["lat"], c["lon"], c["R"])
    od = oracle.Dem(c["lat"], c["lon"], d, radius_cells=c["R"])
    if hashlib.sha256(od.mosaic().tobytes()).hexdigest() != c["mosaic_sha256"]:
        _dem_differs()
    return d, od


def test_oracle_batch_viewpoint_is_the_reference_render():
    """a moved viewpoint inside the 5x5-tile window (pins the host-side derivation of
    the viewer cell / height for viewpoints other than the window's centre)"""
    c = BATCH
    d, od = _batch_inputs()
    g = c["viewpoints"]["37"]
    v = od.view(g["lat"], g["lon"], c["W"], c["H"], c["az_deg0"], c["az_deg1"], znear=c["znear"], zfar=c["zfar"])
    assert {k: float(np.float32(x)) for k, x in v.as_dict().items()} == g["view"]
    o = oracle.render(od.mosaic(), v, c["W"], c["H"], want=("bgr", "z24"))
    assert _sha(o["bgr"]) == g["bgr_sha256"] and _sha(o["z24"]) == g["z24_sha256"]


@pytest.mark.gpu
def test_hip_viewpoint_batch_is_the_reference_render():
    """BASELINE.json configs[3] at full size through the product API: one context over the
    5x5-tile window, horizonator_amd_render_batch() over lattice viewpoints; every byte of
    every image is what the reference's shaders drew on llvmpipe for that viewpoint"""
    import torch
    import horizonator_amd
    c = BATCH
    d, od = _batch_inputs()
    W, H = c["W"], c["H"]
    lats, lons = hzutil.viewpoint_lattice(c["lat"], c["lon"])
    pick = sorted(int(k) for k in c["viewpoints"])
    h = horizonator_amd.horizonator(c["lat"], c["lon"], W, H, dir_dems=d, render_radius_cells=c["R"])
    try:
        h.set_view(c["az_deg0"], c["az_deg1"], znear=c["znear"], zfar=c["zfar"])
        d_img = torch.empty((len(pick), H, W, 3), dtype=torch.uint8, device="cuda:0")
        z = h.render_batch(lats[pick], lons[pick], d_img.data_ptr(), 0)
        h.sync()
        img = d_img.cpu().numpy()
        for k, vp in enumerate(pick):
            g = c["viewpoints"][str(vp)]
            assert np.float32(g["view"]["viewer_z"]) == z[k]
            assert _sha(img[k]) == g["bgr_sha256"], vp
        # depth of one of them through the one-at-a-time API
        g = c["viewpoints"][str(pick[-1])]
        _, _, index, z24 = h.render_full(c["az_deg0"], c["az_deg1"], lat=g["lat"], lon=g["lon"],
                                         znear=c["znear"], zfar=c["zfar"])
        assert _sha(z24) == g["z24_sha256"]
        assert abs(float((index >= 0).mean()) - g["terrain_fraction"]) < 1e-12
    finally:
        h.close()


@pytest.mark.gpu
def test_hip_all_256_viewpoints_batch_equals_one_render_each():
    """BASELINE.json configs[3] whole: the 16x16 lattice of viewpoints over the 5x5-tile window,
    8000x2000 each, queued as ONE batch without a wait in between - and every image and range
    image of the batch equal to what the same viewpoint gives when rendered on its own and
    waited for (the sixteen pinned viewpoints are also hashed against the reference above)"""
    import torch
    import horizonator_amd
    c = BATCH
    d, od = _batch_inputs()
    W, H = c["W"], c["H"]
    lats, lons = hzutil.viewpoint_lattice(c["lat"], c["lon"])
    n = len(lats)
    assert n == 256
    h = horizonator_amd.horizonator(c["lat"], c["lon"], W, H, dir_dems=d, render_radius_cells=c["R"])
    try:
        h.set_view(c["az_deg0"], c["az_deg1"], znear=c["znear"], zfar=c["zfar"])
        dev = torch.device("cuda:0")
        d_img = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        d_rng = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        z = h.render_batch(lats, lons, d_img.data_ptr(), d_rng.data_ptr())
        h.sync()
        one_img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        one_rng = torch.empty((H, W), dtype=torch.float32, device=dev)
        for k in range(n):
            h.set_view(c["az_deg0"], c["az_deg1"], lat=float(lats[k]), lon=float(lons[k]), znear=c["znear"], zfar=c["zfar"])
            assert np.float32(h.view()["viewer_z"]) == z[k], k
            h.render_device(one_img.data_ptr(), one_rng.data_ptr())
            h.sync()
            assert torch.equal(one_img, d_img[k]), f"viewpoint {k}: image"
            assert torch.equal(one_rng, d_rng[k]), f"viewpoint {k}: ranges"
        for vp in sorted(int(k) for k in c["viewpoints"]):
            assert _sha(d_img[vp].cpu().numpy()) == c["viewpoints"][str(vp)]["bgr_sha256"], vp
    finally:
        h.close()


def _api_render(lat, lon, R, W, H, az0, az1, view_lat, view_lon, znear, zfar, viewer_z=None):
    """one render through the reference's own API surface (include/horizonator.h: init, pan_zoom, move, set_zextents,
    then the build's four-output render): hz_host.c's uniform derivation and fill_tanel are in the path, nothing
    computed by the oracle is handed to the library"""
    import ctypes as C
    import horizonator_amd
    d = hzutil.dem_dir_for(lat, lon, R)
    h = horizonator_amd.horizonator(lat, lon, W, H, dir_dems=d, render_radius_cells=R)
    try:
        ctx, lib = C.byref(h._ctx), h._lib
        vz = C.c_float(-1.0 if viewer_z is None else viewer_z)
        assert lib.horizonator_pan_zoom(ctx, az0, az1)
        assert lib.horizonator_move(ctx, C.byref(vz), view_lat, view_lon)
        assert lib.horizonator_set_zextents(ctx, znear, zfar, znear, zfar)
        image = np.empty((H, W, 3), np.uint8); ranges = np.empty((H, W), np.float32)
        index = np.empty((H, W), np.int32); z24 = np.empty((H, W), np.uint32)
        assert lib.horizonator_amd_render(ctx, image.ctypes.data, ranges.ctypes.data, index.ctypes.data, z24.ctypes.data)
        # ... and the reference's own two-output call gives the same two
        image2 = np.empty((H, W, 3), np.uint8); ranges2 = np.empty((H, W), np.float32)
        assert lib.horizonator_render_offscreen(ctx, image2.ctypes.data, ranges2.ctypes.data)
        assert np.array_equal(image, image2) and np.array_equal(ranges, ranges2)
        return image, ranges, index, z24, h.view()
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLD))
def test_api_full_size_is_the_reference_render(name):
    """every full-size scene once through the API (the shim-level tests above feed the kernels
    oracle-computed uniforms and tanel tables; here the library derives both itself)"""
    c = GOLD[name]
    _inputs(c)                                      # (the DEM is the one the hashes were made on)
    image, ranges, index, z24, v = _api_render(c["lat"], c["lon"], c["R"], c["W"], c["H"], c["az_deg0"], c["az_deg1"],
                                               c["view_lat"], c["view_lon"], c["znear"], c["zfar"], c.get("kw", {}).get("viewer_z"))
    assert {k: float(np.float32(v[k])) for k in c["view"]} == c["view"]
    assert _sha(image) == c["bgr_sha256"]
    assert _sha(z24) == c["z24_sha256"]
    assert abs(float((index >= 0).mean()) - c["terrain_fraction"]) < 1e-12
    # the ranges: the naive restatement of reference horizonator-lib.c:1006-1047 on a band of rows around the horizon
    import naive_host_math as nv
    H, W = c["H"], c["W"]
    rows = [r for r in (0, H // 2 - 1, H // 2, H - 1) if 0 <= r < H]
    cols = slice(0, W, max(1, W // 97))
    for yo in rows:
        row = H - 1 - yo
        y = row if row < H - H // 2 else H - 1 - row
        t = nv.get_tanel(y, W, H, v["az_deg0"], v["az_deg1"])
        for x in range(W)[cols]:
            zi = z24[yo, x]
            if zi == 0xFFFFFF:
                assert ranges[yo, x] == -1.0
                continue
            depth = np.float32(np.float64(zi) / np.float64(16777215.0))
            length_en = depth * (np.float32(v["zfar"]) - np.float32(v["znear"])) + np.float32(v["znear"])
            assert ranges[yo, x] == nv.hypotf(length_en, np.float32(t) * length_en), (yo, x)


@pytest.mark.gpu
def test_api_cfg1_is_the_reference_render():
    """BASELINE.json configs[0] (one tile, 2000x500) through the API against the committed llvmpipe render"""
    g = hzutil.load_render_fixture(os.path.join(os.path.dirname(__file__), "golden", "render_G3_cfg1.npz"))
    W, H = int(g["W"]), int(g["H"])
    image, ranges, index, z24, v = _api_render(hzutil.VIEW_LAT, hzutil.VIEW_LON, 600, W, H, -180.0, 180.0,
                                               hzutil.VIEW_LAT, hzutil.VIEW_LON, 100.0, 40000.0)
    for k in oracle.VIEW_FIELDS:
        assert np.float32(v[k]) == np.float32(g["u_" + k]), k
    assert np.array_equal(image, g["bgr"])
    orc = oracle.render(g["mosaic"], oracle.make_view(**{k: float(g["u_" + k]) for k in oracle.VIEW_FIELDS}), W, H)
    hzutil.assert_same_render(dict(bgr=image, ranges=ranges, index=index, z24=z24), orc, "cfg1 through the API")
