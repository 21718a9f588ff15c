"""The strips of the multi-GPU gather against their published format.  tests/test_gpu_parity.py sends a draw through
packer and unpacker and compares what comes out with a plain render: that holds the two kernels to each other.  Here each
is held to include/hz_hip.h alone, through the NumPy encoder and decoder of tests/strip_format.py:

  (a) hz_hip_pack / hz_hip_pack_sparse of draws of the terrain zoo: the words they write against the words the format
      prescribes for the CPU oracle's image of the same view;
  (b) hz_hip_resolve_packed / hz_hip_resolve_sparse / hz_hip_resolve_sparse_strips on strips the device never wrote -
      encoded on the host from hand-made terrain masks, depths and shades - against the conversion of
      tests/strip_format.py (held to tests/naive_host_math.py by tests/test_strip_format.py);
  (c) the calls' argument checks.

Every strip handed to the device is well formed: the kernels trust what they are given.

Which branches of hz_k_resolve.h / hz_convert.cpp the cases are there for (argued from the code):
  k_pack_sparse   rows kept in registers (up to 2048 columns): every case but the next two; `nit > SP_STEPS`, rows read twice:
                  checker-sky 2500x101; segments without a flag bit (`it >= 64`): coast-near360 16900x13; a wave without a
                  row (`yo >= H`): the heights 13, 101, 111, 203; untouched segments beside drawn ones: every case that is
                  not degenerate (asserted on the oracle's image)
  sp_step/sp_emit 16-byte loads and clears (`SW % 4 == 0`): widths 640, 256, 32, 2500, 16900, 1024, 600, 512, 300; their
                  one-word twins: widths 257, 255, 33, 31, 3, 1, 633, 509, 801, 333
  k_pack          both values of HZ_RESOLVE_CLEARS are the sparse packer's; the dense one runs with the default (clearing)
  k_resolve_sparse  12- and 16-byte stores (`out_W % 4 == 0`): the 2304-wide images, one-pixel stores: the 2303-wide ones and
                  the threads at a strip's ragged ends; a second lap of 1024 columns and the alternating set of wave counts:
                  1025 and 2100 columns, and 1023 / 1024 columns that do not start on a multiple of four; `bgr == NULL`,
                  `ranges == NULL`: the outputs asked for; strips of no columns and the loop over launches of HZ_MAX_STRIPS
                  strips: the call with nineteen
  k_resolve_packed  `stride > ncols`, either output alone"""
import ctypes as C
import functools

import numpy as np
import pytest

import hzutil
import oracle
import strip_format as sf

pytestmark = pytest.mark.gpu

SKY = sf.Z24_SKY
SENT = 0x5EA15EA1               # what every device buffer holds before a call
GUARD = 4099                    # words behind the last word a call may write
ZOO = {c["name"]: c for c in hzutil.zoo_cases()}


def _hzview(v):
    out = hzutil.hzlib.View()
    for name, _ in hzutil.hzlib.View._fields_:
        setattr(out, name, getattr(v, name))
    return out


def _err(lib):
    return (lib.hz_hip_last_error() or b"").decode()


def _words(t):
    """a torch int32 tensor as uint32 on the host"""
    return t.cpu().numpy().view(np.uint32)


# ---- (a) the packers ---------------------------------------------------------

# name: the zoo case whose ground and view are drawn, at W x H (the view's aspect follows); sectors: (first column, width,
# mask words beyond the minimum); other: the zoo case (same mosaic size) drawn behind each pack on the same context.
# fraction: the CPU oracle's terrain fraction of the whole W x H image, to four places (asserted in _reference()).
_SECTORS_640 = [(0, 640, 0), (4, 256, 2), (131, 256, 0), (129, 257, 1), (384, 255, 0), (200, 33, 0), (333, 32, 3), (64, 31, 0),
                (401, 3, 0), (500, 1, 1), (321, 1, 0)]
PACK_CASES = [
    dict(name="cliff-near360", W=640, H=160, sectors=_SECTORS_640, other="flat0-near360", fraction=0.3086),
    # rows of more than 2048 pixels: k_pack_sparse reads them twice; 101 rows: one wave of the last workgroup has none
    dict(name="checker-sky", W=2500, H=101, sectors=[(0, 2500, 0)], other="flat0-sky", fraction=0.2834),
    # rows of more than 16384 pixels: segments beyond the 64 that have a flag bit
    dict(name="coast-near360", W=16900, H=13, sectors=[(0, 16900, 2)], other="cliff-near360", fraction=0.5711),
    # a patch seen from 9000 m: most segments untouched
    dict(name="flat0-sky", W=1024, H=256, sectors=[(0, 1024, 5), (250, 600, 0)], other="checker-sky", fraction=0.2121),
    dict(name="coast-sky", W=1024, H=256, sectors=[(0, 1024, 0), (515, 509, 1)], other="cliff-sky", fraction=0.2146),
    # no far clip: z24 = 0 on all of the terrain
    dict(name="spikes-inf_far", W=640, H=160, sectors=[(0, 640, 0), (2, 633, 0)], other="flat0-near360", fraction=0.2941),
    dict(name="cliff-arctic90", W=801, H=203, sectors=[(0, 801, 0), (96, 512, 4)], other="plateau-arctic90", fraction=0.5016),
    # the reference draws nothing (T = 0) / everything (every row all terrain): exempt from the conditions on the fraction
    dict(name="flat0-z005", W=512, H=128, sectors=[(0, 512, 0), (7, 300, 1)], other="checker-near360", fraction=0.0, degenerate=True),
    dict(name="checker-zoom12", W=333, H=111, sectors=[(0, 333, 0), (40, 256, 1)], other="flat0-zoom12", fraction=1.0, degenerate=True),
]


def _view_at(name, W, H):
    v = dict(ZOO[name]["view"])
    v["aspect"] = float(np.float32(W) / np.float32(H))
    return oracle.make_view(**v)


@functools.lru_cache(maxsize=None)
def _oracle_image(name, W, H):
    """the CPU oracle's whole image of zoo case `name` at W x H: computed once, shared, never written to"""
    c = ZOO[name]
    out = oracle.render(hzutil.zoo_mosaic(c["family"], c["N"]), _view_at(name, W, H), W, H)
    for a in out.values():
        a.setflags(write=False)
    return out


def sky_segment_beside_terrain(terrain):
    """rows in which a whole 256-pixel segment (counted from the image's first column, as a whole-image draw has them)
    holds no terrain while a neighbouring segment holds some"""
    H, W = terrain.shape
    nseg = (W + 255) // 256
    has = np.stack([terrain[:, k * 256:(k + 1) * 256].any(axis=1) for k in range(nseg)], axis=1)
    rows = np.zeros(H, bool)
    for k in range(W // 256):                   # the whole segments
        for n in (k - 1, k + 1):
            if 0 <= n < nseg:
                rows |= ~has[:, k] & has[:, n]
    return int(rows.sum())


def _reference(case):
    """the oracle's image of a case, with what the case list promises about it"""
    img = _oracle_image(case["name"], case["W"], case["H"])
    terrain = img["z24"] != SKY
    f = float(terrain.mean())
    assert round(f, 4) == case["fraction"], (case["name"], f)
    if case.get("degenerate"):
        assert f in (0.0, 1.0)
    else:
        assert 0.05 < f < 0.95, (case["name"], f)
        assert sky_segment_beside_terrain(terrain) >= 1, case["name"]
    return img


class _Draws:
    """one context for a case: its ground and the ground drawn behind each pack, in turn"""

    def __init__(self, case):
        import torch
        self.torch = torch
        self.case = case
        self.W, self.H = case["W"], case["H"]
        c, o = ZOO[case["name"]], ZOO[case["other"]]
        assert c["N"] == o["N"] and c["family"] != o["family"]
        self.mosaic = hzutil.zoo_mosaic(c["family"], c["N"])
        self.other_mosaic = hzutil.zoo_mosaic(o["family"], o["N"])
        self.view = _view_at(case["name"], self.W, self.H)
        self.other_view = _view_at(case["other"], self.W, self.H)
        self.want = _reference(case)
        self.other_want = _oracle_image(case["other"], self.W, self.H)
        self.dev = hzutil.HipDev(self.mosaic, self.W, self.H)

    def close(self):
        self.dev.close()

    def draw(self, c0, n):
        """the case's view of its ground into columns [c0, c0+n), queued; the oracle's z24 and shade of those columns"""
        lib, dev = self.dev.lib, self.dev.dev
        assert lib.hz_hip_upload_mosaic(dev, self.mosaic.ctypes.data) == 0
        assert lib.hz_hip_set_sector(dev, c0, c0 + n) == 0
        assert lib.hz_hip_draw(dev, C.byref(_hzview(self.view))) == 0, _err(lib)
        return self.want["z24"][:, c0:c0 + n], self.want["bgr"][:, c0:c0 + n, 2]

    def draw_other(self, c0, n, what):
        """the other ground on the framebuffer that comes next, all four outputs against the oracle"""
        assert self.dev.lib.hz_hip_upload_mosaic(self.dev.dev, self.other_mosaic.ctypes.data) == 0
        got = self.dev.render(self.other_view, c0, c0 + n)
        hzutil.assert_same_render(got, {k: a[:, c0:c0 + n] for k, a in self.other_want.items()},
                                  f"{self.case['other']} behind {what}")

    def buffer(self, nwords):
        t = self.torch.full((nwords + GUARD,), SENT, dtype=self.torch.int32, device="cuda:0")
        self.torch.cuda.synchronize()
        return t


def check_dense(got, z24, red, what):
    H, SW = z24.shape
    want = sf.pack_dense(z24, red)
    body = got[:H * SW].reshape(H, SW)
    terrain = z24 != SKY
    assert np.array_equal(body[terrain], want[terrain]), f"{what}: terrain words"
    # (the header states the upper 24 bits of a sky word, not its low byte)
    assert np.array_equal(body[~terrain] >> 8, want[~terrain] >> 8), f"{what}: sky words"
    assert (got[H * SW:] == SENT).all(), f"{what}: words written behind the strip"


def check_sparse(got, z24, red, ms, what):
    H, SW = z24.shape
    hdr, mw = sf.header_words(H, ms), sf.mask_words(SW)
    terrain = z24 != SKY
    count = terrain.sum(axis=1)
    T = int(count.sum())
    assert int(got[0]) == T, f"{what}: [0] = {int(got[0])}, the oracle has {T} terrain pixels"
    base = got[1:1 + H].astype(np.int64)
    # the rows as they lie in the data: the format leaves their order to the packer, the helper takes it over
    order = np.argsort(base, kind="stable")
    want = sf.pack_sparse(z24, red, ms, order)
    assert int(want[0]) == T and want.size == hdr + T
    gm, wm = got[1 + H:hdr].reshape(H, ms), want[1 + H:hdr].reshape(H, ms)
    bad = np.argwhere(gm[:, :mw] != wm[:, :mw])
    assert not len(bad), f"{what}: mask word {bad[0][1]} of row {bad[0][0]} is {gm[tuple(bad[0])]:#x}, not {wm[tuple(bad[0])]:#x}"
    if SW % 32:
        assert not (gm[:, mw - 1] >> np.uint32(SW % 32)).any(), f"{what}: mask bits beyond the last column"
    # [row_base, row_base + count) of the rows with terrain tile [0, T): they equal the bases of a gapless layout in their
    # own order; a row without terrain has an empty span, anywhere in [0, T]
    full = count > 0
    assert np.array_equal(base[full], want[1:1 + H].astype(np.int64)[full]), f"{what}: the rows' spans do not tile [0, T)"
    assert ((base >= 0) & (base <= T)).all(), f"{what}: row_base beyond T"
    bad = np.flatnonzero(got[hdr:hdr + T] != want[hdr:])
    assert not len(bad), f"{what}: data word {bad[0]} is {got[hdr + bad[0]]:#x}, not {want[hdr + bad[0]]:#x}"
    assert (got[hdr + H * SW:] == SENT).all(), f"{what}: words written behind the strip's room"


@pytest.fixture
def draws(request):
    made = []

    def make(case):
        made.append(_Draws(case))
        return made[-1]
    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: c["name"])
def test_dense_packer_writes_the_words_of_the_header(case, draws):
    d = draws(case)
    lib, dev = d.dev.lib, d.dev.dev
    for c0, n, _ in case["sectors"]:
        what = f"{case['name']} {d.W}x{d.H} columns [{c0},{c0 + n})"
        z24, red = d.draw(c0, n)
        buf = d.buffer(d.H * n)
        assert lib.hz_hip_pack(dev, buf.data_ptr()) == 0, _err(lib)
        assert lib.hz_hip_sync(dev) == 0
        check_dense(_words(buf), z24, red, what)
    d.draw_other(c0, n, what)


@pytest.mark.parametrize("clears", ["1", "0"])
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: c["name"])
def test_sparse_packer_writes_the_stream_of_the_header(case, clears, draws, monkeypatch):
    """... and, where the packer is the draw's last reader (HZ_RESOLVE_CLEARS=1), leaves the framebuffer as glClear would:
    a draw of another ground follows each pack, four times, so that each framebuffer of the ring (HZ_NFB = 3) has been
    cleaned by a packer when a draw compared with the oracle comes to it"""
    monkeypatch.setenv("HZ_RESOLVE_CLEARS", clears)
    d = draws(case)
    lib, dev = d.dev.lib, d.dev.dev
    for c0, n, extra in case["sectors"]:
        ms = sf.mask_words(n) + extra
        for rnd in range(4 if clears == "1" else 1):
            what = f"{case['name']} {d.W}x{d.H} columns [{c0},{c0 + n}) mask_stride {ms} HZ_RESOLVE_CLEARS={clears} round {rnd}"
            z24, red = d.draw(c0, n)
            buf = d.buffer(sf.header_words(d.H, ms) + d.H * n)
            assert lib.hz_hip_pack_sparse(dev, buf.data_ptr(), ms) == 0, _err(lib)
            assert lib.hz_hip_sync(dev) == 0
            check_sparse(_words(buf), z24, red, ms, what)
            d.draw_other(c0, n, what)


# ---- (b) the unpackers -------------------------------------------------------

PATTERNS = ("none", "all", "col0", "col31", "col32", "last", "alternating", "hash97", "hash2")
WIDTHS = (1, 3, 31, 32, 33, 1023, 1024, 1025, 2100)
EXTENTS = ((100.0, 40000.0), (10.0, 5e8))
OUTPUTS = ("both", "bgr", "ranges")
BGR_SENT, RNG_SENT = 77, -7.0


def hand_made(pattern, H, n, seed):
    """(z24, red) of a hand-made strip: terrain where the pattern says, depths and shades by integer hash, with z24 = 0, 1,
    0x800000, 0xFFFFFE and red = 0, 255 among them"""
    y, x = np.mgrid[0:H, 0:n]
    terrain = {"none": lambda: np.zeros((H, n), bool), "all": lambda: np.ones((H, n), bool),
               "col0": lambda: x == 0, "col31": lambda: x == 31, "col32": lambda: x == 32, "last": lambda: x == n - 1,
               "alternating": lambda: ((x ^ y) & 1) == 1,
               "hash97": lambda: hzutil._zoo_hash(x, y, 50 + seed) % np.uint64(97) == 0,
               "hash2": lambda: (hzutil._zoo_hash(x, y, 60 + seed) & np.uint64(1)) == 1}[pattern]()
    h = hzutil._zoo_hash(x, y, 70 + seed)
    z24 = (h % np.uint64(SKY)).astype(np.uint32)                        # (never 0xFFFFFF: that is the sky's)
    red = ((h >> np.uint64(30)) & np.uint64(0xFF)).astype(np.uint8)
    at = np.flatnonzero(terrain)
    special = np.array([0, 1, 0x800000, 0xFFFFFE, 0xFFFFFE, 0], np.uint32)
    k = min(len(at), len(special))
    z24.flat[at[:k]] = special[:k]
    red.flat[at[:k]] = np.array([0, 255, 255, 0, 255, 0], np.uint8)[:k]
    z24[~terrain] = SKY
    red[~terrain] = 0
    return z24, red


def _garbage(shape, seed):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (hzutil._zoo_hash(x, y, 90 + seed) & np.uint64(0xFFFFFFFF)).astype(np.uint32) | np.uint32(1)


def sparse_strip(z24, red, ms, permuted, seed):
    """a well-formed stream for the device: rows in order or permuted in the data, garbage in the mask's padding words"""
    H, n = z24.shape
    step = next(s for s in (5, 7, 11) if H % s)                        # prime to H: a permutation of the rows
    order = (np.arange(H) * step + 3) % H if permuted else None
    s = sf.pack_sparse(z24, red, ms, order)
    mw = sf.mask_words(n)
    if ms > mw:
        s[1 + H:sf.header_words(H, ms)].reshape(H, ms)[:, mw:] = _garbage((H, ms - mw), seed)
    return s


class _Canvas:
    """a context of the output's size (nothing is ever drawn on it) and sentinel-filled full-width outputs with one row of
    guard behind them"""

    def __init__(self, W, H):
        import torch
        self.torch, self.W, self.H = torch, W, H
        self.dev = hzutil.HipDev(hzutil.zoo_mosaic("flat0", 8), W, H)
        self.lib = self.dev.lib
        self.tanel = oracle.tanel(W, H, -60.0, 300.0)
        self.fresh()

    def close(self):
        self.dev.close()

    def fresh(self):
        t = self.torch
        self.bgr = t.full((self.H + 1, self.W, 3), BGR_SENT, dtype=t.uint8, device="cuda:0")
        self.rng = t.full((self.H + 1, self.W), RNG_SENT, dtype=t.float32, device="cuda:0")
        self.want_bgr = np.full((self.H + 1, self.W, 3), BGR_SENT, np.uint8)
        self.want_rng = np.full((self.H + 1, self.W), RNG_SENT, np.float32)

    def upload(self, words):
        return self.torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to("cuda:0")

    def view(self, extents):
        v = hzutil.hzlib.View()
        v.znear, v.zfar = extents
        return v

    def expect(self, z24, red, col0, extents, outputs):
        bgr, rng = sf.convert(z24, red, self.tanel, *extents)
        n = z24.shape[1]
        if outputs != "ranges":
            self.want_bgr[:self.H, col0:col0 + n] = bgr
        if outputs != "bgr":
            self.want_rng[:self.H, col0:col0 + n] = rng
        assert not np.isnan(rng).any()

    def pointers(self, outputs):
        return (self.bgr.data_ptr() if outputs != "ranges" else None, self.rng.data_ptr() if outputs != "bgr" else None)

    def check(self, what):
        assert self.lib.hz_hip_sync(self.dev.dev) == 0
        bgr, rng = self.bgr.cpu().numpy(), self.rng.cpu().numpy()
        bad = np.argwhere(bgr != self.want_bgr)
        assert not len(bad), f"{what}: bgr differs at {len(bad)} places, first (row, column, byte) {bad[0]}: {bgr[tuple(bad[0])]} vs {self.want_bgr[tuple(bad[0])]}"
        bad = np.argwhere(rng.view(np.uint32) != self.want_rng.view(np.uint32))
        assert not len(bad), f"{what}: ranges differ at {len(bad)} places, first (row, column) {bad[0]}: {rng[tuple(bad[0])]} vs {self.want_rng[tuple(bad[0])]}"


@pytest.fixture(scope="module")
def canvas():
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = _Canvas(W, H)
        made[(W, H)].fresh()
        return made[(W, H)]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("H", [7, 64])
@pytest.mark.parametrize("W", [2304, 2303])
def test_sparse_unpacker_reads_the_stream_of_the_header(W, H, pattern, canvas):
    """every width under every terrain pattern at both image widths and heights; the start column's remainder mod 4, the
    outputs asked for, the depth extents, the order of the rows in the data, the mask stride and the entry point rotate,
    so that each value of each meets each width (over the patterns) and each pattern (over the widths)"""
    import torch
    cv = canvas(W, H)
    p = PATTERNS.index(pattern)
    for w, n in enumerate(WIDTHS):
        k = w + p
        col0 = ((W - n) // 2 // 4) * 4 + k % 4
        assert col0 % 4 == k % 4 and col0 + n <= W
        outputs, extents, permuted = OUTPUTS[k % 3], EXTENTS[(k // 3) % 2], bool((k // 2) % 2)
        ms = sf.mask_words(n) + (0, 3)[(k + w // 3) % 2]
        what = f"{pattern} {n} columns at {col0} of {W}x{H}, {outputs}, extents {extents}, rows {'permuted' if permuted else 'in order'}, mask_stride {ms}"
        z24, red = hand_made(pattern, H, n, seed=w)
        strip = cv.upload(sparse_strip(z24, red, ms, permuted, seed=k))
        cv.fresh()
        cv.expect(z24, red, col0, extents, outputs)
        torch.cuda.synchronize()
        d_bgr, d_rng = cv.pointers(outputs)
        v = cv.view(extents)
        if (k // 4) % 2:
            rc = cv.lib.hz_hip_resolve_sparse(cv.dev.dev, C.byref(v), cv.tanel.ctypes.data, strip.data_ptr(), ms, n, col0, d_bgr, d_rng)
        else:
            rc = cv.lib.hz_hip_resolve_sparse_strips(cv.dev.dev, C.byref(v), cv.tanel.ctypes.data, 1, (C.c_void_p * 1)(strip.data_ptr()), ms,
                                                     (C.c_int * 1)(n), (C.c_int * 1)(col0), d_bgr, d_rng)
        assert rc == 0, _err(cv.lib)
        cv.check(what)


def test_the_rotation_covers_what_it_claims():
    """CPU arithmetic only: every start remainder, output set, extent pair, row order, stride and entry point meets every
    width and every pattern of the test above"""
    for fixed in ("w", "p"):
        for a in range(9):
            seen = set()
            for b in range(9):
                w, p = (a, b) if fixed == "w" else (b, a)
                k = w + p
                seen |= {("col", k % 4), ("out", k % 3), ("ext", (k // 3) % 2), ("perm", (k // 2) % 2), ("ms", (k + w // 3) % 2), ("entry", (k // 4) % 2)}
            assert len(seen) == 4 + 3 + 2 + 2 + 2 + 2, (fixed, a, seen)


@pytest.mark.parametrize("outputs", OUTPUTS)
@pytest.mark.parametrize("W", [2304, 2303])
def test_nineteen_strips_in_one_call(W, outputs, canvas):
    """more strips than one launch takes (HZ_MAX_STRIPS = 16): three of them empty, the others of unequal widths, in an order
    that is not the columns', covering the image but for two gaps - whose pixels keep what they held"""
    import torch
    H = 7
    cv = canvas(W, H)
    widths = [1, 3, 31, 32, 33, 100, 257, 64, 5, 129, 200, 77, 300, 256, 400]
    gaps = {4: 5, 11: 9}                                                # columns left out behind strip 4 and strip 11
    widths.append(W - sum(widths) - sum(gaps.values()))
    assert len(widths) == 16 and widths[-1] > 256
    ms = sf.mask_words(max(widths)) + 1
    extents = EXTENTS[0]
    strips, col0 = [], 0
    for k, n in enumerate(widths):
        z24, red = hand_made(PATTERNS[(k + 1) % len(PATTERNS)], H, n, seed=k)
        cv.expect(z24, red, col0, extents, outputs)
        strips.append((cv.upload(sparse_strip(z24, red, ms, permuted=bool(k % 2), seed=k)), n, col0))
        col0 += n + gaps.get(k, 0)
    assert col0 == W
    strips = strips[5:] + strips[:5]                                    # (the table's order is the caller's)
    empty = cv.upload(sparse_strip(*hand_made("none", H, 1, 0), ms, False, 0))
    for at, tensor, c in ((0, empty, 0), (9, None, 17), (18, empty, W)):
        strips.insert(at, (tensor, 0, c))
    assert len(strips) == 19
    covered = np.zeros(W, int)
    for _, n, c in strips:
        covered[c:c + n] += 1
    assert covered.max() == 1 and (covered == 0).sum() == 14
    torch.cuda.synchronize()
    d_bgr, d_rng = cv.pointers(outputs)
    v = cv.view(extents)
    rc = cv.lib.hz_hip_resolve_sparse_strips(cv.dev.dev, C.byref(v), cv.tanel.ctypes.data, 19,
                                             (C.c_void_p * 19)(*[t.data_ptr() if t is not None else None for t, _, _ in strips]), ms,
                                             (C.c_int * 19)(*[n for _, n, _ in strips]), (C.c_int * 19)(*[c for _, _, c in strips]),
                                             d_bgr, d_rng)
    assert rc == 0, _err(cv.lib)
    cv.check(f"19 strips into {W}x{H}, {outputs}")


@pytest.mark.parametrize("H", [7, 64])
@pytest.mark.parametrize("W", [2304, 2303])
def test_dense_unpacker_reads_the_words_of_the_header(W, H, canvas):
    """packed strips with a stride beyond their columns (garbage in the padding) and anything in the low byte of a sky word"""
    import torch
    cv = canvas(W, H)
    for k, n in enumerate((1, 3, 33, 1024, 1025, 2100)):
        pattern = ("hash2", "all", "hash97", "alternating", "none", "last")[k]
        stride = n + (0, 5, 1)[k % 3]
        col0 = (W - n) // 3 // 4 * 4 + k % 4
        outputs, extents = OUTPUTS[k % 3], EXTENTS[k % 2]
        z24, red = hand_made(pattern, H, n, seed=k)
        words = _garbage((H, stride), k)
        words[:, :n] = sf.pack_dense(z24, red)
        sky = np.zeros((H, stride), bool)
        sky[:, :n] = z24 == SKY
        words[sky] |= _garbage((H, stride), k + 1)[sky] & np.uint32(0xFF)
        assert np.array_equal(words[:, :n] >> 8, z24)
        strip = cv.upload(words)
        cv.fresh()
        cv.expect(z24, red, col0, extents, outputs)
        torch.cuda.synchronize()
        d_bgr, d_rng = cv.pointers(outputs)
        v = cv.view(extents)
        assert cv.lib.hz_hip_resolve_packed(cv.dev.dev, C.byref(v), cv.tanel.ctypes.data, strip.data_ptr(), stride, n, col0,
                                            d_bgr, d_rng) == 0, _err(cv.lib)
        cv.check(f"packed {pattern} {n} columns (stride {stride}) at {col0} of {W}x{H}, {outputs}, extents {extents}")


# ---- (c) refusals ------------------------------------------------------------

def _refused(cv, rc, name):
    assert rc == -1, f"{name} was not refused"
    assert name in _err(cv.lib), _err(cv.lib)
    cv.check(f"refused {name}")


def test_unpackers_refuse_what_does_not_fit(canvas):
    import torch
    W, H = 2303, 7
    cv = canvas(W, H)
    lib, dev, tanel = cv.lib, cv.dev.dev, cv.tanel.ctypes.data
    n = 100
    ms = sf.mask_words(n)
    strip = cv.upload(sparse_strip(*hand_made("hash2", H, n, 1), ms, False, 1))
    dense = cv.upload(sf.pack_dense(*hand_made("hash2", H, n, 1)))
    torch.cuda.synchronize()
    v = cv.view(EXTENTS[0])
    bgr, rng = cv.pointers("both")
    one = lambda x, t=C.c_int: (t * 1)(x)
    ptr = strip.data_ptr()

    def strips(nstrips, table, stride, ncols, col0):
        return lib.hz_hip_resolve_sparse_strips(dev, C.byref(v), tanel, nstrips, table, stride, ncols, col0, bgr, rng)
    two = (C.c_void_p * 2)(ptr, ptr)
    _refused(cv, strips(1, one(ptr, C.c_void_p), ms - 1, one(n), one(0)), "hz_hip_resolve_sparse_strips")        # stride too small
    _refused(cv, strips(2, two, ms, (C.c_int * 2)(n, 129), (C.c_int * 2)(0, 200)), "hz_hip_resolve_sparse_strips")  # ... for the second strip
    _refused(cv, strips(1, one(ptr, C.c_void_p), ms, one(n), one(W - n + 1)), "hz_hip_resolve_sparse_strips")    # columns beyond W
    _refused(cv, strips(1, one(ptr, C.c_void_p), ms, one(n), one(-1)), "hz_hip_resolve_sparse_strips")
    _refused(cv, strips(2, two, ms, (C.c_int * 2)(n, -5), (C.c_int * 2)(0, 200)), "hz_hip_resolve_sparse_strips")  # negative ncols
    _refused(cv, strips(1, None, ms, one(n), one(0)), "hz_hip_resolve_sparse_strips")                              # no tables
    _refused(cv, strips(1, one(ptr, C.c_void_p), ms, None, one(0)), "hz_hip_resolve_sparse_strips")
    _refused(cv, strips(1, one(ptr, C.c_void_p), ms, one(n), None), "hz_hip_resolve_sparse_strips")
    _refused(cv, strips(1, one(None, C.c_void_p), ms, one(n), one(0)), "hz_hip_resolve_sparse_strips")            # no strip
    _refused(cv, strips(-1, one(ptr, C.c_void_p), ms, one(n), one(0)), "hz_hip_resolve_sparse_strips")

    def single(stride, ncols, col0):
        return lib.hz_hip_resolve_sparse(dev, C.byref(v), tanel, ptr, stride, ncols, col0, bgr, rng)
    _refused(cv, single(ms - 1, n, 0), "hz_hip_resolve_sparse")
    _refused(cv, single(ms, n, W - n + 1), "hz_hip_resolve_sparse")
    _refused(cv, single(ms, -n, 0), "hz_hip_resolve_sparse")
    _refused(cv, single(ms, 0, 0), "hz_hip_resolve_sparse")

    def packed(stride, ncols, col0):
        return lib.hz_hip_resolve_packed(dev, C.byref(v), tanel, dense.data_ptr(), stride, ncols, col0, bgr, rng)
    _refused(cv, packed(n, n, W - n + 1), "hz_hip_resolve_packed")
    _refused(cv, packed(n, n, -1), "hz_hip_resolve_packed")
    _refused(cv, packed(n, -n, 0), "hz_hip_resolve_packed")
    _refused(cv, packed(n - 1, n, 0), "hz_hip_resolve_packed")
    # the same calls are taken when nothing is wrong with them
    assert strips(2, two, ms, (C.c_int * 2)(n, n), (C.c_int * 2)(0, 200)) == 0 and single(ms, n, W - n) == 0 and packed(n, n, 400) == 0
    assert lib.hz_hip_sync(dev) == 0


def test_packers_refuse_a_small_mask_stride_and_a_textured_context():
    import torch
    c = ZOO["cliff-near360"]
    W, H = c["W"], c["H"]
    m = hzutil.zoo_mosaic(c["family"], c["N"])
    buf = torch.full((sf.header_words(H, sf.mask_words(W)) + H * W + GUARD,), SENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def refused(rc, name):
        assert rc == -1, f"{name} was not refused"
        assert name in _err(dev.lib), _err(dev.lib)
        assert dev.lib.hz_hip_sync(dev.dev) == 0
        assert (_words(buf) == SENT).all(), f"refused {name} wrote into the buffer"
    with hzutil.HipDev(m, W, H) as dev:
        lib = dev.lib
        assert lib.hz_hip_draw(dev.dev, C.byref(_hzview(oracle.make_view(**c["view"])))) == 0
        refused(lib.hz_hip_pack_sparse(dev.dev, buf.data_ptr(), sf.mask_words(W) - 1), "hz_hip_pack_sparse")
        assert lib.hz_hip_set_sector(dev.dev, 10, 75) == 0                  # 65 columns: three mask words
        refused(lib.hz_hip_pack_sparse(dev.dev, buf.data_ptr(), 2), "hz_hip_pack_sparse")
        assert lib.hz_hip_set_sector(dev.dev, 0, W) == 0
        e = hzutil.zoo_tex_entry("cliff-near360")
        dev.set_texture(*hzutil.zoo_tex_inputs(e, c))
        assert lib.hz_hip_draw(dev.dev, C.byref(_hzview(oracle.make_view(**c["view"])))) == 0
        refused(lib.hz_hip_pack(dev.dev, buf.data_ptr()), "hz_hip_pack")
        refused(lib.hz_hip_pack_sparse(dev.dev, buf.data_ptr(), sf.mask_words(W)), "hz_hip_pack_sparse")
        # ... and once the texture is off again the same draw packs
        dev.texture_off()
        assert lib.hz_hip_draw(dev.dev, C.byref(_hzview(oracle.make_view(**c["view"])))) == 0
        assert lib.hz_hip_pack_sparse(dev.dev, buf.data_ptr(), sf.mask_words(W)) == 0, _err(lib)
        assert lib.hz_hip_sync(dev.dev) == 0
        want = _oracle_image("cliff-near360", W, H)
        check_sparse(_words(buf), want["z24"], want["bgr"][..., 2], sf.mask_words(W), "after the texture was switched off")
