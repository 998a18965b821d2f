"""The pass loop's per-ray terms and the record encoder of the trace kernels against the oracle, on the project's smallest frames
(37 x 21: one partial macro tile; 64 x 48: a whole one): divTwoA from the table of rtx_unit.hpp (rtx_device.hpp: half_recip),
viewDir rescaled by the factor read beside it, and colour bytes clamped after the conversion (u8_clamped).

Every frame is compared byte for byte: records and compact pixel words in BIT_ASCII, RGB_ASCII, RGB_PIXEL and RGB_NORMALS, and the
eight floats of RTX_RENDER_VALUES, from the binned, the brute and the REFINE kernels.
  A  three spheres and a floor; the white sphere under the light saturates all three channels of some pixels past 255.
  B  two planes whose Dot(planePos - origin, n) is 1e-20 and 1e20 in size -- both outside div_cr's range [2^-60, 2^60], so the
     generic division runs -- and a sphere between them.
  C  scene A scaled by 1e18, as the scaled scenes of test_gpu_parity.py and test_gpu_unit_rescale.py: squared lengths overflow,
     every hit lies beyond the reference's initial closest distance, and the frame must say so.
  D  scene A's geometry with object colours of +inf, 3e38 and 1e30: shaded colours are +inf (the byte 255) wherever the light
     reaches and NaN (0.2 * inf + 0 * inf; the byte 0) where the diffuse term is zero, in every channel of some visible pixels
     -- what the unclamped colour hands to u8_clamped in records, compact words and the xterm-256 mapper.
  E  scene A under a camera matrix scaled by 1e25: the squared length of every ray direction overflows, the direction becomes 0
     and a = Dot(d, d) = 0 lies outside the tables' window, so half_recip's generic branch runs in every wave; nothing is hit.
(tests/test_gpu_half_recip.py holds the proofs over all 2^32 inputs; these frames check the call sites.)"""
import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

SHAPES = [(37, 21), (64, 48)]
MODES = [O.BIT_ASCII, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS]
PLANS = ["binned", "brute", "refine"]


def _scene(name):
    a_sph = np.array([[1, 10.4, 34, 6, 255, 255, 255], [-14, 2, 50, 8, 255, 40, 10], [12, -4, 35, 6, 20, 90, 255]], dtype=np.float32)
    a_pl = np.array([[0, -12, 60, 0, 1, 0, 100, 100, 100, 300, 200]], dtype=np.float32)
    if name in ("A", "E"):
        return a_sph, a_pl
    if name == "D":
        sph, pl = a_sph.copy(), a_pl.copy()
        inf = np.float32(np.inf)
        sph[:, 4:7] = [[inf, 3e38, 255], [255, inf, 1e30], [3e38, 90, inf]]
        pl[:, 6:9] = [inf, 100, 3e38]
        return sph, pl
    if name == "B":
        sph = np.array([[0, 3, 50, 4, 200, 40, 40]], dtype=np.float32)
        # the camera stands at the origin: Dot(planePos, n) = -1e-20 (a floor a hair below the eye) and -1e20 (a ceiling at
        # y = 100 whose normal is 1e18 long)
        pl = np.array([[0, -1e-20, 0, 0, 1, 0, 90, 160, 60, 3000, 250], [0, 100, 60, 0, -1e18, 0, 60, 90, 160, 3000, 250]], dtype=np.float32)
        return sph, pl
    sph, pl = a_sph.copy(), a_pl.copy()
    sph[:, :4] *= np.float32(1e18)
    pl[:, :3] *= np.float32(1e18)
    pl[:, 9:] *= np.float32(1e18)
    return sph, pl


def _params(R, shape, name):
    W, H = shape
    p = R.camera_params(W, H)
    assert tuple(p.cam_pos[:]) == (0.0, 0.0, 0.0)
    if name == "E":
        inv = np.array(p.inv_v[:], dtype=np.float32).reshape(4, 4) * np.float32(1e25)
        p = U.product_params(inv, p.cam_pos[:], W, H, p.element1, p.element2, p.cam_far)
    return p


_cache = {}


def _want(R, shape, name, mode):
    """The oracle's frame and per-pixel values of a case, computed once and shared by the plans."""
    key = (shape, name, mode)
    if key not in _cache:
        W, H = shape
        p = _params(R, shape, name)
        sph, pl = _scene(name)
        frame, px = O.render(U.oracle_params(p), O.Scene.from_arrays(sph, pl), mode, want_pixels=True)
        frame.setflags(write=False)
        px.setflags(write=False)
        _cache[key] = (frame, px.reshape(H, W))
    return _cache[key]


def _rows(R, c, p, mode, flags, S):
    import torch
    W, H = int(p.x), int(p.y)
    buf = torch.full((W * H * S,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fill is queued on torch's stream; the library renders on its own)
    c.render_rows(p, mode, 0, H, d_out=buf.data_ptr(), out_row_base=0, flags=flags)
    c.synchronize()
    return buf.cpu().numpy()


def same_bits_or_both_nan(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(64, 48)
    yield c
    c.close()


def test_the_scenes_show_what_they_are_for(R):
    for shape in SHAPES:
        W, H = shape
        _, px = _want(R, shape, "A", O.RGB_ASCII)
        hit = px["hit"] != 0
        assert int((px["color"][hit] >= 255.0).all(axis=1).sum()) >= 20      # every channel saturated (the oracle's colour is clamped)
        assert int((px["normal"][hit][:, 1] == 1.0).sum()) > 50               # ... and a floor
        _, px = _want(R, shape, "B", O.RGB_ASCII)
        hit = px["hit"] != 0
        assert int((px["distance"][hit] < 1e-10).sum()) > 100                 # the floor with the tiny numerator
        assert int((px["normal"][hit][:, 1] < -0.99).sum()) > 20              # the ceiling with the huge one
        assert int(((px["distance"][hit] > 1.0) & (px["normal"][hit][:, 1] > -0.99)).sum()) > 20   # the sphere
        _, px = _want(R, shape, "C", O.RGB_ASCII)
        assert int((px["hit"] != 0).sum()) == 0
        _, px = _want(R, shape, "D", O.RGB_ASCII)
        hit = (px["hit"] != 0)
        hit[:, -1] = False
        col = px["color"][hit]
        assert int(np.isnan(col).any(axis=1).sum()) >= 50                     # visible pixels with a NaN channel ...
        assert int((col == 255.0).any(axis=1).sum()) >= 200                   # ... and with an infinite one (the oracle's colour is clamped)
        _, px = _want(R, shape, "E", O.RGB_ASCII)
        assert int((px["hit"] != 0).sum()) == 0
        # div_cr's range, from rtx_device.hpp: both numerators are outside it
        assert 1e-20 < 2.0 ** -60 and 1e20 > 2.0 ** 60


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
@pytest.mark.parametrize("shape", SHAPES, ids=["37x21", "64x48"])
def test_frames_match_the_oracle_byte_for_byte(R, ctx, shape, name, plan):
    W, H = shape
    p = _params(R, shape, name)
    sph, pl = _scene(name)
    ctx.set_option(R.OPT_KERNEL, R.KERNEL_BRUTE if plan == "brute" else R.KERNEL_BINNED)
    ctx.set_option(R.OPT_REFINE, 1 if plan == "refine" else 0)
    ctx.set_scene(sph, pl)
    try:
        for mode in MODES:
            S = 20 if mode >= O.RGB_ASCII else 12
            want, _ = _want(R, shape, name, mode)
            want = want[:S * W * H]
            got = _rows(R, ctx, p, mode, 0, S)
            kernel = ctx.last_kernel
            assert kernel.startswith("rtx_trace<") and ("true" if plan != "brute" else "false") in kernel, kernel
            assert kernel.endswith(",refine>") == (plan == "refine"), kernel
            assert np.array_equal(got, want), "%s %s %s records: %s" % (name, plan, O.MODE_NAMES[mode], U.first_diff(got, want, S, W))
            words = _rows(R, ctx, p, mode, R.RENDER_COMPACT, 4).view(np.uint32)
            assert ctx.last_kernel.endswith(",refine>") == (plan == "refine"), ctx.last_kernel
            kind = ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4")
            back = U.words_to_records(words, S, kind)
            assert np.array_equal(back, want), "%s %s %s compact words: %s" % (name, plan, O.MODE_NAMES[mode], U.first_diff(back, want, S, W))
        # the floats behind the record
        _, px = _want(R, shape, name, O.RGB_ASCII)
        got = _rows(R, ctx, p, O.RGB_ASCII, R.RENDER_VALUES, 32).view(np.float32).reshape(H, W, 8)
        traced = np.ones((H, W), dtype=bool)
        traced[:, -1] = False                      # column W-1 is never traced (RayTracing.cu:187)
        hit = (px["hit"] != 0) & traced
        for what, g, w in (("distance", got[..., 0][traced], px["distance"][traced]),   # (misses: 99999999.f on both sides)
                           ("shadingValue", got[..., 1][hit], px["shading_value"][hit]), ("normal", got[..., 2:5][hit], px["normal"][hit]),
                           ("colour", got[..., 5:8][hit], px["color"][hit])):
            ok = same_bits_or_both_nan(np.ascontiguousarray(g), np.ascontiguousarray(w))
            assert ok.all(), "%s %s: %s differs on %d of %d values" % (name, plan, what, int((~ok).sum()), ok.size)
        assert not got[:, -1, :].any()
    finally:
        ctx.set_option(R.OPT_KERNEL, R.KERNEL_AUTO)
        ctx.set_option(R.OPT_REFINE, -1)
