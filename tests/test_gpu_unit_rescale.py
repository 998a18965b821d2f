"""Re-normalising unit vectors from a table (csrc/rtx_unit.hpp, rtx_device.hpp: unit_rescale / renormalize_gpu).

1. The proof: unit_rescale(x) returns the bits of 1.0f / sqrtf(x) for every one of the 2^32 fp32 inputs (the table inside its
   window, the generic expansions outside), on the GPU, as tests/test_gpu_math.py proves rcp_cr and sqrt_cr.
2. Parity of the four call sites on small frames: the floats behind the records (RTX_RENDER_VALUES: distance, shadingValue,
   normal, colour) of the brute and the culling kernel, bit for bit against the oracle -- three ordinary scenes, the scene of
   test_gpu_parity.py scaled by 1e18 (every hit lies beyond the reference's initial closest distance of 99999999: nothing is
   shaded, the frame must say so) and by 1e-18 (everything is shaded, from squared lengths around 1e-34), and one in which
   pixels certainly leave the table's window: planes beyond the kernels' LDS table, whose raw, un-normalised normals go
   through renormalize_gpu.  (No scene reaches the window's outside at the other three call sites -- they see vectors that
   normalize_gpu has just produced; there the proof above stands alone.)"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import util as U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 160, 90

# rtx_unit.hpp: the window of bit offsets from 1.0f that the table answers
ONE_BITS, K_MIN, K_MAX = 0x3F800000, -12, 3


# ---------------------------------------------------------------- the proof

def test_unit_rescale_is_bit_identical_on_all_inputs():
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy first)
    path = os.path.join(HERE, "gpu_checks", "libunit_check.so")
    assert os.path.exists(path), "run __graft_entry__.build()"
    lib = C.CDLL(path)
    lib.rtx_check_unit_rescale_exhaustive.restype = C.c_longlong
    lib.rtx_check_unit_rescale_exhaustive.argtypes = [C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]
    first, tabled = C.c_uint(0), C.c_ulonglong(0)
    bad = lib.rtx_check_unit_rescale_exhaustive(C.byref(first), C.byref(tabled))
    assert bad == 0, "unit_rescale(x) != 1.0f/sqrtf(x) on %d inputs, first bit pattern 0x%08x" % (bad, first.value)
    assert tabled.value == K_MAX - K_MIN + 1   # the table answered exactly its window: the walk did go through it


# ---------------------------------------------------------------- parity of the call sites

def _scaled_scene(scale):
    """test_gpu_parity.py: test_scenes_at_extreme_scales, its scene."""
    rng = np.random.default_rng(12)
    n = 120
    centres = np.stack([rng.uniform(-60, 60, n), rng.uniform(-20, 20, n), rng.uniform(20, 200, n)], axis=1) * scale
    radii = rng.uniform(2, 15, n) * scale
    cols = np.floor(rng.uniform(1, 256, (n, 3)))
    sph = np.concatenate([centres, radii[:, None], cols], axis=1).astype(np.float32)
    pl = np.array([[0, -30 * scale, 125 * scale, 0, 1, 0, 100, 100, 100, 3000 * scale, 250 * scale]], dtype=np.float32)
    return sph, pl


def _many_planes():
    """20 small planes in front of the camera, none with a unit normal: those past the 16th are shaded from the arrays."""
    rng = np.random.default_rng(21)
    pl = np.zeros((20, 11), dtype=np.float32)
    for i in range(20):
        pl[i, 0:3] = (rng.uniform(-25, 25), rng.uniform(-12, -2), rng.uniform(25, 120))
        pl[i, 3:6] = (rng.normal(0, 0.3), rng.uniform(0.5, 3.0), rng.normal(0, 0.3))
        pl[i, 6:9] = np.floor(rng.uniform(1, 256, 3))
        pl[i, 9:11] = (rng.uniform(20, 60), rng.uniform(20, 60))
    sph = np.array([[0, 4, 60, 5, 200, 40, 40], [-12, 6, 80, 4, 40, 200, 40]], dtype=np.float32)
    return sph, pl


CASES = ["seed1", "seed2", "seed3", "scale1e18", "scale1e-18", "planes20"]
_cache = {}


def _case(R, name):
    """Inputs and the oracle's per-pixel values of a case, computed once and shared by the kernels."""
    if name not in _cache:
        if name.startswith("seed"):
            p = R.camera_params(W, H)
            sph, pl = R.synth_scene(int(name[4:]), 64, 2, p.element1, p.element2)
        elif name.startswith("scale"):
            p = R.camera_params(W, H, (0.0, 0.0, 0.0), (0.05, 3.1, 0.0))
            sph, pl = _scaled_scene(float(name[5:]))
        else:
            p = R.camera_params(W, H)
            sph, pl = _many_planes()
        _, px = O.render(U.oracle_params(p), O.Scene.from_arrays(sph, pl), O.RGB_ASCII, want_pixels=True)
        px.setflags(write=False)
        _cache[name] = (p, sph, pl, px)
    return _cache[name]


def outside_window(v):
    """Per vector: is its squared length, formed as normalize_gpu forms it in fp32, outside the table's window?"""
    v = v.astype(np.float32)
    with np.errstate(all="ignore"):
        len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    k = len2.view(np.uint32).astype(np.int64) - ONE_BITS
    return (k < K_MIN) | (k > K_MAX)


def same_bits_or_both_nan(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def R():
    return U.pkg()


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(W, H)
    yield c
    c.close()


@pytest.mark.parametrize("kernel", ["brute", "binned"])
@pytest.mark.parametrize("name", CASES)
def test_values_match_the_oracle_bit_for_bit(R, ctx, name, kernel):
    import torch
    p, sph, pl, px = _case(R, name)
    ctx.set_option(R.OPT_KERNEL, {"brute": R.KERNEL_BRUTE, "binned": R.KERNEL_BINNED}[kernel])
    ctx.set_scene(sph, pl)
    vals = torch.zeros(W * H * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.render_rows(p, R.RGB_ASCII, 0, H, d_out=vals.data_ptr(), out_row_base=0, flags=R.RENDER_VALUES)
    ctx.synchronize()
    assert ctx.last_kernel.startswith("rtx_trace<RTX_K_RGB_ASCII,%s" % ("true" if kernel == "binned" else "false")), ctx.last_kernel
    got = vals.cpu().numpy().reshape(H, W, 8)
    traced = np.ones((H, W), dtype=bool)
    traced[:, -1] = False                      # column W-1 is never traced (RayTracing.cu:187)
    hit = (px["hit"] != 0) & traced
    if name == "scale1e18":
        assert hit.sum() == 0
    else:
        assert hit.sum() > 0.5 * traced.sum(), "the scene shows too little"
        assert int(outside_window(px["normal"][hit]).sum()) == 0   # what normalize_gpu produced stays inside the window
    if name == "planes20":
        # pixels won by a plane past the table: the oracle's normal there is that plane's normalised normal and no table plane's
        n = pl[:, 3:6].astype(np.float64)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        near = np.abs(px["normal"][hit][:, None, :].astype(np.float64) - n[None, :, :]).max(axis=2) < 1e-6
        assert int((near[:, 16:].any(axis=1) & ~near[:, :16].any(axis=1)).sum()) > 50
    for what, g, w in (("distance", got[..., 0][traced], px["distance"][traced]),   # (misses: 99999999.f on both sides)
                       ("shadingValue", got[..., 1][hit], px["shading_value"][hit]), ("normal", got[..., 2:5][hit], px["normal"][hit]),
                       ("colour", got[..., 5:8][hit], px["color"][hit])):
        ok = same_bits_or_both_nan(np.ascontiguousarray(g), np.ascontiguousarray(w))
        assert ok.all(), "%s %s: %s differs on %d of %d values" % (name, kernel, what, int((~ok).sum()), ok.size)
    assert not got[:, -1, :].any()
