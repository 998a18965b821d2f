"""rtx_set_option / rtx_get_option and the device-backed counters through the public API alone, pinned to what the library did while
every option was a `case` of its own and every counter read-back written out: defaults, accepted and refused values with the refusal
texts, counters that read 0 before any frame, and which launch sets leave RTX_STAT_REFLECT_RAYS and RTX_STAT_REFLECT_SHADOW_POINTS
readable.  64 x 32 RGB_ASCII frames of the reference default scene."""
import ctypes as C

import pytest

import util as U

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# number, lo, hi, extra accepted value (a hole in the range) or None, default, refusal text
ROWS = [
    (1, 0, 2, None, 0, "RTX_OPT_KERNEL: unknown kernel"),
    (2, 2, 6, 0, 0, "RTX_OPT_TILE_LOG2_W: 0 or 2..6"),
    (3, 0, 16, None, 0, "RTX_OPT_SUBTILES: 0..16"),
    (4, -1, 2, None, -1, "RTX_OPT_TWO_LEVEL: -1 (auto), 0 or 1 (2 is accepted as 1)"),
    (5, -1, 1, None, -1, "RTX_OPT_REFINE: -1 (auto), 0 or 1"),
    (6, -1, 1 << 20, None, -1, "RTX_OPT_TILE_ORDER: -1 (auto), 0 (off) or the refresh period in frames"),
    (7, 0, 1 << 31, None, 0, "RTX_OPT_CELL_CAPACITY: 0 (auto) or entries per cell list"),
    (8, -1, 1, None, -1, "RTX_OPT_CELL_REUSE: -1 (auto), 0 or 1"),
    (9, -1, 1, None, -1, "RTX_OPT_XCD_ORDER: -1 (auto), 0 or 1"),
    (10, -1, 1, None, -1, "RTX_OPT_VIEW_ADAPT: -1 (auto), 0 or 1"),
    (11, -1, 1, None, -1, "RTX_OPT_SORTED_STORE: -1 (auto), 0 or 1"),
    (14, -1, 1, None, -1, "RTX_OPT_BATCH: -1 (auto), 0 or 1"),
    (15, -1, 1, None, -1, "RTX_OPT_UPDATE_WORDS: -1 (auto), 0 or 1"),
    (17, -1, 2, None, -1, "RTX_OPT_MINIMIZE_FUSED: -1 (auto), 0, 1 or 2"),
    (19, -1, 1, None, -1, "RTX_OPT_UPDATE_HOST_WRITE: -1 (auto), 0 or 1"),
    (20, 0, 1, None, 0, "RTX_OPT_SHADOWS: 0 or 1"),
    (21, 0, 2, None, 0, "RTX_OPT_SHADOW_CHECK: 0, 1 or 2"),
    (22, 0, 2, None, 0, "RTX_OPT_REFLECT_CHECK: 0, 1 or 2"),
    (23, 0, 1, None, 0, "RTX_OPT_QUERY_CHECK: 0 or 1"),
    (24, 0, 4096, None, 0, "RTX_OPT_QUERY_LOAD: 0 (default) or sixteenths of a sphere per cell, up to 4096"),
    (25, 0, 1, None, 0, "RTX_OPT_LIGHTS_CHECK: 0 or 1"),
    (26, 1, 4, None, 1, "RTX_OPT_REFLECT_DEPTH: 1 .. RTX_MAX_REFLECT_DEPTH"),
    (27, 0, 1, None, 0, "RTX_OPT_REFLECT_DEPTH_CHECK: 0 or 1"),
    (28, 0, 1, None, 0, "RTX_OPT_REFLECT_SHADOWS: 0 or 1"),
    (29, 0, 1, None, 0, "RTX_OPT_SHADOW_GRID: 0 or 1"),
    (30, 1, 4, None, 1, "RTX_OPT_SUPERSAMPLE: 1, 2, 3 or 4"),
    (31, 0, 1, None, 0, "RTX_OPT_REFLECT_GRID: 0 or 1"),
]

W, H = 64, 32
MIRRORS = {0: 0.3, 2: 0.8, 5: 0.6}  # two spheres and the floor


@pytest.fixture(scope="module")
def R():
    return U.pkg()


def _get(R, c, option):
    v = C.c_int64(-12345)
    return R.lib().rtx_get_option(c._h, option, C.byref(v)), v.value


def _set(R, c, option, value):
    return R.lib().rtx_set_option(c._h, option, value)


def _error(R, c):
    return (R.lib().rtx_last_error(c._h) or b"").decode()


def test_options_on_a_fresh_context(R):
    assert len(ROWS) == 27
    with R.Context(W, H) as c:
        for option, lo, hi, extra, default, text in ROWS:
            assert _get(R, c, option) == (R.OK, default), option
        for option, lo, hi, extra, default, text in ROWS:
            refused = [lo - 1, hi + 1, I64_MIN, I64_MAX] + ([1, 7] if option == R.OPT_TILE_LOG2_W else [])
            for stored in [lo, hi] + ([extra] if extra is not None else []):
                assert _set(R, c, option, stored) == R.OK, (option, stored)
                assert _get(R, c, option) == (R.OK, stored), (option, stored)
                for bad in refused:
                    assert _set(R, c, option, bad) == R.ERR_INVALID_ARGUMENT, (option, bad)
                    assert _error(R, c) == text, (option, bad)
                    assert _get(R, c, option) == (R.OK, stored), (option, bad)
            assert _set(R, c, option, default) == R.OK
        for option, lo, hi, extra, default, text in ROWS:  # nobody's store landed in a neighbour
            assert _get(R, c, option) == (R.OK, default), option
        for unknown in (0, 32):
            assert _set(R, c, unknown, 0) == R.ERR_INVALID_ARGUMENT and _error(R, c) == "unknown option"
            assert _get(R, c, unknown) == (R.ERR_INVALID_ARGUMENT, -12345)


def _device_counters(R):
    per_level = [base + l for base in (R.STAT_REFLECT_RAYS, R.STAT_REFLECT_SHADOW_POINTS) for l in range(R.MAX_REFLECT_DEPTH)]
    return [R.STAT_SHADOW_LONGEST_LIST, R.STAT_REFLECT_LONGEST_LIST] + per_level + [
        R.STAT_SHADOW_GRID_FALLBACK_POINTS, R.STAT_REFLECT_GRID_FALLBACK_RAYS, R.STAT_DELTA_CELLS, R.STAT_DELTA_RUNS, R.STAT_QUERY_FALLBACK_RAYS]


def test_device_counters_read_zero_before_any_frame(R):
    with R.Context(W, H) as c:
        for stat in _device_counters(R):
            assert _get(R, c, stat) == (R.OK, 0), stat
        c.set_reference_default_scene()
        for stat in _device_counters(R):
            assert _get(R, c, stat) == (R.OK, 0), stat


def _levels(R, c, base):
    return [int(c.get_option(base + l)) for l in range(R.MAX_REFLECT_DEPTH)]


def test_which_launch_sets_leave_the_mirror_counters_readable(R):
    with R.Context(W, H) as c:
        c.set_reference_default_scene()
        p = R.camera_params(W, H)
        n = c.object_count
        # (a) the chain kernels with shadows seen in mirrors: both arrays count
        for i, k in MIRRORS.items():
            c.set_reflectivity(i, k)
        c.set_option(R.OPT_SHADOWS, 1)
        c.set_option(R.OPT_REFLECT_SHADOWS, 1)
        c.set_option(R.OPT_REFLECT_DEPTH, 2)
        c.render_to_host(p, R.RGB_ASCII)
        rays, points = _levels(R, c, R.STAT_REFLECT_RAYS), _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS)
        print("(a) rays", rays, "points", points, c.last_kernel)
        assert rays[0] > 0 and rays[1] > 0 and rays[2:] == [0, 0]
        assert points[0] > 0
        # (b) nothing reflects, the shaded path: the rays of (a) stay readable, the points read 0
        c.set_reflectivity(0, [0.0] * n)
        c.render_to_host(p, R.RGB_ASCII)
        print("(b)", c.last_kernel)
        assert "reflect" not in c.last_kernel and "chain" not in c.last_kernel
        assert _levels(R, c, R.STAT_REFLECT_RAYS) == rays
        assert _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS) == [0, 0, 0, 0]
        # (c) the one-bounce mirror path: neither array counts
        for i, k in MIRRORS.items():
            c.set_reflectivity(i, k)
        c.set_option(R.OPT_REFLECT_DEPTH, 1)
        c.set_option(R.OPT_REFLECT_SHADOWS, 0)
        c.render_to_host(p, R.RGB_ASCII)
        print("(c)", c.last_kernel)
        assert "reflect_shade" in c.last_kernel
        assert _levels(R, c, R.STAT_REFLECT_RAYS) == [0, 0, 0, 0]
        assert _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS) == [0, 0, 0, 0]
        # (d) the direct path leaves the rays as (c) did, and the points read 0
        c.render_to_host(p, R.RGB_NORMALS)
        print("(d)", c.last_kernel)
        assert _levels(R, c, R.STAT_REFLECT_RAYS) == [0, 0, 0, 0]
        assert _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS) == [0, 0, 0, 0]
        # ... and a direct frame after a counting set leaves the rays of that set readable, as (b)
        c.set_option(R.OPT_REFLECT_DEPTH, 2)
        c.set_option(R.OPT_REFLECT_SHADOWS, 1)
        c.render_to_host(p, R.RGB_ASCII)
        assert _levels(R, c, R.STAT_REFLECT_RAYS) == rays and _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS) == points
        c.render_to_host(p, R.RGB_NORMALS)
        assert _levels(R, c, R.STAT_REFLECT_RAYS) == rays
        assert _levels(R, c, R.STAT_REFLECT_SHADOW_POINTS) == [0, 0, 0, 0]
