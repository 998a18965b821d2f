"""Roll-call scenes for the trace kernels' staging and list bookkeeping (rtx_trace_body.inc, stage_chunk in rtx_kernels.hip), shared
by tests/test_host_rollcall.py (the judge: float64 and the oracle, no GPU) and tests/test_gpu_rollcall.py (the device).

A random scene pins little of that bookkeeping: most of its spheres own no pixel, so an off-by-one that drops item 256 of a staging
step or the last entry of a full list shows only where that sphere happens to be the visible winner.  Here EVERY object owns a
pixel, so losing any one item changes the frame, and the counts are swept across every threshold of the code.

The lattice.  A sphere sits on the float64 ray of a chosen pixel (c, r), directions as cull_geometry.Cam.pixel_dirs forms them, at a
depth of its own in 40 .. 200, with radius F * (the smallest angle between neighbouring pixel rays of the frame) * depth, F = 0.3;
centre and radius rounded to float32; colours >= 30 per channel.  Its own ray passes through its centre, every foreign pixel ray
passes at least 3.33 r away (by construction; the judge demands 1.5 r), so the sphere wins exactly its pixel, and it lies 0.5 pixel
pitch inside its tile's pyramid and 0.5 pitch outside its neighbour's: 0.2 pitch clear of the culling margin on either side, so that
the candidates of every tile, cell and 64-pixel wave region are KNOWN.

Multiplicity.  More candidates than pixels: fillers on the same pixel rays at larger depths (130 .. 240, inside cam_far = 250), the
same angular size, hidden behind the owner (which then lies in 40 .. 120).  They are candidates wherever the owner is, and never
win; where an owner is dropped, its filler shows.  The owners take the lowest, the highest or interleaved indices of the region.

Planes have a roll call of their own: floor rectangles (normal (0, 1, 0): Plane::Trace bounds x and z only) at distinct heights below
the camera, each around the hit point of its own pixel and smaller than the pixel spacing around it.

The thresholds the sweeps cross are literals below, each with the source line it restates; the tile shapes and cell grids the counts
assume are literals too (PLANS).  tests/test_host_rollcall.py holds both against the sources and against rtxplan's own answers."""
import functools

import numpy as np

import cull_geometry as CG
from cull_geometry import F32

F = 0.3
FAR = 250.0   # rtx_camera_params' cam_far (the host test holds it against the library's)

# ---------------------------------------------------------------------------------------------- thresholds, with their source lines
K_THREADS, K_CHUNK = 256, 512
CAP_BRUTE, CAP_CULL, CAP_REFINE = 1024, 704, 640
WAVE_CAP, REFINE_GATE = 128, 8
PLANE_TABLE, PLANE_CULL_FROM = 16, 2
SORTED_FROM = 256
TILE_LIST = 1024

SOURCE_LINES = (   # (file under csrc/, the text of the line)
    ("rtx_workgroup.hpp", "constexpr int kThreads = %d;" % K_THREADS),
    ("rtx_workgroup.hpp", "constexpr int kChunk = 2 * kThreads;"),
    ("rtx_kernels.hip", "constexpr int kListCapBrute = %d;" % CAP_BRUTE),
    ("rtx_kernels.hip", "constexpr int kListCapCull = %d;" % CAP_CULL),
    ("rtx_kernels.hip", "constexpr int kListCapRefine = %d;" % CAP_REFINE),
    ("rtx_kernels.hip", "constexpr int kWaveListCap = %d;" % WAVE_CAP),
    ("rtx_kernels.hip", "constexpr int kPlaneTable = %d;" % PLANE_TABLE),
    ("rtx_kernels.hip", "const bool second_half_empty = base + (uint32_t)kThreads >= ns;"),
    ("rtx_kernels.hip", "if (grown > cap) {"),
    ("rtx_trace_body.inc", "bool overflow = !CULL && ns > (uint32_t)kListCap;"),
    ("rtx_trace_body.inc", "if (REFINE && total > %du) {" % REFINE_GATE),
    ("rtx_trace_body.inc", "if (keepw && pos < (uint32_t)kWaveListCap) {"),
    ("rtx_trace_body.inc", "if (cnt <= (uint32_t)kWaveListCap) {"),
    ("rtx_trace_body.inc", "if (listed <= a.cell_cap) {"),
    ("rtx_trace_body.inc", "if (!REFINE && first_step_requested && listed > (uint32_t)kThreads) {"),
    ("rtx_trace_body.inc", "if (tot > (uint32_t)(kListCap - kChunk) || base + kChunk >= nit) {"),
    ("rtx_trace_body.inc", "np >= %du && !ABL(128u) && plane_invisible(" % PLANE_CULL_FROM),
    ("rtx_trace_body.inc", "const uint32_t np_tab = np < (uint32_t)kPlaneTable ? np : (uint32_t)kPlaneTable;"),
    ("rtx_tile_pass.inc", "constexpr int kTileList = %d;" % TILE_LIST),
    ("rtx_render.cpp", "ctx->sorted_gen != ctx->scene_gen && ctx->ns >= %du) {" % SORTED_FROM),
)

# ---------------------------------------------------------------------------------------------- plans
# name: (RTX_OPT_KERNEL, _TILE_LOG2_W, _SUBTILES, _TWO_LEVEL, _REFINE), what last_kernel must contain / end with.
PLANS = {
    "brute": (("brute", 0, 0, 0, 0), ",false"),
    "sub1": (("binned", 0, 1, 0, 0), ",true"),
    "sub4": (("binned", 4, 4, 0, 0), ",true"),
    "sub16": (("binned", 0, 16, 0, 0), ",true"),
    "t16": (("binned", 4, 1, 0, 0), ",true"),
    "two": (("binned", 4, 4, 1, 0), ",true"),
    "refine": (("binned", 4, 4, 0, 1), ",refine>"),
    "two_refine": (("binned", 4, 4, 1, 1), ",refine>"),
}
# (frame, plan): macro tile mw x mh, sub-tiles, REFINE taken (1) or declined (0), and the coarse-cell grid of the two-level plans:
# cells_x, cells_y, cell_w, cell_h.  Frames of fewer than 256 macro tiles: a cell is one macro tile.
SHAPES = {
    ((65, 64), "sub1"): (16, 16, 1, 0, None),
    ((65, 64), "sub4"): (32, 32, 4, 0, None),
    ((65, 64), "sub16"): (64, 64, 16, 0, None),
    ((65, 64), "two"): (32, 32, 4, 0, (3, 2, 32, 32)),
    ((65, 64), "refine"): (32, 32, 4, 1, None),
    ((73, 88), "sub4"): (32, 32, 4, 0, None),
    ((73, 88), "refine"): (32, 32, 4, 1, None),
    ((73, 88), "two"): (32, 32, 4, 0, (3, 3, 32, 32)),
    ((73, 88), "two_refine"): (32, 32, 4, 1, (3, 3, 32, 32)),
    ((65, 64), "t16"): (16, 16, 1, 0, None),   # (either way the tiles of columns 32 .. 63 see none of the planes 0 .. 15)
}


# ---------------------------------------------------------------------------------------------- geometry

@functools.lru_cache(maxsize=None)
def frame_dirs(W, H, pose):
    """The camera, its unit pixel directions (H, W, 3) in float64 and the smallest angle between neighbouring pixel rays."""
    cam = CG.camera(W, H, pose)
    d = CG.unit(cam.pixel_dirs((0, 0, W, H))).reshape(H, W, 3)
    ang = lambda a, b: np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0))
    pitch = min(float(ang(d[:, 1:], d[:, :-1]).min()), float(ang(d[1:], d[:-1]).min()))
    return cam, d, pitch


class Case:
    """sph (ns, 7) and planes (np, 11) float32 as rtx_scene_add_spheres / add_plane take them.  pix: the pixel (r * W + c) every sphere
    sits on; owner: whether it is the nearest object there.  plane_pix: the pixel every plane must win.  counts: (rect, candidates)
    pairs, rect = (c0, r0, w, h) of a macro tile, a cell or a wave region as the kernel forms it."""

    def __init__(self, name, W, H, pose="default"):
        self.name, self.W, self.H, self.pose = name, W, H, pose
        self.cam, self.dirs, self.pitch = frame_dirs(W, H, pose)
        self.sph, self.planes = np.zeros((0, 7), F32), np.zeros((0, 11), F32)
        self.pix, self.owner = np.zeros(0, np.int64), np.zeros(0, bool)
        self.plane_pix = np.zeros(0, np.int64)
        self.counts = []

    def set_spheres(self, pix, owner, rng):
        """Spheres in index order on the pixels `pix`; an owner lies in front of the fillers of its pixel."""
        pix, owner = np.asarray(pix, np.int64), np.asarray(owner, bool)
        n = len(pix)
        assert (pix % self.W != self.W - 1).all(), "column W - 1 is never traced"
        assert len(np.unique(pix[owner])) == int(owner.sum()) and np.isin(pix[~owner], pix[owner]).all()
        crowded = np.isin(pix, pix[~owner])
        depth = np.where(owner, np.where(crowded, rng.uniform(40.0, 120.0, n), rng.uniform(40.0, 200.0, n)), rng.uniform(130.0, 240.0, n))
        # fillers of one pixel: depths at least 2 % apart (redrawn from a ladder where two came close)
        for p in np.unique(pix[~owner]):
            i = np.flatnonzero((pix == p) & ~owner)
            if len(i) > 1:
                depth[i] = 130.0 + (240.0 - 130.0) * (rng.permutation(len(i)) + rng.uniform(0.2, 0.8, len(i))) / len(i)
        d = self.dirs.reshape(-1, 3)[pix]
        self.sph = np.zeros((n, 7), F32)
        self.sph[:, :3] = (self.cam.pos + d * depth[:, None]).astype(F32)
        self.sph[:, 3] = (F * self.pitch * depth).astype(F32)
        self.sph[:, 4:7] = rng.integers(30, 256, (n, 3)).astype(F32)
        self.pix, self.owner = pix, owner

    def count_in(self, rect):
        """Spheres whose pixel lies in the rectangle: by construction, the rectangle's candidates."""
        c0, r0, w, h = rect
        r, c = np.divmod(self.pix, self.W)
        return int(((c >= c0) & (c < c0 + w) & (r >= r0) & (r < r0 + h)).sum())

    def state_tiles(self, mw, mh):
        """States the count of every macro tile (= cell) of the frame."""
        for rect in _tiles(self.W, self.H, mw, mh):
            self.counts.append((rect, self.count_in(rect)))

    def params(self):
        import util as U
        c = self.cam
        return U.product_params(c.packed[:16], c.packed[16:19], self.W, self.H, c.packed[19], c.packed[20], FAR)


def _pixels(W, rect, rng=None, H=1 << 30):
    """Traced pixels of a rectangle (never column W - 1, no row from H on), in screen order or shuffled."""
    c0, r0, w, h = rect
    cols = np.arange(c0, min(c0 + w, W - 1))
    p = (np.arange(r0, min(r0 + h, H))[:, None] * W + cols[None, :]).ravel()
    return p if rng is None else rng.permutation(p)


def _tiles(W, H, mw, mh):
    return [(c0, r0, mw, mh) for r0 in range(0, H, mh) for c0 in range(0, W, mw)]


def _arranged(n_own, n_fill, order):
    """Owner flags of a region's n_own + n_fill candidates in index order: owners lowest, highest or interleaved."""
    n = n_own + n_fill
    flags = np.zeros(n, bool)
    if order == "lowest":
        flags[:n_own] = True
    elif order == "highest":
        flags[n - n_own:] = True
    else:
        assert order == "interleaved"
        flags[np.unique(np.floor(np.arange(n_own) * (n / max(n_own, 1))).astype(np.int64))[:n_own]] = True
        assert int(flags.sum()) == n_own
    return flags


def _region(pixels, k, order):
    """k candidates on the given pixels (shuffled): min(k, pixels) owners, the rest fillers dealt round over the owners' pixels."""
    n_own = min(k, len(pixels))
    flags = _arranged(n_own, k - n_own, order)
    pix = np.empty(k, np.int64)
    pix[flags] = pixels[:n_own]
    pix[~flags] = pixels[np.arange(k - n_own) % max(n_own, 1)]
    return pix, flags


# ---------------------------------------------------------------------------------------------- sweep 1: scene size

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537)
SIZE_PLANS = ("brute", "sub1", "sub4", "sub16", "two", "refine")


@functools.lru_cache(maxsize=None)
def size_case(ns, order="permuted", pose="default"):
    """ns owners spread over the whole 65 x 64 frame, index order a fixed permutation of the screen order (or the identity)."""
    c = Case("size %d %s %s" % (ns, order, pose), 65, 64, pose)
    rng = np.random.default_rng(29000 + ns)
    pix = np.sort(_pixels(65, (0, 0, 65, 64), rng)[:ns])
    if order == "permuted":
        pix = rng.permutation(pix)
    c.set_spheres(pix, np.ones(ns, bool), rng)
    return c


# ---------------------------------------------------------------------------------------------- sweep 2: candidates of one macro tile

# 73 x 88: nearly square pixels, so that the frame holds 6336 traced pixels at a pitch of 0.0093 rad -- the float32 hit test's own
# error on a sphere of 0.3 pitch is then 7e-5 of its distance at most (a wider frame's narrower pixels take it past the judge's 1e-4)
TILE_FRAME = (73, 88)
MACRO = (32, 32)                 # the macro tile of the sub4 / refine / two plans on this frame (SHAPES)
TILE_RECT = (32, 0, 32, 32)      # macro tile (1, 0): 1024 traced pixels, none of the last column
TILE_K = {cap: tuple(cap + d for d in (-513, -512, -511, -1, 0, 1, 511, 512, 513)) + (2 * cap + 1,) for cap in (CAP_CULL, CAP_REFINE)}
ORDERS = ("lowest", "highest", "interleaved")


def tile_variants(cap):
    """(k, placement, order): every k at both placements; the three owner orders where the tile has fillers (k > its 1024 pixels), in
    the `first` placement, interleaved alone in the `spread` one."""
    out = []
    for k in TILE_K[cap]:
        for placement in ("first", "spread"):
            for order in (ORDERS if k > 1024 and placement == "first" else ("interleaved",)):
                out.append((k, placement, order))
    return out


@functools.lru_cache(maxsize=None)
def tile_case(k, placement, order):
    """The tile TILE_RECT holds k candidates; three times as many owners lie in the other tiles.  `first`: the tile's candidates
    take the lowest scene indices (a capacity is crossed at the start of a staging step); `spread`: every fourth index is one of
    them (... inside a step)."""
    W, H = TILE_FRAME
    c = Case("tile %d %s %s" % (k, placement, order), W, H)
    rng = np.random.default_rng(31000 + k)
    mine, flags = _region(_pixels(W, TILE_RECT, rng), k, order)
    inside = set(_pixels(W, TILE_RECT).tolist())
    others = np.array([p for p in _pixels(W, (0, 0, W, H), rng) if p not in inside], np.int64)[:3 * k]
    assert len(others) == 3 * k
    if placement == "first":
        pix, owner = np.concatenate([mine, others]), np.concatenate([flags, np.ones(3 * k, bool)])
    else:
        assert placement == "spread"
        pix, owner = np.empty(4 * k, np.int64), np.ones(4 * k, bool)
        pix[0::4], owner[0::4] = mine, flags
        for j in (1, 2, 3):
            pix[j::4] = others[j - 1::3]
    c.set_spheres(pix, owner, rng)
    c.state_tiles(*MACRO)
    assert (TILE_RECT, k) in c.counts
    return c


# ---------------------------------------------------------------------------------------------- sweep 3: a wave's list (REFINE)

WAVE_FRAME = TILE_FRAME
WAVE_TILE = (32, 0, 32, 32)
WAVE_RECT = (48, 4, 16, 4)       # sub-tile 1 (16 x 16), wave 1: all its 16 columns, rows 4 .. 7
WAVE_COUNTS = (127, 128, 129, 192)
GATE_TOTALS = (REFINE_GATE, REFINE_GATE + 1)


def wave_regions(tile):
    """The sixteen 64-pixel wave regions of a macro tile of four 16 x 16 sub-tiles, laid out mw / 16 wide (rtx_trace_body.inc: region =
    sub-tile * 4 + wave; a wave's pixels are all 16 columns of its sub-tile and 4 rows)."""
    c0, r0, mw, _ = tile
    nx = mw // 16
    return [(c0 + (s % nx) * 16, r0 + (s // nx) * 16 + w * 4, 16, 4) for s in range(4) for w in range(4)]


@functools.lru_cache(maxsize=None)
def wave_case(n, order):
    """One wave region with n candidates (64 owners, n - 64 fillers); the other fifteen regions of its tile hold 6 owners each (far
    below the wave capacity: refined and unrefined waves in one workgroup), the other tiles 40 each."""
    W, H = WAVE_FRAME
    c = Case("wave %d %s" % (n, order), W, H)
    rng = np.random.default_rng(33000 + n)
    mine, flags = _region(_pixels(W, WAVE_RECT, rng), n, order)
    pix, owner = [mine], [flags]
    for reg in wave_regions(WAVE_TILE):
        if reg != WAVE_RECT:
            pix.append(_pixels(W, reg, rng)[:6])
    for rect in _tiles(W, H, *MACRO):
        if rect != WAVE_TILE:
            pix.append(_pixels(W, rect, rng, H)[:40])
    owner += [np.ones(len(p), bool) for p in pix[1:]]
    # the region's candidates keep their order among themselves; the scene's index order mixes them with the rest
    pix, owner = np.concatenate(pix), np.concatenate(owner)
    slot = np.sort(rng.permutation(len(pix))[:n])
    rest = np.setdiff1d(np.arange(len(pix)), slot)
    p2, o2 = np.empty_like(pix), np.empty_like(owner)
    p2[slot], o2[slot] = pix[:n], owner[:n]
    mix = rng.permutation(len(pix) - n) + n
    p2[rest], o2[rest] = pix[mix], owner[mix]
    c.set_spheres(p2, o2, rng)
    c.state_tiles(*MACRO)
    for reg in wave_regions(WAVE_TILE):
        c.counts.append((reg, c.count_in(reg)))
    assert c.count_in(WAVE_RECT) == n and c.count_in(WAVE_TILE) == n + 90 <= CAP_REFINE
    return c


@functools.lru_cache(maxsize=None)
def gate_case(total):
    """The tile WAVE_TILE holds `total` candidates (the REFINE gate: total > 8), the other tiles 20 each."""
    W, H = WAVE_FRAME
    c = Case("gate %d" % total, W, H)
    rng = np.random.default_rng(34000 + total)
    pix = [_pixels(W, WAVE_TILE, rng)[:total]]
    for rect in _tiles(W, H, *MACRO):
        if rect != WAVE_TILE:
            pix.append(_pixels(W, rect, rng, H)[:20])
    pix = rng.permutation(np.concatenate(pix))
    c.set_spheres(pix, np.ones(len(pix), bool), rng)
    c.state_tiles(*MACRO)
    return c


# ---------------------------------------------------------------------------------------------- sweep 4: cell lists (two-level)

CELL_FRAME = TILE_FRAME
CELL_RECT = (32, 32, 32, 32)     # cell 4, the middle one of the 3 x 3 grid (a cell is one 32 x 32 macro tile)
CELL_LISTED = (0, 1, 255, 256, 257, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def cell_case(listed):
    """The cell CELL_RECT lists `listed` owners; the other cells 40 each."""
    W, H = CELL_FRAME
    c = Case("cell %d" % listed, W, H)
    rng = np.random.default_rng(35000 + listed)
    pix = [_pixels(W, CELL_RECT, rng)[:listed]]
    for rect in _tiles(W, H, *MACRO):
        if rect != CELL_RECT:
            pix.append(_pixels(W, rect, rng, H)[:40])
    pix = rng.permutation(np.concatenate(pix))
    c.set_spheres(pix, np.ones(len(pix), bool), rng)
    c.state_tiles(*MACRO)
    assert (CELL_RECT, listed) in c.counts
    return c


# ---------------------------------------------------------------------------------------------- sweep 5: planes

PLANE_FRAME = (65, 64)
PLANE_COUNTS = (0, 1, 2, 15, 16, 17, 18, 33)
PLANE_SPHERES = 300


@functools.lru_cache(maxsize=None)
def plane_case(n_planes, with_spheres):
    """n_planes floors, each the winner of its own pixel of the lower half of a 65 x 64 frame: planes 0 .. 15 (the LDS table's) in the
    left half, planes 16 .. in the right half, whose tiles therefore see no table plane at all (table empty, direct form alone).
    Optionally a 300-sphere lattice in the upper half."""
    W, H = PLANE_FRAME
    c = Case("planes %d%s" % (n_planes, " + spheres" if with_spheres else ""), W, H)
    rng = np.random.default_rng(37000 + n_planes)
    rows = (35, 39, 43, 47, 51, 55, 59)
    left = [(col, r) for r in rows for col in range(3, 30, 6)]
    right = [(col, r) for r in rows for col in range(35, 62, 6)]
    slots = [left[i] if i < PLANE_TABLE else right[i - PLANE_TABLE] for i in range(n_planes)]
    o = c.cam.pos
    planes = np.zeros((n_planes, 11), F32)
    for i, (col, r) in enumerate(slots):
        height = 3.0 + 0.25 * i                       # below the camera: y = o.y - height
        hit = lambda cc, rr: o + c.dirs[rr, cc] * (height / -c.dirs[rr, cc, 1])
        p = hit(col, r)
        half_w = 0.8 * min(abs(hit(col + 1, r)[0] - p[0]), abs(hit(col - 1, r)[0] - p[0]))
        half_h = 0.8 * min(abs(hit(col, r + 1)[2] - p[2]), abs(hit(col, r - 1)[2] - p[2]))
        planes[i] = [p[0], p[1], p[2], 0.0, 1.0, 0.0] + list(rng.integers(30, 256, 3)) + [2.0 * half_w, 2.0 * half_h]
    c.planes = planes
    c.plane_pix = np.array([r * W + col for col, r in slots], np.int64)
    if with_spheres:
        pix = _pixels(W, (0, 0, W, 30), rng)[:PLANE_SPHERES]
        c.set_spheres(pix, np.ones(len(pix), bool), rng)
    return c


def all_cases():
    """Every case of the sweeps, for the judge."""
    out = [size_case(n) for n in SIZES]
    out += [size_case(n, "identity") for n in (257, 1025)] + [size_case(n, "permuted", "rolled") for n in (513, 1281)]
    for cap in (CAP_CULL, CAP_REFINE):
        out += [tile_case(*v) for v in tile_variants(cap)]
    out += [wave_case(n, order) for n in WAVE_COUNTS for order in ORDERS]
    out += [gate_case(t) for t in GATE_TOTALS]
    out += [cell_case(n) for n in CELL_LISTED]
    out += [plane_case(n, s) for n in PLANE_COUNTS for s in (False, True)]
    return out
