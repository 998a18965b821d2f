"""tests/restate.py on the CPU: no GPU, no torch.
  1. The anchor: with no mirrors and the reference's light, trace_chain + shade_chain equal the CPU oracle's per-pixel values
     (distance, shading_value, normal, colour) bit for bit on every visible pixel, and the hit masks agree, on the default scene,
     C1 and six of tests/fuzz_cases.py's scenes (general matrices, tiny radii, planes with arbitrary normals, up to 700 spheres).
  2. encode_records equals the oracle's records on the same frames in the four character modes and RGB_NORMALS; encode_words
     expanded (util.words_to_records) equals them too.
  3. A set holding only the reference's light reproduces tests/test_gpu_reflect_depth.py::restate_chain at depths 1-4, and depth 1
     under three lights reproduces tests/test_gpu_lights.py::restate.
  4. The inputs of tests/test_gpu_chain_lights.py, judged on the restatement alone so that the GPU tests cannot hide a failure
     behind them: rays per level, colours below the clamp, shadow coverage as float64 decides it, few ambiguous pixels, light order
     and mirror blend that show in the bytes."""
import functools

import numpy as np
import pytest

import fuzz_cases as F
import oracle as O
import restate as RS
import util as U

f32 = np.float32
ANCHOR_FUZZ_SEEDS = [0, 1, 2, 4, 7, 11]
ANCHORS = ["default", "C1"] + ["fuzz%d" % s for s in ANCHOR_FUZZ_SEEDS]


@functools.lru_cache(maxsize=None)
def _anchor(name):
    """(params, scene arrays, pixels, the oracle's pixels, the restatement's eight values) without mirrors, the reference's light."""
    if name == "default":
        p, sph, pl = O.camera_params(400, 150), RS.DEFAULT_SPH, RS.DEFAULT_PL
        pix = np.arange(400 * 150)
    elif name == "C1":
        p, sph, pl = RS.config_case("C1")
        pix = np.arange(int(p.x) * int(p.y))
    else:
        p, sph, pl, _, _, pix = F.chain_inputs(int(name[4:]))
        assert len(sph) <= 700 and len(pix) <= 8000
    sc = O.Scene.from_arrays(sph, pl)
    _, px = O.render(p, sc, O.RGB_ASCII, want_pixels=True)
    trace = RS.trace_chain(p, sph, pl, {}, pix, max_depth=1)
    vals = RS.values8(trace, RS.shade_chain(trace, [RS.reference_light()])[1])
    return p, sc, pix, px.reshape(-1)[pix], trace, vals


# ---------------------------------------------------------------- 1. the anchor

@pytest.mark.parametrize("name", ANCHORS)
def test_restatement_equals_oracle(name):
    p, sc, pix, px, trace, vals = _anchor(name)
    W = int(p.x)
    assert trace["rays"] == [0]
    inside = pix % W != W - 1  # (the oracle, like the kernels, traces no pixel of column W-1)
    assert np.array_equal(px["hit"][inside] != 0, trace["hit"][inside]), "hit masks differ at %d pixels" % int(((px["hit"] != 0) != trace["hit"])[inside].sum())
    assert not px["hit"][~inside].any()
    vis = trace["vis"]
    if name in ("default", "C1"):
        assert vis.sum() > 0.15 * len(pix)
    want = np.concatenate([px["distance"][:, None], px["shading_value"][:, None], px["normal"], px["color"]], axis=1).astype(np.float32)
    same = RS.same_floats(vals, want)
    for j, field in enumerate(["distance", "shading_value", "normal.x", "normal.y", "normal.z", "colour.r", "colour.g", "colour.b"]):
        bad = np.nonzero(~same[:, j] & vis)[0]
        assert bad.size == 0, "%s: %s differs at %d of %d visible pixels, e.g. pixel %d: restatement %r oracle %r" % (
            name, field, bad.size, int(vis.sum()), int(pix[bad[0]]), vals[bad[0], j], want[bad[0], j])
    # a pixel without a hit: the distance the oracle starts from
    assert (vals[~trace["hit"] & inside, 0] == RS.NO_HIT).all() and (px["distance"][~trace["hit"] & inside] == RS.NO_HIT).all()


def test_the_anchor_scenes_have_edges():
    """What the six fuzz scenes bring that the tame ones do not: planes whose normal is no axis, a rolled camera matrix, radii
    under 0.05, visible pixels in the first and the last row, hits beyond the far plane (no record, but values)."""
    skew = tiny = rolled = first = last = beyond = 0
    for s in ANCHOR_FUZZ_SEEDS:
        p, sph, pl, _, _, pix = F.chain_inputs(s)
        trace = _anchor("fuzz%d" % s)[4]
        W, H = int(p.x), int(p.y)
        skew += int((np.abs(RS.host_planes(pl)[:, 3:6]).max(axis=1) < 0.999).sum()) if len(pl) else 0
        tiny += int((sph[:, 3] < 0.05).sum())
        rolled += int(abs(p.inv_v[1][0]) > 1e-3)
        first += int(trace["vis"][pix < W].sum())
        last += int(trace["vis"][pix >= (H - 1) * W].sum())
        beyond += int((trace["vis"] & (trace["t"] > f32(p.cam_far))).sum())
    print("skew planes %d, tiny spheres %d, rolled cameras %d, visible in the first row %d, in the last %d, beyond far %d" % (skew, tiny, rolled, first, last, beyond))
    assert skew >= 10 and tiny >= 10 and rolled >= 3 and first >= 100 and last >= 100


# ---------------------------------------------------------------- 2. the encoders

@pytest.mark.parametrize("mode", [O.BIT_ASCII, O.BIT_PIXEL, O.RGB_ASCII, O.RGB_PIXEL, O.RGB_NORMALS])
@pytest.mark.parametrize("name", ANCHORS)
def test_encoders_equal_oracle_records(name, mode):
    p, sc, pix, px, trace, vals = _anchor(name)
    W, H = int(p.x), int(p.y)
    S = 12 if mode < O.RGB_ASCII else 20
    want = O.render(p, sc, mode)[:W * H * S].reshape(-1, S)[pix]
    got = RS.encode_records(vals, mode, p.cam_far)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s %s: %d records differ, e.g. pixel %d: %r, the oracle %r" % (
        name, O.MODE_NAMES[mode], bad.size, int(pix[bad[0]]), bytes(got[bad[0]]), bytes(want[bad[0]]))
    words = RS.encode_words(vals, mode, p.cam_far)
    assert (words[pix % W == W - 1] == 0xFFFFFFFF).all()
    back = U.words_to_records(words, S, ord("3") if mode in (O.BIT_ASCII, O.RGB_ASCII) else ord("4")).reshape(-1, S)
    assert np.array_equal(back, want), "%s %s: the words expand to other records" % (name, O.MODE_NAMES[mode])
    # the words hold what the records hold: colour bytes and glyph of every visible pixel
    visible = (want[:, 2] == ord("3")) if mode in (O.BIT_ASCII, O.RGB_ASCII) else (words != 0) & (words != 0xFFFFFFFF)
    assert np.array_equal((words >> np.uint32(24))[visible].astype(np.uint8), want[visible, S - 1])


def test_encoder_edges():
    """u8_sat, ramp_index and digits3 at their edges: NaN and negative colours give 0, 255.9 truncates, a NaN or negative
    shadingValue clamps to ramp index 1, 1.0 reaches index 67, distance == far is visible and the next float is not."""
    far = 250.0
    v = np.zeros((6, 8), dtype=np.float32)
    v[:, 0] = [10.0, 10.0, far, np.nextafter(f32(far), f32(1e9)), 10.0, 0.0]
    v[:, 1] = [np.nan, -0.5, 1.0, 1.0, 0.0149, 0.0]
    v[:, 5] = [np.nan, -3.0, 255.0, 255.0, 9.99, 0.0]
    v[:, 6] = [254.999, 100.0, 99.5, 1.0, 10.0, 0.0]
    v[:, 7] = [0.5, 7.0, 200.0, 1.0, 100.0, 0.0]
    rec = RS.encode_records(v, O.RGB_ASCII, far)
    assert bytes(rec[0]) == b"\x1b[38;2;\x00\x000;254;\x00\x000m."
    assert bytes(rec[1]) == b"\x1b[38;2;\x00\x000;100;\x00\x007m."
    assert bytes(rec[2]) == b"\x1b[38;2;255;\x0099;200m@"
    assert bytes(rec[3]) == b"\x1b[48;2;\x00\x000;\x00\x000;\x00\x000m "
    assert bytes(rec[4]) == b"\x1b[38;2;\x00\x009;\x0010;100m."
    assert bytes(rec[5]) == b"\x00" * 20
    words = RS.encode_words(v, O.RGB_PIXEL, far)
    assert [int(w) for w in words] == [0x2000FE00, 0x20076400, 0x20C863FF, 0, 0x20640A09, 0xFFFFFFFF]
    bit = RS.encode_records(v, O.BIT_PIXEL, far)
    assert bytes(bit[3]) == b"\x1b[48;5;\x0016m " and bytes(bit[5]) == b"\x00" * 12
    index = O.lib().orc_ansi256_from_rgb(0xFF63C8)
    assert index >= 100 and bytes(bit[2]) == b"\x1b[48;5;%dm " % index


# ---------------------------------------------------------------- 3. the older restatements

@functools.lru_cache(maxsize=None)
def _scene(name):
    p, sph, pl, ks, pix = RS.chain_scene(name)
    return p, sph, pl, ks, pix, RS.trace_chain(p, sph, pl, ks, pix)


@pytest.mark.parametrize("name", ["default", "mirror_floor"])
def test_reference_light_set_reproduces_restate_chain(name):
    from test_gpu_reflect_depth import restate_chain
    p, sph, pl, ks, pix, trace = _scene(name)
    t, gid, levels, colour_at = restate_chain(RS.flat_params(p), sph, pl, ks, pix)
    assert np.array_equal(t.view(np.uint32), trace["t"].view(np.uint32)) and np.array_equal(gid, trace["gid"])
    assert [int(levels[l]["exists"].sum()) for l in range(1, 5)] == trace["rays"]
    for l in range(1, 5):
        assert np.array_equal(levels[l]["gid"], trace["levels"][l]["gid"]) and np.array_equal(levels[l]["left"], trace["levels"][l]["left"])
    colour = RS.shade_chain(trace, [RS.reference_light()])
    for depth in (1, 2, 3, 4):
        want = colour_at(depth)
        for q in range(3):
            assert np.array_equal(colour[depth][q][trace["vis"]].view(np.uint32), want[q][trace["vis"]].view(np.uint32)), (depth, q)


@pytest.mark.parametrize("name", ["default", "mirror_floor"])
def test_depth_1_reproduces_the_lights_restatement(name):
    import test_gpu_lights as TL
    p, sph, pl, ks, pix, trace = _scene(name)
    lights = RS.light_set(3, zero=1, scale=0.6)
    with np.errstate(all="ignore"):
        t, gid, refl, colour = TL.restate(RS.flat_params(p), sph, pl, lights, pix, ks)
    assert np.array_equal(t.view(np.uint32), trace["t"].view(np.uint32)) and np.array_equal(gid, trace["gid"])
    assert np.array_equal(refl, trace["levels"][1]["exists"]) and refl.sum() > 1000
    got = RS.shade_chain(trace, lights)[1]
    for q in range(3):
        assert np.array_equal(got[q][trace["vis"]].view(np.uint32), colour[q][trace["vis"]].view(np.uint32)), q


# ---------------------------------------------------------------- 4. the inputs of tests/test_gpu_chain_lights.py

RAY_FLOORS = {"default": (500, 200, 50), "mirror_floor": (5000, 2000, 1000), "mirror_floor_shadows": (5000, 2000, 1000), "directed": (2000, 500, 100), "C2": (1000, 100, 20), "C3": (1000, 1000, 1000)}


@pytest.mark.parametrize("name", ["default", "mirror_floor", "mirror_floor_shadows", "directed", "C2", "C3"])
def test_rays_per_level(name):
    """Pixels with a ray at levels 1, 2, 3, 4 (the floors hold levels 2, 3, 4: the two whole-frame scenes keep those of
    tests/test_gpu_reflect_depth.py; the others ask for enough rays that a wrong deep term shows at many pixels):
      default scene, 320 x 180, every pixel:            8192,   624,  228,   55
      mirror floor, 320 x 180, every pixel:            33643,  5932, 2690, 1047  (the same with the floor at k = 0.6 for the shadow tests)
      directed scene, plane and sphere reflective:     42167,  5764, 1958,  486
      C2 floor+quarter, 40 000-pixel sample:            9230,  1900,  315,   68
      C3 room, 40 000-pixel sample:                     4839,  3708, 3311, 2433"""
    trace = _scene(name)[5]
    print(name, "rays per level", trace["rays"])
    lo = RAY_FLOORS[name]
    assert trace["rays"][1] >= lo[0] and trace["rays"][2] >= lo[1] and trace["rays"][3] >= lo[2], trace["rays"]
    assert trace["rays"][0] >= trace["rays"][1]


@pytest.mark.parametrize("which", list(RS.LIGHT_SETS))
@pytest.mark.parametrize("name", ["default", "mirror_floor", "C2", "C3"])
def test_light_sets_stay_below_the_clamp_and_their_order_shows(name, which):
    """With the powers of restate.LIGHT_SCALES every colour component stays below 255 on at least 5 % of the pixels that have a
    level-2 ray, at depths 2 and 4 (measured: on all of them, in all 16 pairs; the brightest component of any visible pixel is 127.5),
    so the clamp cannot hide the deep terms.  The deep terms show: depth 4 differs from depth 1 on most pixels with a level-2 ray.
    A set of two or more lights in reverse order gives other bits on at least 10 of those pixels (the GPU test compares every
    pixel bit for bit, so one would do; measured: 134 of 3708 on C3 with two lights, the fewest)."""
    p, sph, pl, ks, pix, trace = _scene(name)
    lights = RS.chain_lights(name, which)
    colour = RS.shade_chain(trace, lights)
    l2 = trace["levels"][2]["exists"]
    for depth in (2, 4):
        below = np.maximum.reduce(colour[depth])[l2] < f32(255.0)
        print(name, which, "depth", depth, "below the clamp: %d of %d" % (int(below.sum()), int(l2.sum())))
        assert below.sum() >= 0.05 * l2.sum()
    deep = np.logical_or.reduce([colour[4][q].view(np.uint32) != colour[1][q].view(np.uint32) for q in range(3)])[l2]
    assert deep.sum() >= 0.5 * l2.sum(), "depth 4 shows at %d of %d pixels" % (int(deep.sum()), int(l2.sum()))
    if len(lights) > 1:
        rev = RS.shade_chain(trace, lights[::-1])
        differs = np.logical_or.reduce([colour[4][q].view(np.uint32) != rev[4][q].view(np.uint32) for q in range(3)])[l2]
        print(name, which, "reversed order differs at %d of %d" % (int(differs.sum()), int(l2.sum())))
        assert differs.sum() >= 10


def shadow_sets(name, nl, depth=4):
    """For a shadow scene under its nl lights: (trace, lights, per pixel the set of lights float64 puts it in shadow from, decided
    for every light, ambiguous for some light)."""
    import test_gpu_lights as TL
    p, sph, pl, ks, pix, trace = _scene(name)
    lights = RS.shadow_lights(name, nl)
    vals = RS.values8(trace, RS.shade_chain(trace, lights)[depth])
    cls = [TL.classify64(p, trace["sph"], trace["pl"], vals, l.pos, pix) for l in lights]
    decided = np.logical_and.reduce([k >= 0 for k in cls])
    dset = sum(((k == 1).astype(np.int64) << i) for i, k in enumerate(cls))
    amb = np.logical_or.reduce([k == -1 for k in cls])
    return trace, lights, dset, decided, amb


@pytest.mark.parametrize("nl", [1, 2, 3])
@pytest.mark.parametrize("name", ["mirror_floor_shadows", "directed"])
def test_shadow_inputs(name, nl):
    """float64 (classify64 on the restatement's own distance and normal) over the 57 600 pixels of each frame:
      scene         lights  ambiguous  shadowed from exactly one  from two or more  level-2 ray and dark for some light
      mirror floor    1         4              6372                     -                 3712 of 5932
      mirror floor    2         6              5486                   2695                4244 of 5932
      mirror floor    3         9              6127                   4017                5022 of 5932
      directed        1         2              5914                     -                 2807 of 5764
      directed        2         2              4916                   2584                2807 of 5764
      directed        3         2              4876                   4210                2807 of 5764
    The floors: 1 % of the pixels shadowed from exactly one light, 1 % from two or more (sets of two or more), 1 % of the pixels
    with a level-2 ray dark for some light at level 0; ambiguous pixels at most 0.001 x lights x pixels.  And the dark set shows:
    on at least 1 % of the level-2 pixels the colour of the decided set differs from the colour of the empty set."""
    trace, lights, dset, decided, amb = shadow_sets(name, nl)
    n = trace["n"]
    l2 = trace["levels"][2]["exists"]
    count = np.array([bin(int(v)).count("1") for v in range(1 << nl)])[dset]
    one, more, dark2 = decided & (count == 1), decided & (count >= 2), decided & (count >= 1) & l2
    print(name, nl, "ambiguous", int(amb.sum()), "one", int(one.sum()), "two or more", int(more.sum()), "level 2 and dark", int(dark2.sum()), "of", int(l2.sum()))
    assert amb.sum() <= 0.001 * nl * n
    assert one.sum() >= 0.01 * n
    if nl >= 2:
        assert more.sum() >= 0.01 * n
    assert dark2.sum() >= 0.01 * l2.sum()
    lit = RS.shade_chain(trace, lights, 0)[4]
    shows = np.zeros(n, dtype=bool)
    for S in range(1, 1 << nl):
        c = RS.shade_chain(trace, lights, S)[4]
        shows |= (dset == S) & np.logical_or.reduce([c[q].view(np.uint32) != lit[q].view(np.uint32) for q in range(3)])
    print("the decided dark set shows on %d of the %d level-2 pixels" % (int((shows & dark2).sum()), int(l2.sum())))
    assert (shows & dark2).sum() >= 0.01 * l2.sum()


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_mirror_blend_shows_in_the_record_bytes(name):
    """On the record scenes (C1 with a quarter of its spheres reflective, whole; C2 floor+quarter, the 40 000-pixel sample) the
    blended colour and the local colour truncate to different bytes on at least 5 % of the visible pixels, under the reference's
    light at depths 1 and 3: a kernel that encoded the unblended colour would write other records."""
    if name == "C1":
        p, sph, pl = RS.config_case("C1")
        pix = np.arange(int(p.x) * int(p.y))
        trace = RS.trace_chain(p, sph, pl, RS._scene_k("C1", sph, pl, "quarter"), pix)
    else:
        p, sph, pl, ks, pix, trace = _scene("C2")
    lights = RS.record_lights(3)
    colour = RS.shade_chain(trace, lights)
    with np.errstate(all="ignore"):
        L0 = trace["levels"][0]
        local = RS._shade_lights(L0["O"], L0["D"], L0["t"], L0["normal"], L0["od"], lights)
    vis = trace["vis"] & (trace["t"] <= f32(p.cam_far))
    for depth in (1, 3):
        differs = np.logical_or.reduce([RS._u8_sat(colour[depth][q]) != RS._u8_sat(local[q]) for q in range(3)]) & vis
        print(name, "depth", depth, "blend shows in the bytes of %d of %d visible pixels" % (int(differs.sum()), int(vis.sum())))
        assert differs.sum() >= 0.05 * vis.sum()


def test_fuzz_seeds_reach_deep_levels():
    """The 12 fixed seeds of the fuzzed GPU test together: at least 40 000 visible sampled pixels, 5000 level-1 rays, 500 level-2
    rays and 50 level-4 rays, so that the comparison is not one of empty frames."""
    vis, rays = 0, np.zeros(4, dtype=np.int64)
    for seed in RS.FUZZ_SEEDS:
        p, sph, pl, k, lights, pix = F.chain_inputs(seed)
        assert len(sph) <= 700 and len(pix) <= 8000 and 1 <= len(lights) <= 3 and (k > 0).any()
        trace = RS.trace_chain(p, sph, pl, k, pix)
        vis += int(trace["vis"].sum())
        rays += np.array(trace["rays"])
    print("fuzz seeds: visible", vis, "rays per level", rays.tolist())
    assert vis >= 40000 and rays[0] >= 5000 and rays[1] >= 500 and rays[3] >= 50
