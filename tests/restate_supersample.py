"""RTX_OPT_SUPERSAMPLE's fold (include/rtx.h) restated in numpy, exactly as worded there: per cell the n = S x S samples in the
order k = j S + i, vis_k = distance_k <= cam_far, the minimum distance of the visible ones, and for each of the seven other floats
sequential fp32 adds of (vis_k ? v_k : 0.0f) from 0.0f, then ONE fp32 multiply by 1.0f / (float)n.  Step 3, the encoding, is
restate.encode_records / encode_words of the folded values."""
import numpy as np

import restate as RS

f32 = np.float32
NO_HIT = f32(99999999.0)


def sample_params(p, S):
    """p' of the rule: a copy of the params `p` (the oracle's or the library's struct) with x = S W and y = S H, nothing else touched."""
    q = type(p).from_buffer_copy(p)
    q.x, q.y = S * int(p.x), S * int(p.y)
    return q


def case_params(O, W, H, S, pos, far, rot=None):
    """(p, p') of a test case of W x H cells at S x S samples: p' is the camera of an S W x S H frame at `pos` (oracle.camera_params, whose
    element1 follows the frame's height) with cam_far = far, and p is p' with x = W, y = H -- so that p' is p with x = S W, y = S H."""
    ps = O.camera_params(S * W, S * H, pos=pos) if rot is None else O.camera_params(S * W, S * H, pos=pos, rot=rot)
    ps.cam_far = far
    p = type(ps).from_buffer_copy(ps)
    p.x, p.y = W, H
    assert bytes(sample_params(p, S)) == bytes(ps)
    return p, ps


def fold(samples, W, rows, S, cam_far, order=None):
    """samples: the RTX_RENDER_VALUES floats of S rows sample rows of S W samples -> (rows * W, 8) folded values, column W-1 all 0.
    `order`: the samples' order in the sums, a permutation of range(S * S) (None: the rule's, k = 0 .. n - 1)."""
    n = S * S
    s = np.ascontiguousarray(samples, dtype=np.float32).reshape(S * rows, S * W, 8)
    cells = s[:, :S * (W - 1)].reshape(rows, S, W - 1, S, 8)  # [row, j, col, i]
    acc = np.zeros((rows, W - 1, 7), dtype=np.float32)
    nearest = np.full((rows, W - 1), np.inf, dtype=np.float32)
    m = np.zeros((rows, W - 1), dtype=np.int64)
    for k in (range(n) if order is None else order):
        j, i = divmod(k, S)
        v = cells[:, j, :, i]
        with np.errstate(invalid="ignore"):
            vis = v[..., 0] <= f32(cam_far)
            nearest = np.where(vis & (v[..., 0] < nearest), v[..., 0], nearest)
            acc = (acc + np.where(vis[..., None], v[..., 1:], f32(0.0))).astype(np.float32)
        m += vis
    out = np.zeros((rows, W, 8), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        out[:, :W - 1, 1:] = acc * (f32(1.0) / f32(n))
    out[:, :W - 1, 0] = np.where(m > 0, nearest, NO_HIT)
    out[:, :W - 1, 1:][m == 0] = f32(0.0)
    return out.reshape(rows * W, 8)


def expected(samples, W, rows, S, mode, cam_far):
    """(values (rows * W, 8), records (rows * W, 12 or 20) uint8, words (rows * W) uint32) of the folded frame."""
    v = fold(samples, W, rows, S, cam_far)
    return v, RS.encode_records(v, mode, cam_far), RS.encode_words(v, mode, cam_far)


def cell_classes(distance, hit, W, H, S, cam_far):
    """The kinds of cells of a sample frame (distance, hit: (S H, S W) arrays of the samples): a dict of boolean (H, W - 1) arrays.
    none: no visible sample and no hit; all: every sample visible; some: some but not all; edge: a visible sample beside a hit
    beyond cam_far in the same cell; beyond: hits only beyond cam_far."""
    d = np.asarray(distance, dtype=np.float32)[:, :S * (W - 1)].reshape(H, S, W - 1, S)
    h = np.asarray(hit)[:, :S * (W - 1)].reshape(H, S, W - 1, S) != 0
    vis = d <= f32(cam_far)
    far_hit = h & ~vis
    m = vis.sum(axis=(1, 3))
    return {"none": (m == 0) & ~h.any(axis=(1, 3)), "all": m == S * S, "some": (m > 0) & (m < S * S),
            "edge": (m > 0) & far_hit.any(axis=(1, 3)), "beyond": (m == 0) & far_hit.any(axis=(1, 3))}
