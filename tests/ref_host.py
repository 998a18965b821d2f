"""Cases for the host build of the reference's own sources (oracle/ref_host/, built by oracle/Makefile into
oracle/_ref/ref_driver and ref_driver_pinpow): write a case file, run the binary as a child process, parse what it wrote.

The binary is `ref_driver CASE_FILE RESULT_FILE`.  Both files are plain little-endian data:

  case    u32 magic 0x43585452 ("RTXC"), u32 kind, then by kind
    0 UPDATE    u32 W, H, mode, scene_src, params_src, nobj, nsteps, 0
                f32[22] params: params_src 0 = raw (inverse view matrix 16 row-major, cam pos 3, element1, element2, far);
                                params_src 1 = Camera3D (pos 3, rot 3, rest ignored: SetPos, SetRot, Init, Update)
                nobj x OBJECT (60 bytes: i32 type (1 plane, 2 sphere), f32 center[3], color[3], radius, i32 mover, f32 speed,
                               f32 normal[3] (as given to CreatePlane, not normalised), width, height), in creation order;
                               scene_src 0 = created with Scene3D::CreateSphere / CreatePlane in that order,
                               scene_src 1 = Scene3D::Init's fixed scene (the six records then only carry mover and speed)
                f64[nsteps] dt: RayTracingManager::Update is called once per entry
    1 MINIMIZE  u32 W, H, mode, 0;  u8[20*W*H] the host result array;  MinimizeResults alone
    2 ANSI256   nothing
    3 CAMERA    u32 W, H, n, 0;  n x f32[6] (pos 3, rot 3)

  result
    0 UPDATE    u32 magic, W, H, nsteps, nobj, 0;  f32[22] the params used (raw layout);  then per step
                nobj x (f32 center.y, i32 mover (0 for a plane)),  u8[20*W*H] the host result array,
                u64 n, u8[n] the bytes handed to PrintMachine::SetDataInBackBuffer
    1 MINIMIZE  u32 magic, 0;  u64 n;  u8[n]
    2 ANSI256   u8[2^24]: ansi256_from_rgb of every packed 0xRRGGBB
    3 CAMERA    n x f32[22] (raw layout)

The reference's directory itself is only needed to build the binaries; nothing here reads it.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

import oracle as O

REF_OUT = os.path.join(O.ORACLE_DIR, "_ref")
STOCK = os.path.join(REF_OUT, "ref_driver")
PINPOW = os.path.join(REF_OUT, "ref_driver_pinpow")
DEFAULT_REF_DIR = "/root/reference/ConsoleProject"   # oracle/Makefile's REF_DIR default

MAGIC = 0x43585452
OBJECT_DTYPE = np.dtype([("type", "<i4"), ("center", "<f4", 3), ("color", "<f4", 3), ("radius", "<f4"), ("mover", "<i4"),
                         ("speed", "<f4"), ("normal", "<f4", 3), ("width", "<f4"), ("height", "<f4")])
assert OBJECT_DTYPE.itemsize == 60
STATE_DTYPE = np.dtype([("y", "<f4"), ("mover", "<i4")])


def ref_dir():
    return os.environ.get("REF_DIR", DEFAULT_REF_DIR)


def have_binaries():
    return os.path.exists(STOCK) and os.path.exists(PINPOW)


def have_reference():
    return os.path.isdir(ref_dir())


def availability():
    """(usable, message): the rule of tests/test_ref_host.py.  Binary there: run.  Binary and reference both absent: skip, naming
    both.  Reference there but no binary: that is a broken build, and the caller fails."""
    if have_binaries():
        return True, ""
    msg = "no %s and no %s" % (STOCK, PINPOW) if not os.path.exists(STOCK) else "no %s" % PINPOW
    return False, "%s; reference directory %s %s" % (msg, ref_dir(), "exists" if have_reference() else "does not exist either")


def objects(n):
    return np.zeros(n, dtype=OBJECT_DTYPE)


def sphere(radius, pos, color, mover=-1, speed=1.0):
    o = objects(1)
    o["type"], o["center"], o["color"], o["radius"], o["mover"], o["speed"] = O.SPHERE, pos, color, radius, mover, speed
    return o


def plane(pos, normal, color, width, height):
    o = objects(1)
    o["type"], o["center"], o["color"], o["normal"], o["width"], o["height"] = O.PLANE, pos, color, normal, width, height
    return o


def from_arrays(sph, pl, order=None, movers=None, speeds=None):
    """Spheres (N,7) and planes (M,11) as fuzz_cases.scene() makes them -> object records.  `order`: a permutation of
    range(N+M) (indices into spheres-then-planes) giving the creation order; default spheres first."""
    sph = np.asarray(sph, dtype=np.float32).reshape(-1, 7)
    pl = np.asarray(pl, dtype=np.float32).reshape(-1, 11)
    o = objects(len(sph) + len(pl))
    s, p = o[:len(sph)], o[len(sph):]
    s["type"], s["center"], s["radius"], s["color"] = O.SPHERE, sph[:, 0:3], sph[:, 3], sph[:, 4:7]
    s["mover"] = -1 if movers is None else movers
    s["speed"] = 1.0 if speeds is None else speeds
    p["type"], p["center"], p["normal"], p["color"], p["width"], p["height"] = O.PLANE, pl[:, 0:3], pl[:, 3:6], pl[:, 6:9], pl[:, 9], pl[:, 10]
    return o if order is None else o[np.asarray(order)]


DEFAULT_SCENE = np.concatenate([
    sphere(7.0, (0.0, 10.0, 20.0), (255.0, 1.0, 1.0)), sphere(6.0, (5.0, 10.0, 20.0), (1.0, 255.0, 1.0)),
    sphere(10.0, (10.0, 10.0, 40.0), (1.0, 1.0, 255.0)), sphere(3.0, (5.0, 10.0, 20.0), (225.0, 210.0, 20.0)),
    sphere(4.0, (-5.0, 10.0, 40.0), (225.0, 10.0, 220.0)),
    plane((0.0, -3.0, 30.0), (0.0, 1.0, 0.0), (100.0, 100.0, 100.0), 10, 20)])   # Scene3D.cpp:28-33


def oracle_scene(objs):
    """The oracle's scene of the same records, in the same creation order."""
    sc = O.Scene()
    for o in objs:
        if o["type"] == O.SPHERE:
            sc.add_sphere(o["radius"], o["center"], o["color"], mover=int(o["mover"]), speed=float(o["speed"]))
        else:
            sc.add_plane(o["center"], o["normal"], o["color"], o["width"], o["height"])
    return sc


def raw_params(inv_v, cam, e1, e2, far):
    v = np.zeros(22, dtype=np.float32)
    v[0:16] = np.asarray(inv_v, dtype=np.float32).reshape(16)
    v[16:19] = cam
    v[19:22] = e1, e2, far
    return v


def raw_of_oracle_params(p):
    return raw_params(np.array(p.inv_v, dtype=np.float32), p.cam_pos[:], p.element1, p.element2, p.cam_far)


def oracle_params_of_raw(v, w, h):
    return O.params_from_arrays(v[0:16], v[16:19], w, h, v[19], v[20], v[21])


def _run(binary, case_bytes):
    if not os.path.exists(binary):
        raise FileNotFoundError(binary)
    with tempfile.TemporaryDirectory(prefix="ref_host_") as d:
        cpath, rpath = os.path.join(d, "case.bin"), os.path.join(d, "result.bin")
        with open(cpath, "wb") as f:
            f.write(case_bytes)
        r = subprocess.run([binary, cpath, rpath], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("%s exited with %d: %s" % (os.path.basename(binary), r.returncode, r.stderr.decode(errors="replace").strip()))
        with open(rpath, "rb") as f:
            return f.read()


class UpdateResult:
    """params: f32[22] as used; per step: states[k] (y, mover per object), frames[k] (u8[20*W*H]), streams[k] (u8[n])."""

    def __init__(self, params, states, frames, streams):
        self.params, self.states, self.frames, self.streams = params, states, frames, streams


def update(objs, w, h, mode, params, dts=(0.0,), camera=False, init_scene=False, binary=None):
    """RayTracingManager::Update once per dt.  params: f32[22] raw, or with camera=True (pos, rot) for Camera3D."""
    pv = np.zeros(22, dtype=np.float32)
    if camera:
        pv[0:3], pv[3:6] = params[0], params[1]
    else:
        pv[:] = params
    objs = np.ascontiguousarray(objs, dtype=OBJECT_DTYPE)
    dts = np.asarray(dts, dtype="<f8")
    case = struct.pack("<10I", MAGIC, 0, w, h, mode, 1 if init_scene else 0, 1 if camera else 0, len(objs), len(dts), 0)
    out = _run(binary or STOCK, case + pv.tobytes() + objs.tobytes() + dts.tobytes())
    magic, rw, rh, nsteps, nobj, _ = struct.unpack_from("<6I", out, 0)
    if (magic, rw, rh, nsteps, nobj) != (MAGIC, w, h, len(dts), len(objs)):
        raise RuntimeError("unexpected result header %r" % ((magic, rw, rh, nsteps, nobj),))
    at = 24
    used = np.frombuffer(out, dtype="<f4", count=22, offset=at).copy()
    at += 88
    states, frames, streams = [], [], []
    for _ in range(nsteps):
        states.append(np.frombuffer(out, dtype=STATE_DTYPE, count=nobj, offset=at).copy())
        at += 8 * nobj
        frames.append(np.frombuffer(out, dtype=np.uint8, count=20 * w * h, offset=at).copy())
        at += 20 * w * h
        n, = struct.unpack_from("<Q", out, at)
        at += 8
        streams.append(np.frombuffer(out, dtype=np.uint8, count=n, offset=at).copy())
        at += n
    if at != len(out):
        raise RuntimeError("result file has %d bytes, parsed %d" % (len(out), at))
    return UpdateResult(used, states, frames, streams)


def minimize(mode, buf, w, h, binary=None):
    """RayTracingManager::MinimizeResults alone on a 20*W*H host array (shorter input is zero-padded, as the array is)."""
    full = np.zeros(20 * w * h, dtype=np.uint8)
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    full[:buf.size] = buf
    out = _run(binary or STOCK, struct.pack("<6I", MAGIC, 1, w, h, mode, 0) + full.tobytes())
    n, = struct.unpack_from("<Q", out, 8)
    if len(out) != 16 + n:
        raise RuntimeError("result file has %d bytes, header says %d" % (len(out), 16 + n))
    return np.frombuffer(out, dtype=np.uint8, count=n, offset=16).copy()


def ansi256_table(binary=None):
    out = _run(binary or STOCK, struct.pack("<2I", MAGIC, 2))
    if len(out) != 1 << 24:
        raise RuntimeError("ansi256 table has %d bytes" % len(out))
    return np.frombuffer(out, dtype=np.uint8)


def camera(w, h, poses, binary=None):
    """Camera3D's params for each (pos, rot): (n, 22) float32, raw layout."""
    pr = np.asarray([list(p) + list(r) for p, r in poses], dtype="<f4").reshape(-1, 6)
    out = _run(binary or STOCK, struct.pack("<6I", MAGIC, 3, w, h, len(pr), 0) + pr.tobytes())
    return np.frombuffer(out, dtype="<f4").reshape(len(pr), 22).copy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))
