"""Worlds that are not y-up: the same scene in five orientations (helper, no test).

A rigid rotation of the whole world -- bodies, plane, static boxes, gravity -- changes nothing about the physics, but it moves
the scene onto other branches of everything in the product that tells (x, z) from y: safe-zone discs, the hashed column grid,
the `ballistic` predicate, the per-tile "lateral axis fixed" words, AABB tests, the hull filter.  ODE's own convention is z-up.

Each orientation is a unit quaternion qR (w, x, y, z) with its matrix R.  The four signed permutations move and negate
components -- no float matrix is multiplied in -- so their vectors are exact images; `tilted` is a general rotation.  Everything
is rotated in float64 and rounded to the world's precision afterwards, so the device and the oracle get identical numbers."""
import dataclasses
import math

import numpy as np

H = 1.0 / 60.0
GRAVITY = (0.0, -9.8, 0.0)

_T = math.radians(50.0) / 2.0
_AX = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
QUATS = {
    "y_up": (1.0, 0.0, 0.0, 0.0),                      # control
    "z_up": (0.5, 0.5, 0.5, 0.5),                      # x -> y -> z -> x: gravity (0, 0, -g), plane (0, 0, 1, d)
    "x_up": (0.5, -0.5, -0.5, -0.5),                   # the inverse permutation: gravity (-g, 0, 0)
    "down": (0.0, 1.0, 0.0, 0.0),                      # 180 degrees about x: gravity (0, +g, 0), plane (0, -1, 0, d)
    "tilted": (math.cos(_T), *(math.sin(_T) * _AX)),   # 50 degrees about (1, 2, 3) / sqrt 14: nothing axis-aligned
}
# (R v)[i] = sign[i] * v[perm[i]]
_PERM = {"y_up": ((0, 1, 2), (1.0, 1.0, 1.0)), "z_up": ((2, 0, 1), (1.0, 1.0, 1.0)),
         "x_up": ((1, 2, 0), (1.0, 1.0, 1.0)), "down": ((0, 1, 2), (1.0, -1.0, -1.0))}
ORIENTATIONS = tuple(QUATS)
ROTATED = ORIENTATIONS[1:]


def quat_matrix(q):
    w, x, y, z = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def matrix(name):
    """R as a float64 matrix (exact for the signed permutations)"""
    if name in _PERM:
        perm, sign = _PERM[name]
        R = np.zeros((3, 3))
        for i in range(3):
            R[i, perm[i]] = sign[i]
        return R
    return quat_matrix(QUATS[name])


def _rows(name, a, inverse=False):
    """R (or its transpose) applied along the first axis of `a` (3 x ...), float64"""
    a = np.asarray(a, dtype=np.float64)
    if name in _PERM:
        perm, sign = _PERM[name]
        out = np.empty_like(a)
        for i in range(3):
            if inverse:
                out[perm[i]] = sign[i] * a[i]
            else:
                out[i] = sign[i] * a[perm[i]]
        return out
    R = matrix(name)
    return np.tensordot(R.T if inverse else R, a, axes=(1, 0))


def rotate_vectors(name, v, inverse=False):
    """rows of `v` (n x 3, or one 3-vector) -> R v"""
    v = np.asarray(v, dtype=np.float64)
    return _rows(name, v.T, inverse).T


def _quat_mul(a, b):
    """a (one quaternion) times the rows of b (n x 4)"""
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = np.asarray(b, dtype=np.float64).T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def _round(v, dtype):
    return tuple(float(np.dtype(dtype).type(c)) for c in v)


def rotate_static(name, box, dtype=np.float64):
    """one static box (sides3, pos3, R12): the centre moves, the 3 x 3 part of the 3 x 4 matrix becomes R M"""
    sz, at, R12 = box
    M = np.asarray(R12, dtype=np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    out[:, :3] = _rows(name, M[:, :3])
    return (tuple(sz), _round(rotate_vectors(name, at), dtype), list(_round(out.ravel(), dtype)))


def rotate_plane(name, plane, dtype=np.float64):
    return _round((*rotate_vectors(name, plane[:3]), plane[3]), dtype)


def rotate_gravity(name, gravity=GRAVITY, dtype=np.float64):
    return _round(rotate_vectors(name, gravity), dtype)


def rotate_scene(scene, name, dtype=None, gravity=GRAVITY):
    """-> (scene', gravity'): the scene and the gravity vector turned by orientation `name`, in precision `dtype` (default: the
    scene's own).  Body-frame data (hull points and faces, sides, mass, inertia) is unchanged."""
    dtype = np.dtype(scene.pos.dtype if dtype is None else dtype)
    rotated = dataclasses.replace(
        scene,
        pos=rotate_vectors(name, scene.pos), lvel=rotate_vectors(name, scene.lvel),
        avel=rotate_vectors(name, scene.avel),                       # angular velocity is world-frame
        quat=_quat_mul(QUATS[name], scene.quat),
        plane=None if scene.plane is None else rotate_plane(name, scene.plane, dtype),
        static_boxes=None if scene.static_boxes is None else [rotate_static(name, b, dtype) for b in scene.static_boxes])
    return rotated.astype(dtype), rotate_gravity(name, gravity, dtype)


def rotate_back(state, name):
    """(pos, quat, lvel, avel) of a rotated world, expressed in the y-up frame again (float64)"""
    pos, quat, lvel, avel = state
    w, x, y, z = QUATS[name]
    return (rotate_vectors(name, pos, True), _quat_mul((w, -x, -y, -z), quat), rotate_vectors(name, lvel, True),
            rotate_vectors(name, avel, True))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's side of a scene, as tests/test_gpu_fuzz.py::test_random_scene_matches_oracle sets it up, plus gravity
# ---------------------------------------------------------------------------------------------------------------------
GEOM_SPHERE, GEOM_BOX, GEOM_CONVEX = 1, 2, 3


def oracle_world(scene, dtype, params=None, gravity=GRAVITY, exact=False, sphere_hull=True):
    """an oracle world holding `scene` (body by body: geometry classes may be interleaved); params: the fuzz scenes' dict
    (iters, sor_w, erp, cfm, gyro, mu, bounce_on, bounce, bounce_vel, max_contacts), None = the oracle's defaults;
    sphere_hull=False: category / collide bits that keep spheres and hulls from meeting one another (nothing else changes)"""
    from oracle.orc_ctypes import CONTACT_BOUNCE, Oracle
    orc = Oracle(dtype)
    lib = orc.lib
    ow = orc.world(gravity=gravity)
    ow.set_stepper(exact)
    if params is not None:
        p = params
        lib.orc_world_set_quickstep(ow.w, p["iters"], p["sor_w"]); lib.orc_world_set_erp(ow.w, p["erp"])
        lib.orc_world_set_cfm(ow.w, p["cfm"]); lib.orc_world_set_gyro_mode(ow.w, p["gyro"])
        lib.orc_world_set_surface(ow.w, CONTACT_BOUNCE if p["bounce_on"] else 0, p["mu"], p["bounce"], p["bounce_vel"])
        lib.orc_world_set_max_contacts(ow.w, p["max_contacts"])
    if scene.plane is not None:
        ow.add_plane(*scene.plane)
    if scene.hull_points is not None:
        ow.set_hull(scene.hull_points)
        ow.set_hull_faces(scene.hull_planes)
    for sz, at, R12 in (scene.static_boxes or []):
        ow.add_static_box(sz, at, R12)
    for i in range(scene.n):
        b = lib.orc_body_create(ow.w)
        lib.orc_body_set_position(ow.w, b, *scene.pos[i])
        _, qp = orc.arr(scene.quat[i]); lib.orc_body_set_quaternion(ow.w, b, qp)
        lib.orc_body_set_linear_vel(ow.w, b, *scene.lvel[i])
        lib.orc_body_set_angular_vel(ow.w, b, *scene.avel[i])
        _, ip = orc.arr(np.diag(scene.inertia[i]).ravel()); lib.orc_body_set_mass(ow.w, b, scene.mass[i, 0], ip)
        gt = scene.gtype[i]
        g = (lib.orc_geom_create_sphere(ow.w, scene.sides[i, 0]) if gt == GEOM_SPHERE
             else lib.orc_geom_create_convex(ow.w) if gt == GEOM_CONVEX
             else lib.orc_geom_create_box(ow.w, *scene.sides[i]))
        if sphere_hull:
            cat, col = 2, 3
        else:                  # boxes 2, hulls 4, spheres 8: everything meets the statics (1) and the boxes, spheres never a hull
            cat, col = {GEOM_BOX: (2, 15), GEOM_CONVEX: (4, 7), GEOM_SPHERE: (8, 11)}[int(gt)]
        lib.orc_geom_set_category_bits(ow.w, g, cat); lib.orc_geom_set_collide_bits(ow.w, g, col)
        lib.orc_geom_set_body(ow.w, g, b)
    return ow


def device_world(pkg, scene, dtype, params=None, gravity=GRAVITY):
    """the device's side of the same: a BatchWorld with the fuzz scenes' parameters and this gravity, scene loaded"""
    w = pkg.BatchWorld(scene.n, dtype=dtype, gravity=gravity)
    if params is not None:
        p = params
        w.set_quickstep(p["iters"], p["sor_w"]); w.set_erp(p["erp"]); w.set_cfm(p["cfm"]); w.set_gyro_mode(p["gyro"])
        w.set_surface(pkg.batch.CONTACT_BOUNCE if p["bounce_on"] else 0, p["mu"], p["bounce"], p["bounce_vel"])
        w.set_max_contacts(p["max_contacts"])
    w.load_scene(scene)
    return w
