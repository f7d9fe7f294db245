"""Populations of ISOLATED geom pairs in adversarial poses, for one-tick parity of the narrowphase (no tests in here).

tests/test_collider_geometry.py certifies the oracle's colliders against brute-force geometry on random pairs drawn by regime;
tests/test_pair_population.py checks that the populations below cover those regimes (by the oracle alone, no GPU).  They are made
for a one-tick comparison of the device with the oracle, body by body and bit for bit: a contact that is wrong in position, normal,
depth, count or order changes the velocity of its two bodies and of nothing else, so a mismatch names its pair.

Layout: pair k is bodies 2k, 2k + 1 in lattice cell k (8 m pitch in x and z: the largest pair spans 7.2 m, so nothing reaches
another cell); velocities zero, mass 1, inertia identity, gravity on, orientations given as quaternions.  For pairs of two
classes the class in the lower slot alternates with k (dCollide swaps the collider's arguments and negates the normal for one
of the two orders).  Every generator is seeded; every population is float64 and is cast / translated by `scene()`.

The single-body populations (`on_plane`, `on_statics`) have one body per cell.  `on_statics` cannot keep the 8 m pitch: 512 bodies
out to +-40 m on the 100 m floor need less; its bodies keep >= 2.1 m between centres (the largest body is 1.74 m across), and the
test asserts from the oracle's joints that no contact joins two bodies."""
import ctypes as C
import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from __graft_entry__ import load_package
from oracle.orc_ctypes import Oracle

pkg = load_package()
SPHERE, BOX, CONVEX = pkg.scenes.GEOM_SPHERE, pkg.scenes.GEOM_BOX, pkg.scenes.GEOM_CONVEX
CLASS_NAME = {SPHERE: "sphere", BOX: "box", CONVEX: "hull"}
PITCH = 8.0
H = 1.0 / 60.0
FAR = (4096.0, 0.0, -2560.0)                       # the translation of the "far from the origin" runs
PLANE = (0.1, 1.0, -0.07, 0.2)                     # a tilted ground plane given with a non-unit normal
HULL_SHAPES = ("tetra", "cube", "ell63", "ell64", "ell65", "ell150")


# ---- random rotations and the box-box regimes: shared with tests/test_collider_geometry.py, which draws the same numbers from them
def _rand_rot(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.empty((n, 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _small_rot(rng, n, angle):
    """rotations by `angle` radians (scalar or per-pair) about random axes: boxes with near-parallel edges"""
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    a = np.broadcast_to(np.asarray(angle, float), (n,))
    K = np.zeros((n, 3, 3))
    K[:, 0, 1] = -ax[:, 2]; K[:, 0, 2] = ax[:, 1]; K[:, 1, 0] = ax[:, 2]; K[:, 1, 2] = -ax[:, 0]; K[:, 2, 0] = -ax[:, 1]; K[:, 2, 1] = ax[:, 0]
    return np.eye(3)[None] + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)


def _boxbox_cases(rng, n):
    """three regimes: generic pairs near contact; near-parallel edges (tiny relative rotation); a floor-sized box under a small one"""
    n1, n2 = n // 2, n // 4
    n3 = n - n1 - n2
    s1 = rng.uniform(0.2, 1.0, (n, 3)); s2 = rng.uniform(0.2, 1.0, (n, 3))
    R1 = _rand_rot(rng, n); R2 = _rand_rot(rng, n)
    R2[n1:n1 + n2] = _small_rot(rng, n2, 10.0 ** rng.uniform(-9, -2, n2)) @ R1[n1:n1 + n2]
    p1 = rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    reach = 0.5 * (np.linalg.norm(s1, axis=1) + np.linalg.norm(s2, axis=1))
    p2 = p1 + d * (rng.uniform(0.15, 1.0, n) * reach)[:, None]
    # the reference's floor (main.c:115): 100 x 1 x 100, a spawned box resting on / sunk into / hovering over its top
    a = n1 + n2
    s2[a:] = [100.0, 1.0, 100.0]
    R2[a:] = np.eye(3)
    R1[a:] = _small_rot(rng, n3, rng.choice([0.0, 1e-7, 1e-3, 0.3], n3)) @ np.eye(3)
    p2[a:] = 0.0
    p1[a:, 0] = rng.uniform(-40, 40, n3); p1[a:, 2] = rng.uniform(-40, 40, n3)
    p1[a:, 1] = 0.5 + 0.5 * s1[a:, 1] + rng.uniform(-0.05, 0.02, n3)
    return p1, R1, s1, p2, R2, s2


# ------------------------------------------------------------------------------------------------------------ hull shapes
@dataclass
class HullShape:
    name: str
    points: np.ndarray        # body frame (pkg.hull.build's)
    planes: np.ndarray        # nf x 4
    radius: float


def _ellipsoid(n):
    """n points on the ellipsoid with semi-axes 0.5, 0.35, 0.4 (a Fibonacci spiral): every one is a vertex of the hull"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.column_stack([r * np.cos(phi), r * np.sin(phi), z]) * [0.5, 0.35, 0.4]


@functools.lru_cache(maxsize=None)
def hull_shape(name):
    if name == "tetra":
        pts = 0.45 * np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], float)
    elif name == "cube":                                # the 0.8 m cube: its face triangles are coplanar in pairs
        pts = np.array(list(itertools.product((-0.4, 0.4), repeat=3)), float)
    elif name.startswith("ell"):                        # ell63 / ell64 / ell65: a 64-point pass ends one short, exactly, one over
        pts = _ellipsoid(int(name[3:]))
    else:
        raise KeyError(name)
    h = pkg.hull.build(pts)
    assert len(h.points) == len(pts), (name, len(h.points))
    return HullShape(name, h.points.copy(), pkg.hull.planes(h.points), float(h.radius))


# ------------------------------------------------------------------------------------------------------------ population
@dataclass
class Population:
    name: str
    pos: np.ndarray
    quat: np.ndarray
    sides: np.ndarray
    gtype: np.ndarray
    cell: np.ndarray                      # body -> cell index (a pair's two bodies share it)
    cell_pitch: float = PITCH
    plane: Optional[tuple] = None
    static_boxes: Optional[list] = None   # [(sides3, pos3, R12)]
    hull: Optional[HullShape] = None
    notes: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.pos)

    @property
    def paired(self):
        return self.n == 2 * (int(self.cell.max()) + 1)

    def first(self, n_bodies):
        """the population's first n_bodies slots (whole cells)"""
        n = min(int(n_bodies), self.n)
        return Population(self.name, self.pos[:n], self.quat[:n], self.sides[:n], self.gtype[:n], self.cell[:n], self.cell_pitch,
                          self.plane, self.static_boxes, self.hull, self.notes)

    def scene(self, dtype, shift=None):
        """a scenes.Scene in `dtype`, the whole world translated by `shift` (plane and static boxes with it)"""
        s = np.zeros(3) if shift is None else np.asarray(shift, float)
        n = self.n
        plane = None
        if self.plane is not None:
            a, b, c, d = self.plane
            plane = (a, b, c, d + float(np.dot((a, b, c), s)))
        statics = None
        if self.static_boxes:
            statics = [(tuple(sz), tuple(float(v) for v in np.asarray(at, float) + s), list(R12)) for sz, at, R12 in self.static_boxes]
        hp = None if self.hull is None else self.hull.points
        hpl = None if self.hull is None else self.hull.planes
        return pkg.scenes.Scene(self.pos + s, self.quat, np.zeros((n, 3)), np.zeros((n, 3)), np.ones((n, 1)), np.ones((n, 3)),
                                self.sides, self.gtype, plane, hp, hpl, statics).astype(dtype)

    def describe(self, cells, scene=None):
        """everything needed to rebuild the bodies of `cells` alone: classes in slot order, poses and sizes as repr"""
        out = []
        for c in cells:
            ids = np.flatnonzero(self.cell == c)
            out.append(f"cell {int(c)} of {self.name}: slots {ids.tolist()} classes {[CLASS_NAME[int(self.gtype[i])] for i in ids]}")
            for i in ids:
                p = self.pos[i] if scene is None else scene.pos[i]
                q = self.quat[i] if scene is None else scene.quat[i]
                sd = self.sides[i] if scene is None else scene.sides[i]
                out.append(f"  slot {int(i)} {CLASS_NAME[int(self.gtype[i])]}: pos={p!r} quat={q!r} sides={sd!r}")
        return "\n".join(out)


def _quat_from_R(R):
    """(n, 3, 3) rotations -> (n, 4) unit quaternions (w, x, y, z), by the largest of the four squared components"""
    n = len(R)
    t = np.stack([1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2],
                  1 - R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], 1 - R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]], axis=1)
    k = np.argmax(t, axis=1)
    q = np.empty((n, 4))
    a = np.arange(n)
    s = 2.0 * np.sqrt(t[a, k])
    rows = [np.stack([0.25 * s, (R[:, 2, 1] - R[:, 1, 2]) / s, (R[:, 0, 2] - R[:, 2, 0]) / s, (R[:, 1, 0] - R[:, 0, 1]) / s], 1),
            np.stack([(R[:, 2, 1] - R[:, 1, 2]) / s, 0.25 * s, (R[:, 0, 1] + R[:, 1, 0]) / s, (R[:, 0, 2] + R[:, 2, 0]) / s], 1),
            np.stack([(R[:, 0, 2] - R[:, 2, 0]) / s, (R[:, 0, 1] + R[:, 1, 0]) / s, 0.25 * s, (R[:, 1, 2] + R[:, 2, 1]) / s], 1),
            np.stack([(R[:, 1, 0] - R[:, 0, 1]) / s, (R[:, 0, 2] + R[:, 2, 0]) / s, (R[:, 1, 2] + R[:, 2, 1]) / s, 0.25 * s], 1)]
    for j in range(4):
        q[k == j] = rows[j][k == j]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q


def _cell_origin(k, pitch=PITCH, per_row=64):
    k = np.asarray(k)
    return np.stack([(k % per_row) * pitch, np.zeros(len(k)), (k // per_row) * pitch], axis=1)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _interleave(name, first, second, swap, **kw):
    """pairs (first[k], second[k]) -> bodies 2k, 2k+1; where swap[k] the two trade slots.  first / second: (pos, R, sides, class)"""
    n = len(first[0])
    pos = np.empty((2 * n, 3)); quat = np.empty((2 * n, 4)); sides = np.zeros((2 * n, 3)); gt = np.empty(2 * n, np.uint8)
    lo = np.where(swap, 1, 0) + 2 * np.arange(n)
    hi = np.where(swap, 0, 1) + 2 * np.arange(n)
    org = _cell_origin(np.arange(n))
    for idx, (p, R, s, cls) in ((lo, first), (hi, second)):
        pos[idx] = p + org; quat[idx] = _quat_from_R(R); sides[idx] = s; gt[idx] = cls
    return Population(name, pos, quat, sides, gt, np.repeat(np.arange(n), 2), **kw)


# ------------------------------------------------------------------------------------------------------------ generators
@functools.lru_cache(maxsize=None)
def box_box(seed=31):
    """3 072 pairs: regimes 1 (generic pairs near contact, 2 048) and 2 (relative rotation 1e-9 .. 1e-2 rad: near-parallel edges,
    1 024) of test_collider_geometry._boxbox_cases -- that function itself, asked for 4 096 and cut before its regime 3"""
    rng = np.random.default_rng(seed)
    p1, R1, s1, p2, R2, s2 = _boxbox_cases(rng, 4096)
    n = 3072
    return _interleave("box_box", (p1[:n], R1[:n], s1[:n], BOX), (p2[:n], R2[:n], s2[:n], BOX), np.zeros(n, bool))


@functools.lru_cache(maxsize=None)
def sphere_box(seed=32):
    """1 024 pairs with the centre distance U(0.15, 1.0) x the pair's reach; then 64 with the sphere's centre inside the box and 64
    on dCollideSphereBox's degenerate branches (centres coincide; the centre exactly on a face plane, inside its rectangle)"""
    rng = np.random.default_rng(seed)
    n0, n = 1024, 1024 + 128
    side = rng.uniform(0.2, 1.0, (n, 3))
    Rb = _rand_rot(rng, n)
    r = rng.uniform(0.1, 0.4, n)
    pb = rng.uniform(-1, 1, (n, 3))
    reach = r + 0.5 * np.linalg.norm(side, axis=1)
    ps = pb + _unit(rng, n) * (rng.uniform(0.15, 1.0, n) * reach)[:, None]
    a, b = n0, n0 + 64
    loc = rng.uniform(-0.49, 0.49, (64, 3)) * side[a:b]                       # inside the box
    ps[a:b] = pb[a:b] + np.einsum("nij,nj->ni", Rb[a:b], loc)
    Rb[b::2] = np.eye(3)                                                      # every other one: the pose's arithmetic is exact
    pb[b:] = np.round(pb[b:] * 8) / 8                                         # exact in float32 too, also after the far translation
    side[b:] = np.round(side[b:] * 16 + 4) / 16
    loc = rng.uniform(-0.45, 0.45, (64, 3)) * side[b:]
    axis = rng.integers(0, 3, 64)
    loc[np.arange(64), axis] = 0.5 * side[b:][np.arange(64), axis] * rng.choice([-1.0, 1.0], 64)     # on a face plane
    loc[:16] = 0.0                                                            # coincident centres
    ps[b:] = pb[b:] + np.einsum("nij,nj->ni", Rb[b:], loc)
    rad = np.column_stack([r, np.zeros(n), np.zeros(n)])
    I = np.tile(np.eye(3), (n, 1, 1))
    return _interleave("sphere_box", (ps, I, rad, SPHERE), (pb, Rb, side, BOX), np.arange(n) % 2 == 1)


@functools.lru_cache(maxsize=None)
def sphere_sphere(seed=33):
    """1 024 pairs with the centre distance U(0.15, 1.0) x (r1 + r2); then 64 with one centre inside the other sphere and 64 with
    coincident centres (dCollideSpheres' d <= 0 branch)"""
    rng = np.random.default_rng(seed)
    n0, n = 1024, 1024 + 128
    r1 = rng.uniform(0.1, 0.4, n); r2 = rng.uniform(0.1, 0.4, n)
    p1 = rng.uniform(-1, 1, (n, 3))
    f = rng.uniform(0.15, 1.0, n)
    f[n0:n0 + 64] = rng.uniform(0.01, 0.5, 64) * (np.minimum(r1, r2) / (r1 + r2))[n0:n0 + 64]
    f[n0 + 64:] = 0.0
    p2 = p1 + _unit(rng, n) * (f * (r1 + r2))[:, None]
    z = np.zeros(n)
    I = np.tile(np.eye(3), (n, 1, 1))
    return _interleave("sphere_sphere", (p1, I, np.column_stack([r1, z, z]), SPHERE), (p2, I, np.column_stack([r2, z, z]), SPHERE),
                       np.zeros(n, bool))


# centre distance as a share of the pair's reach, per hull population and shape: U(0.3, 1.0) unless the shape needs it tighter to
# meet the coverage conditions of tests/test_pair_population.py.  Every deviation: the tetrahedron in all three populations (its four
# vertices are seldom inside anything, and with its centre near the other geom's they are outside it again: hull-hull U(0.2, 0.6),
# box-hull U(0.1, 0.7), sphere-hull U(0.1, 0.8)) and the cube's hull-hull (U(0.25, 0.9): U(0.3, 1.0) left 90 near misses of the 100)
_HULL_RANGE = {("hull_hull", "tetra"): (0.2, 0.6), ("hull_hull", "cube"): (0.25, 0.9), ("box_hull", "tetra"): (0.1, 0.7),
               ("sphere_hull", "tetra"): (0.1, 0.8)}


def _hull_sizes(h, n):
    s = np.zeros((n, 3))
    s[:, 0] = h.radius
    return s


@functools.lru_cache(maxsize=None)
def hull_hull(shape, seed=34):
    h = hull_shape(shape)
    rng = np.random.default_rng(seed + HULL_SHAPES.index(shape))
    n = 1024
    lo, hi = _HULL_RANGE.get(("hull_hull", shape), (0.3, 1.0))
    pa = rng.uniform(-1, 1, (n, 3))
    pb = pa + _unit(rng, n) * (rng.uniform(lo, hi, n) * 2 * h.radius)[:, None]
    return _interleave(f"hull_hull[{shape}]", (pa, _rand_rot(rng, n), _hull_sizes(h, n), CONVEX),
                       (pb, _rand_rot(rng, n), _hull_sizes(h, n), CONVEX), np.zeros(n, bool), hull=h)


@functools.lru_cache(maxsize=None)
def sphere_hull(shape, seed=44):
    h = hull_shape(shape)
    rng = np.random.default_rng(seed + HULL_SHAPES.index(shape))
    n = 1024
    lo, hi = _HULL_RANGE.get(("sphere_hull", shape), (0.3, 1.0))
    r = rng.uniform(0.1, 0.4, n)
    ph = rng.uniform(-1, 1, (n, 3))
    ps = ph + _unit(rng, n) * (rng.uniform(lo, hi, n) * (r + h.radius))[:, None]
    z = np.zeros(n)
    return _interleave(f"sphere_hull[{shape}]", (ps, np.tile(np.eye(3), (n, 1, 1)), np.column_stack([r, z, z]), SPHERE),
                       (ph, _rand_rot(rng, n), _hull_sizes(h, n), CONVEX), np.arange(n) % 2 == 1, hull=h)


@functools.lru_cache(maxsize=None)
def box_hull(shape, seed=54):
    h = hull_shape(shape)
    rng = np.random.default_rng(seed + HULL_SHAPES.index(shape))
    n = 1024
    lo, hi = _HULL_RANGE.get(("box_hull", shape), (0.3, 1.0))
    side = rng.uniform(0.3, 1.2, (n, 3))
    ph = rng.uniform(-1, 1, (n, 3))
    pb = ph + _unit(rng, n) * (rng.uniform(lo, hi, n) * (0.5 * np.linalg.norm(side, axis=1) + h.radius))[:, None]
    return _interleave(f"box_hull[{shape}]", (pb, _rand_rot(rng, n), side, BOX), (ph, _rand_rot(rng, n), _hull_sizes(h, n), CONVEX),
                       np.arange(n) % 2 == 1, hull=h)


# ---- single bodies at static geometry ---------------------------------------------------------------------------------------
def _support(cls, R, size, hull, d):
    """how far the body reaches from its centre along the unit direction d"""
    if cls == SPHERE:
        return float(size[0])
    if cls == BOX:
        return float(0.5 * np.abs(R.T @ d) @ size)
    return float(np.max(hull.points @ (R.T @ d)))


def _frame_on(normal):
    """a rotation whose y axis is `normal`"""
    y = normal / np.linalg.norm(normal)
    x = np.cross(y, np.eye(3)[int(np.argmin(np.abs(y)))]); x /= np.linalg.norm(x)
    return np.column_stack([x, y, np.cross(x, y)])


def _yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _roll(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _body_draw(rng, k, hull, flat_frame, cls=None, flat=None):
    """class (cycling with k unless given), size and orientation of a single body: every third one flat on `flat_frame` to 1e-7 rad"""
    cls = (BOX, SPHERE, CONVEX)[k % 3] if cls is None else cls
    if cls == BOX:
        size = rng.uniform(0.2, 1.0, 3)
    elif cls == SPHERE:
        size = np.array([rng.uniform(0.1, 0.4), 0.0, 0.0])
    else:
        size = np.array([hull.radius, 0.0, 0.0])
    if ((k // 3) % 3 == 0) if flat is None else flat:
        R = flat_frame @ _small_rot(rng, 1, 10.0 ** rng.uniform(-9, -7))[0] @ _yaw(rng.uniform(0, 2 * np.pi))
        if cls == CONVEX:                        # a face of the hull down: that face's outward normal along -y of the frame
            f = hull.planes[rng.integers(0, len(hull.planes)), :3]
            R = R @ _frame_on(-f).T
    else:
        R = _rand_rot(rng, 1)[0]
    return cls, size, R


@functools.lru_cache(maxsize=None)
def on_plane(shape="ell65", seed=64):
    """1 024 single bodies -- boxes, spheres, hulls in turn -- whose lowest point is within +-0.05 of the tilted plane PLANE (drawn
    from U(-0.05, 0.02): 0.05 into it to 0.02 above, so most touch); one third lie flat on it to 1e-7 rad"""
    h = hull_shape(shape)
    rng = np.random.default_rng(seed)
    n = 1024
    nrm = np.array(PLANE[:3]); ln = np.linalg.norm(nrm)
    up, d = nrm / ln, PLANE[3] / ln
    F = _frame_on(up)
    org = _cell_origin(np.arange(n), per_row=32)
    pos = np.empty((n, 3)); Rs = np.empty((n, 3, 3)); sides = np.zeros((n, 3)); gt = np.empty(n, np.uint8)
    for k in range(n):
        cls, size, R = _body_draw(rng, k, h, F)
        x, z = org[k, 0], org[k, 2]
        foot = np.array([x, (d * ln - PLANE[0] * x - PLANE[2] * z) / PLANE[1], z])              # on the plane
        pos[k] = foot + up * (_support(cls, R, size, h, -up) + rng.uniform(-0.05, 0.02))
        Rs[k] = R; sides[k] = size; gt[k] = cls
    return Population("on_plane", pos, _quat_from_R(Rs), sides, gt, np.arange(n), plane=PLANE, hull=h)


def _R12(R):
    return [float(v) for v in np.column_stack([R, np.zeros(3)]).ravel()]


@functools.lru_cache(maxsize=None)
def on_statics(shape="ell65", seed=74):
    """512 single bodies at 64 static boxes (DMX_MAX_STATIC_BOXES): the reference's 100 x 1 x 100 floor (top at y = 0.5) and, one in
    each 10 m cell of an 8 x 8 lattice on it but the first, 63 more in turn:
      planks  5-6 m long lying on the floor, turned about y and (up to 0.2 rad) about z -- bodies on their upper face;
      walls   5-6 m long, 1-3 m high, standing in the floor, turned about y (and 0.05 rad about z) -- bodies in the corner of floor and wall;
      strips  5-6 m long, 0.3-0.5 m wide, their upper face flush with the floor's to a millimetre -- bodies across them, on both.
    Eight bodies a cell: three at the cell's static box (2.1 m apart along it), five on the floor alone, out to +-39.6 m (regime 3 of
    _boxbox_cases: a small box on a floor-sized one).  Penetrations U(-0.02, 0.05): hovering within 0.02 above to 0.05 deep."""
    h = hull_shape(shape)
    rng = np.random.default_rng(seed)
    up = np.array([0.0, 1.0, 0.0])
    top = 0.5
    statics = [((100.0, 1.0, 100.0), (0.0, 0.0, 0.0), _R12(np.eye(3)))]
    pos, Rs, sides, gt = [], [], [], []

    def put(cls, size, R, c):
        pos.append(c); Rs.append(R); sides.append(size); gt.append(cls)

    k = 0
    for c in range(64):
        o = np.array([(c % 8 - 3.5) * 10.0, 0.0, (c // 8 - 3.5) * 10.0])
        kind = None if c == 0 else ("plank", "wall", "strip")[c % 3]
        yaw = rng.uniform(0, np.pi)
        L = rng.uniform(5.0, 6.0)
        if kind == "plank":
            sz = np.array([L, rng.uniform(0.3, 0.6), rng.uniform(0.5, 1.0)])
            Rst = _yaw(yaw) @ _roll(rng.uniform(-0.2, 0.2))
            cst = o + up * (top + 0.5 * sz[1] + 0.5 * L * abs(Rst[1, 0]) - 0.05)
        elif kind == "wall":
            sz = np.array([L, rng.uniform(1.0, 3.0), rng.uniform(0.3, 0.6)])
            Rst = _yaw(yaw) @ _roll(rng.uniform(-0.05, 0.05))
            cst = o + up * (top + 0.5 * sz[1] - 0.2)
        elif kind == "strip":
            sz = np.array([L, 1.0, rng.uniform(0.3, 0.5)])
            Rst = _yaw(yaw)
            cst = o + up * rng.uniform(-1e-3, 1e-3)
        if kind is not None:
            statics.append((tuple(float(v) for v in sz), tuple(float(v) for v in cst), _R12(Rst)))
        for j in range(8):
            pen = rng.uniform(-0.02, 0.05)
            if j >= 3 or kind is None:                                        # on the floor alone
                off = [(-3.8, -3.8), (3.8, -3.8), (-3.8, 3.8), (3.8, 3.8), (0.0, 4.6), (-2.1, 0.0), (0.0, 0.0), (2.1, 0.0)][(j + 5) % 8]
                cls, size, R = _body_draw(rng, k, h, np.eye(3))
                ctr = o + np.array([off[0], 0.0, off[1]])
                ctr[1] = top + _support(cls, R, size, h, -up) - pen
            else:
                along = (j - 1) * 2.1
                if kind == "plank":
                    nrm = Rst[:, 1]
                    cls, size, R = _body_draw(rng, k, h, Rst)
                    face = cst + Rst @ np.array([along, 0.5 * sz[1], rng.uniform(-0.1, 0.1)])
                    ctr = face + nrm * (_support(cls, R, size, h, -nrm) - pen)
                elif kind == "wall":
                    sg = rng.choice([-1.0, 1.0])
                    nrm = sg * Rst[:, 2]                                      # horizontal: a turn about z leaves the z axis alone
                    cls, size, R = _body_draw(rng, k, h, _yaw(yaw))
                    face = cst + Rst @ np.array([along, 0.0, sg * 0.5 * sz[2]])
                    ctr = face + nrm * (_support(cls, R, size, h, -nrm) - rng.uniform(-0.02, 0.05))
                    ctr[1] = top + _support(cls, R, size, h, -up) - pen
                else:                                                         # across the strip, flat boxes mostly: floor + strip
                    cls, size, R = _body_draw(rng, k, h, np.eye(3), cls=BOX, flat=k % 4 != 3)
                    if cls == BOX:
                        size = np.array([rng.uniform(0.6, 1.0), rng.uniform(0.2, 1.0), rng.uniform(0.6, 1.0)])
                    ctr = cst + Rst @ np.array([along, 0.0, rng.uniform(-0.1, 0.1)])
                    pen = abs(pen) + 2e-3
                    ctr[1] = top + _support(cls, R, size, h, -up) - pen
            put(cls, size, R, ctr)
            k += 1
    n = len(pos)
    return Population("on_statics", np.array(pos), _quat_from_R(np.array(Rs)), np.array(sides), np.array(gt, np.uint8), np.arange(n),
                      cell_pitch=2.1, static_boxes=statics, hull=h)


def get(name, shape=None):
    """a population by name; the hull populations (and the hull of on_plane / on_statics) take a shape of HULL_SHAPES"""
    g = globals()[name]
    return g(shape) if shape is not None else g()


ALL = ([("box_box", None), ("sphere_box", None), ("sphere_sphere", None)] +
       [(p, s) for p in ("hull_hull", "sphere_hull", "box_hull") for s in HULL_SHAPES] + [("on_plane", None), ("on_statics", None)])


def pop_id(key):
    return key[0] if key[1] is None else f"{key[0]}-{key[1]}"


# ------------------------------------------------------------------------------------------------------------ the oracle side
def oracle_world(pop, dtype, shift=None, max_contacts=8):
    """the population in the oracle: plane, hull, static boxes, then the bodies ONE BY ONE in slot order (the bulk adders would impose
    an order by class); mass 1 and identity inertia are dBodyCreate's own.  -> (Oracle, World, scene)"""
    return oracle_world_of(pop.scene(dtype, shift), dtype, max_contacts)


def oracle_world_of(sc, dtype, max_contacts=8, cfm=None):
    """`oracle_world` for a scene already made (its values are cast to `dtype`); cfm None: the precision's default"""
    sc = sc.astype(dtype)
    orc = Oracle(dtype)
    lib = orc.lib
    ow = orc.world()
    lib.orc_world_set_max_contacts(ow.w, int(max_contacts))
    if cfm is not None:
        lib.orc_world_set_cfm(ow.w, cfm)
    if sc.plane is not None:
        ow.add_plane(*sc.plane)
    if sc.hull_points is not None:
        ow.set_hull(sc.hull_points)
        ow.set_hull_faces(sc.hull_planes)
    for sz, at, R12 in (sc.static_boxes or []):
        ow.add_static_box(sz, at, R12)
    P = sc.pos.tolist(); S = sc.sides.tolist(); G = sc.gtype.tolist()
    quat = np.ascontiguousarray(sc.quat)
    Q = (orc.real * 4 * sc.n).from_buffer(quat)
    for i in range(sc.n):
        b = lib.orc_body_create(ow.w)
        lib.orc_body_set_position(ow.w, b, *P[i])
        lib.orc_body_set_quaternion(ow.w, b, Q[i])
        g = (lib.orc_geom_create_sphere(ow.w, S[i][0]) if G[i] == SPHERE else lib.orc_geom_create_convex(ow.w) if G[i] == CONVEX
             else lib.orc_geom_create_box(ow.w, *S[i]))
        lib.orc_geom_set_category_bits(ow.w, g, 2); lib.orc_geom_set_collide_bits(ow.w, g, 3)
        lib.orc_geom_set_body(ow.w, g, b)
    return orc, ow, sc


def joints_by_cell(pop, ow):
    """the last tick's contact joints by cell: (body-body contacts per cell, contacts with static geometry per cell, the joints whose
    two bodies are of different cells, the joints themselves)"""
    nc = int(pop.cell.max()) + 1
    bb = np.zeros(nc, int); st = np.zeros(nc, int)
    crossing = []
    js = ow.joints()
    for j in js:
        b1, b2 = j[0], j[1]
        if b2 >= 0:
            if pop.cell[b1] != pop.cell[b2]:
                crossing.append((b1, b2))
            bb[pop.cell[b1]] += 1
        else:
            st[pop.cell[b1]] += 1
    return bb, st, crossing, js


def bulk_counts(orc, hull, cls1, pose1, size1, cls2, pose2, size2, maxc=8, plane=None):
    """orc_collide_bulk's contact counts for n pairs of body-less geoms of two classes at the given poses (pos3 + R12), in the
    oracle's own precision; cls2 None: against `plane`"""
    w = orc.world()
    if hull is not None:
        w.set_hull(hull.points)
        w.set_hull_faces(hull.planes)

    def geom(cls):
        if cls is None:
            return orc.lib.orc_geom_create_plane(w.w, *plane)
        return (orc.lib.orc_geom_create_sphere(w.w, 0.3) if cls == SPHERE else orc.lib.orc_geom_create_convex(w.w) if cls == CONVEX
                else orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0))
    g1, g2 = geom(cls1), geom(cls2)
    n = len(pose1)
    counts = np.zeros(n, np.int32)
    out = (orc.ContactGeom * (n * maxc))()
    keep = [None if a is None else np.ascontiguousarray(a, orc.dtype) for a in (pose1, size1, pose2, size2)]
    orc.lib.orc_collide_bulk(w.w, g1, g2, n, *[None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep], maxc,
                             counts.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p))
    w.close()
    return counts


def world_poses(orc, ow, n):
    """(n, 15) poses (pos3 + R12) of the oracle's bodies, bit for bit as its colliders read them"""
    out = np.empty((n, 15), orc.dtype)
    for b in range(n):
        out[b, :3] = np.ctypeslib.as_array(orc.lib.orc_body_get_position(ow.w, b), (3,))
        out[b, 3:] = np.ctypeslib.as_array(orc.lib.orc_body_get_rotation(ow.w, b), (12,))
    return out


def aabbs(pose, sides, gtype, hull):
    """world AABBs by the oracle's formulas (float64 arithmetic on its values): (lo, hi), each (n, 3)"""
    pose = np.asarray(pose, float)
    p = pose[:, :3]
    R = pose[:, 3:].reshape(-1, 3, 4)[:, :, :3]
    n = len(p)
    r = np.zeros((n, 3))
    sp = gtype == SPHERE; bx = gtype == BOX; cv = gtype == CONVEX
    r[sp] = np.asarray(sides, float)[sp, :1]
    r[bx] = 0.5 * np.einsum("nij,nj->ni", np.abs(R[bx]), np.asarray(sides, float)[bx])
    lo, hi = p - r, p + r
    if cv.any():
        v = np.einsum("nij,kj->nki", R[cv], hull.points) + p[cv][:, None, :]
        lo[cv] = v.min(axis=1); hi[cv] = v.max(axis=1)
    return lo, hi


def static_aabbs(scene):
    """(lo, hi) of the scene's static boxes by the oracle's formula"""
    sz = np.array([s[0] for s in scene.static_boxes], float)
    at = np.array([s[1] for s in scene.static_boxes], float)
    R = np.array([s[2] for s in scene.static_boxes], float).reshape(-1, 3, 4)[:, :, :3]
    r = 0.5 * np.einsum("nij,nj->ni", np.abs(R), sz)
    return at - r, at + r


def analyse(pop, dtype, shift=None, max_contacts=8):
    """One oracle tick of the population and what it shows -- a dict of counts -- after the checks every population must pass: the
    state stays finite, no joint crosses cells, and per cell the world's contact count equals orc_collide_bulk's on the same poses
    wherever the AABBs overlap (and is zero wherever they are apart); cells whose AABBs are within `tol` of touching may go either
    way in the AABB test and are left out of that one comparison (counted in "aabb_marginal")."""
    orc, ow, sc = oracle_world(pop, dtype, shift, max_contacts)
    n = sc.n
    pose = world_poses(orc, ow, n)
    ow.tick(orc.dtype.type(H))
    for name, a in zip(("pos", "quat", "lvel", "avel"), ow.state()):
        assert np.all(np.isfinite(a)), f"{pop.name} {dtype}: {name} not finite after the tick"
    bb, st, crossing, js = joints_by_cell(pop, ow)
    assert not crossing, f"{pop.name}: joints across cells {crossing[:5]}"
    assert len(js) == ow.n_contacts()
    tol = 1e-4 if np.dtype(dtype).itemsize == 4 and shift is not None else (1e-6 if np.dtype(dtype).itemsize == 4 else 1e-12)
    lo, hi = aabbs(pose, sc.sides, sc.gtype, pop.hull)
    gt = sc.gtype
    out = {"bodies": n, "cells": int(pop.cell.max()) + 1, "contacts": int(ow.n_contacts())}
    if pop.paired:
        a, b = np.arange(0, n, 2), np.arange(1, n, 2)
        gap = np.max(np.maximum(lo[a] - hi[b], lo[b] - hi[a]), axis=1)            # > 0: the AABBs are apart
        bulk = np.zeros(len(a), int)
        for c1, c2 in sorted({(int(x), int(y)) for x, y in zip(gt[a], gt[b])}):
            m = (gt[a] == c1) & (gt[b] == c2)
            bulk[m] = bulk_counts(orc, pop.hull, c1, pose[a[m]], sc.sides[a[m]], c2, pose[b[m]], sc.sides[b[m]], max_contacts)
        over, apart = gap < -tol, gap > tol
        assert np.array_equal(bb[over], bulk[over]), f"{pop.name}: world and bulk collider disagree in cells {np.flatnonzero(over & (bb != bulk))[:8]}"
        assert not bb[apart].any(), f"{pop.name}: contacts although the AABBs are apart, cells {np.flatnonzero(apart & (bb > 0))[:8]}"
        assert not st.any()
        assert (~over & ~apart).sum() <= 0.01 * len(a), f"{pop.name}: {int((~over & ~apart).sum())} cells within {tol} of touching AABBs"
        out.update(pairs=len(a), colliding=int((bb > 0).sum()), near_miss=int((over & (bb == 0)).sum()), at_cap=int((bb >= max_contacts).sum()),
                   aabb_marginal=int((~over & ~apart).sum()), bulk=bulk, per_cell=bb, joints=js)
        return out
    # single bodies: against the plane, against each static box
    assert not bb.any(), f"{pop.name}: a contact joins two bodies"
    want = np.zeros(n, int)
    touched = np.zeros(n, int)
    marginal = 0
    classes = sorted({int(x) for x in gt})
    if sc.plane is not None:
        for c1 in classes:
            m = gt == c1
            want[m] += bulk_counts(orc, pop.hull, c1, pose[m], sc.sides[m], None, np.zeros((int(m.sum()), 15)), None, max_contacts, plane=sc.plane)
    ok = np.ones(n, bool)
    if sc.static_boxes:
        slo, shi = static_aabbs(sc)
        for s, (sz, at, R12) in enumerate(sc.static_boxes):
            gap = np.max(np.maximum(lo - shi[s], slo[s] - hi), axis=1)
            over = gap < -tol
            ok &= over | (gap > tol)
            marginal += int((~over & ~(gap > tol)).sum())
            sp = np.concatenate([np.asarray(at, float), np.asarray(R12, float)])
            for c1 in classes:
                m = (gt == c1) & over
                if not m.any():
                    continue
                k = int(m.sum())
                got = bulk_counts(orc, pop.hull, BOX, np.tile(sp, (k, 1)), np.tile(np.asarray(sz, float), (k, 1)), c1, pose[m], sc.sides[m], max_contacts)
                want[m] += got
                touched[m] += got > 0
    assert (~ok).sum() <= 0.01 * n, f"{pop.name}: {int((~ok).sum())} bodies within {tol} of touching a static box's AABB"
    assert np.array_equal(st[ok], want[ok]), f"{pop.name}: world and bulk collider disagree for bodies {np.flatnonzero(ok & (st != want))[:8]}"
    out.update(colliding=int((st > 0).sum()), two_statics=int((touched >= 2).sum()), over_8=int((st > 8).sum()), aabb_marginal=marginal,
               per_cell=st, joints=js)
    return out


# ------------------------------------------------------------------------------------------------------------ float32 against float64
# One tick of a population in float32 against the same tick in float64 ON THE SAME float32 VALUES, both at cfm 1e-5 (the precisions'
# defaults, 1e-5 / 1e-10, alone move the states at the 1e-3 level).  tests/test_pair_population.py measures and asserts this through the
# two oracles; tests/test_gpu_precision_pairs.py holds the device to the same numbers.  DESIGN.md section 5, "float32 against float64
# geometry", carries the tables.
EPS32 = float(np.finfo(np.float32).eps)
CFM_BOTH = 1e-5
MAX_NOT_COMPARABLE = 0.08            # share of a population's cells whose contacts may differ in count, slot or by more than the band

# k of the band k eps32 M, per collider: the largest deviation of the float32 oracle from the float64 numpy references of
# tests/test_collider_geometry.py over >= 10^5 draws, near and far, x 2, rounded up to a power of two (the measured maxima are in
# that file's F32_MEASURED and in DESIGN.md).  K_CONTACT, the band of a contact joint in the tick comparison, is their maximum.
K_BAND = {"box_box": 4, "box_on_face": 2, "sphere_box": 2, "sphere_sphere": 2, "sphere_plane": 4, "box_plane": 8, "hulls": 2}
K_CONTACT = max(K_BAND.values())

# measured through the two oracles (tests/test_pair_population.py::test_one_tick_in_float32_against_float64 prints them): the largest |float32 - float64| over the
# comparable cells' bodies per population class and place, velocities in eps32 M_world / h, poses in eps32 M_world.
# (lvel, avel, pos, quat); the tolerance is 4 x these (the maxima sit 3-10 x over the p99: a long tail).
TICK_MEASURED = {
    "box_box": {"near": (0.01, 0.037, 0.25, 0.017), "far": (0.017, 0.046, 0.45, 0.024)},
    "sphere_box": {"near": (0.08, 0.027, 0.25, 0.011), "far": (0.26, 0.16, 0.44, 0.068)},
    "sphere_sphere": {"near": (0.0014, 0.012, 0.25, 0.0061), "far": (0.0024, 0.023, 0.44, 0.011)},
    "hull_hull": {"near": (0.061, 0.17, 0.27, 0.077), "far": (0.5, 0.45, 0.59, 0.2)},
    "sphere_hull": {"near": (0.0033, 0.0099, 0.25, 0.0049), "far": (0.0063, 0.022, 0.45, 0.01)},
    "box_hull": {"near": (0.054, 0.2, 0.27, 0.089), "far": (0.29, 0.41, 0.48, 0.19)},
    "on_plane": {"near": (0.022, 0.051, 0.26, 0.029), "far": (0.034, 0.072, 0.42, 0.034)},
    "on_statics": {"near": (0.11, 0.089, 0.31, 0.05), "far": (0.1, 0.16, 0.56, 0.063)},
}
TICK_FACTOR = 4.0


def tick_tolerance(name, far):
    """(lvel, avel, pos, quat) tolerances in the units of `precision_tick`, for a population class and place"""
    return tuple(TICK_FACTOR * v for v in TICK_MEASURED[name]["far" if far else "near"])


def scene_in_float32_values(pop, shift=None):
    """the population's float32 scene and the same VALUES as a float64 scene: the plane and the static boxes, which `astype` leaves as
    Python floats, rounded to float32 too"""
    sc = pop.scene("float32", shift)
    r = lambda v: float(np.float32(v))
    plane = None if sc.plane is None else tuple(r(v) for v in sc.plane)
    statics = None if not sc.static_boxes else [(tuple(r(v) for v in sz), tuple(r(v) for v in at), [r(v) for v in R12])
                                                for sz, at, R12 in sc.static_boxes]
    sc32 = pkg.scenes.Scene(sc.pos, sc.quat, sc.lvel, sc.avel, sc.mass, sc.inertia, sc.sides, sc.gtype, plane, sc.hull_points,
                            sc.hull_planes, statics)
    return sc32, sc32.astype("float64")


def _extents(pop, sc):
    """per body: the bounding radius and the smallest extent (sphere: r; box: half the diagonal / the least side; hull: its radius /
    twice the nearest face's distance from the centre)"""
    s = np.asarray(sc.sides, float)
    big = np.where(sc.gtype == SPHERE, s[:, 0], 0.5 * np.linalg.norm(s, axis=1))
    small = np.where(sc.gtype == SPHERE, s[:, 0], s.min(axis=1))
    if pop.hull is not None:
        cv = sc.gtype == CONVEX
        big[cv] = pop.hull.radius
        small[cv] = 2.0 * float(np.min(pop.hull.planes[:, 3]))
    return big, small


def _static_reach(sc):
    """the static geometry's own numbers: (|plane offset|, normalised; the largest |coordinate| of the static boxes' AABBs)"""
    off = 0.0 if sc.plane is None else abs(sc.plane[3]) / float(np.linalg.norm(sc.plane[:3]))
    far = 0.0
    if sc.static_boxes:
        lo, hi = static_aabbs(sc)
        far = float(max(np.abs(lo).max(), np.abs(hi).max()))
    return off, far


@functools.lru_cache(maxsize=None)
def precision_tick(key, far, k_contact=K_CONTACT):
    """One tick of population `key` through the float32 and the float64 oracle on the same float32 values, cfm 1e-5 in both.
    COMPARABLE cells, decided from the two oracles' joints alone: the same contact count, every contact in the same slot between the
    same bodies, pos and depth within band = k eps32 M_cell and the normal within band / (the cell's smallest extent) radians;
    M_cell = the largest |coordinate| of the cell's bodies and of the static boxes + the bodies' bounding radii + |plane offset|.  -> a dict; the states
    are read-only."""
    pop = get(*key)
    sc32, sc64 = scene_in_float32_values(pop, FAR if far else None)
    nc = int(pop.cell.max()) + 1
    side = {}
    for dtype, sc in (("float32", sc32), ("float64", sc64)):
        orc, ow, _ = oracle_world_of(sc, dtype, cfm=CFM_BOTH)
        ow.tick(orc.dtype.type(H))
        st = ow.state()
        for a in st:
            a.setflags(write=False)
        per = [[] for _ in range(nc)]
        for j in ow.joints():
            per[pop.cell[j[0]]].append(j)
        side[dtype] = (st, per, ow.n_contacts())
        ow.close()
    big, small = _extents(pop, sc64)
    plane_off, static_far = _static_reach(sc64)
    m_body = np.abs(sc64.pos).max(axis=1)
    m_cell = np.zeros(nc); ext = np.full(nc, np.inf)
    r_cell = np.zeros(nc)
    np.maximum.at(m_cell, pop.cell, m_body)
    np.add.at(r_cell, pop.cell, big)
    np.minimum.at(ext, pop.cell, small)
    m_cell = np.maximum(m_cell, static_far) + r_cell + plane_off
    band = k_contact * EPS32 * m_cell
    comparable = np.ones(nc, bool)
    by_count = 0
    worst = np.zeros(3)                                   # pos, depth (in eps32 M_cell), normal (in eps32 M_cell / extent) over same-slot contacts
    for c in range(nc):
        a, b = side["float32"][1][c], side["float64"][1][c]
        if len(a) != len(b):
            comparable[c] = False; by_count += 1
            continue
        for ja, jb in zip(a, b):
            if ja[0] != jb[0] or ja[1] != jb[1]:
                comparable[c] = False
                break
            dp = float(np.max(np.abs(np.subtract(ja[2], jb[2])))); dd = abs(ja[4] - jb[4])
            dn = float(np.linalg.norm(np.subtract(ja[3], jb[3])))
            if dp > band[c] or dd > band[c] or dn > band[c] / ext[c]:
                comparable[c] = False
                break
            u = EPS32 * m_cell[c]
            worst = np.maximum(worst, [dp / u, dd / u, dn * ext[c] / u])
    m_world = float(max(m_body.max(), static_far) + big.max() + plane_off)
    body_ok = comparable[pop.cell]
    units = (EPS32 * m_world / H, EPS32 * m_world / H, EPS32 * m_world, EPS32 * m_world)          # lvel, avel, pos, quat
    s32, s64 = side["float32"][0], side["float64"][0]
    order = (2, 3, 0, 1)                                   # state() is (pos, quat, lvel, avel)
    dev = tuple(float(np.max(np.abs(s32[i][body_ok].astype(float) - s64[i][body_ok]))) / u for i, u in zip(order, units))
    n32 = np.array([len(x) for x in side["float32"][1]]); n64 = np.array([len(x) for x in side["float64"][1]])
    return dict(pop=pop, sc32=sc32, sc64=sc64, state32=s32, state64=s64, comparable=comparable, body_ok=body_ok, m_world=m_world,
                units=units, dev=dev, not_comparable=int((~comparable).sum()), by_count=by_count, cells=nc, contacts32=n32, contacts64=n64,
                total32=side["float32"][2], total64=side["float64"][2], contact_dev=tuple(float(v) for v in worst))


def deviation(state_a, state_b, body_ok, units):
    """(lvel, avel, pos, quat) largest |a - b| over the bodies of `body_ok`, in `units`; states are (pos, quat, lvel, avel)"""
    return tuple(float(np.max(np.abs(np.asarray(state_a[i], float)[body_ok] - np.asarray(state_b[i], float)[body_ok]))) / u
                 for i, u in zip((2, 3, 0, 1), units))
