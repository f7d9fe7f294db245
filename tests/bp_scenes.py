"""Scenes for the broadphase tests (tests/test_broadphase_reference.py on the CPU, tests/test_gpu_broadphase.py on the
device): plain arrays, float64, rounded to the batch's precision by whoever uploads them.  Every scene that rounding can
touch is drawn from a seed; test_broadphase_reference.py checks with the reference alone that each leaves at most its
allowed share of pairs inside the band (2 %; 0.1 % near the origin)."""
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from bp_reference import GEOM_BOX, GEOM_CONVEX, GEOM_NONE, GEOM_SPHERE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@dataclass
class Case:
    name: str
    pos: np.ndarray
    quat: np.ndarray
    sides: np.ndarray
    gtype: np.ndarray
    hull: Optional[np.ndarray] = None
    statics: list = field(default_factory=list)
    n_active: Optional[int] = None
    near_origin: bool = True           # band share limit: 0.1 % near the origin, 2 % elsewhere
    exact: bool = False                # every number exactly representable and every comparison exact: no band at all

    @property
    def n(self):
        return len(self.pos)

    def moved(self, offset, name=None):
        off = np.asarray(offset, np.float64)
        st = [(s, tuple(np.asarray(p, np.float64) + off), R) for s, p, R in self.statics]
        return Case(name or f"{self.name}@{tuple(offset)}", self.pos + off, self.quat, self.sides, self.gtype, self.hull, st,
                    self.n_active, bool(np.abs(off).max() < 100.0) and self.near_origin, self.exact)


IDENT_R12 = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)


def rot_y_z(ay, az):
    cy, sy, cz, sz = np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    R = Ry @ Rz
    return tuple(np.concatenate([R, np.zeros((3, 1))], 1).ravel())


def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _ident_quats(n):
    q = np.zeros((n, 4)); q[:, 0] = 1.0
    return q


def cube_hull(side=0.8):
    return 0.5 * side * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def teapot_hull():
    """the stored teapot hull's points about their centroid, scaled to about a metre across"""
    p = np.load(os.path.join(ROOT, "tests", "golden", "teapot_hull.npz"))["points"].astype(np.float64) * 0.01
    return p - p.mean(0)


def hull_radius(h):
    return float(np.sqrt((h * h).sum(1).max()))


def tumbling_boxes(n, seed, extent=None, height=3.0):
    """n boxes with sides in [0.2, 1], random attitudes, in a slab extent x height x extent: about 3-10 AABB pairs per body"""
    rng = np.random.default_rng(seed)
    extent = extent if extent is not None else 0.62 * np.sqrt(n)
    pos = rng.uniform([-extent / 2, 0.0, -extent / 2], [extent / 2, height, extent / 2], size=(n, 3))
    sides = rng.uniform(0.2, 1.0, size=(n, 3))
    return Case(f"boxes{n}s{seed}", pos, _unit_quats(rng, n), sides, np.full(n, GEOM_BOX, np.uint8))


def mixed(n, seed, hull, none_share=0.0, extent=None, height=2.5, name="mixed"):
    """spheres, boxes and hulls in equal shares (and GEOM_NONE slots sprinkled in: their data is as live as anyone's)"""
    rng = np.random.default_rng(seed)
    extent = extent if extent is not None else 0.6 * np.sqrt(n)
    pos = rng.uniform([-extent / 2, 0.0, -extent / 2], [extent / 2, height, extent / 2], size=(n, 3))
    g = rng.integers(1, 4, size=n).astype(np.uint8)
    sides = rng.uniform(0.2, 1.0, size=(n, 3))
    sides[g == GEOM_SPHERE, 0] = rng.uniform(0.15, 0.55, size=int((g == GEOM_SPHERE).sum()))
    sides[g == GEOM_CONVEX, 0] = hull_radius(hull)
    if none_share > 0:
        g[rng.random(n) < none_share] = GEOM_NONE
    return Case(f"{name}{n}s{seed}", pos, _unit_quats(rng, n), sides, g, hull)


def lattice_boxes():
    """identity-quaternion boxes with sides in {0.5, 1, 2} at multiples of 0.25: faces touching (a pair), 2^-10 apart (no pair),
    nested, and touching along an edge and at a corner; every sum is exact in float32, so no band applies"""
    e = 2.0 ** -10
    rows = [
        ((0.0, 0.0, 0.0), 1.0), ((1.0, 0.0, 0.0), 1.0),            # 0-1 faces touching in x
        ((0.0, 1.0 + e, 0.0), 1.0),                                 # 2: 2^-10 above 0 and 1: no pair
        ((0.0, 0.0, 1.0), 1.0),                                     # 3: touches 0 in z, 1 along an edge
        ((1.0, 0.0, -1.0 - e), 1.0),                                # 4: 2^-10 short of 1 in z: no pair
        ((5.0, 0.0, 5.0), 2.0), ((5.0, 0.25, 5.25), 0.5),           # 5-6: nested
        ((6.25, 0.0, 5.0), 0.5),                                    # 7: face on 5's (6.0)
        ((6.25 + e, 1.0, 5.0), 0.5),                                # 8: 2^-10 clear of 5 in x, well above 7: no pair
        ((-3.0, 0.0, -3.0), 1.0), ((-4.0, -1.0, -4.0), 1.0),        # 9-10: corner to corner, negative coordinates
        ((-3.0, 0.0, -4.0 - e), 1.0),                               # 11: 2^-10 short of 9 in z; meets 10 at x = -3.5
        ((-0.0, 4.0, -0.0), 0.5), ((0.5, 4.0, 0.0), 0.5),           # 12-13 touching across x = 0.25
        ((-0.5 - e, 4.0, 0.0), 0.5),                                # 14: 2^-10 short of 12
    ]
    pos = np.array([r[0] for r in rows], np.float64)
    sides = np.array([[r[1]] * 3 for r in rows], np.float64)
    n = len(rows)
    return Case("lattice", pos, _ident_quats(n), sides, np.full(n, GEOM_BOX, np.uint8), exact=True)


def cell_boundary_spheres():
    """spheres of radius 0.4 (cell = exactly 1.0) with centres on integer cell boundaries, at x = -0.0, and straddling
    ix = -1 | 0, touching (centres 0.8 apart; 0.75 and 0.5 overlap) and 0.8125 apart (no pair)"""
    c = [(0.0, 0.0, 0.0), (0.75, 0.0, 0.0), (-0.75, 0.0, 0.0), (-0.0, 0.0, 0.75), (0.0, 0.0, -0.75),
         (3.0, 0.0, 3.0), (3.0, 0.0, 3.8125), (3.8125, 0.0, 3.0), (2.25, 0.0, 3.0), (3.0, 0.5, 2.5),
         (-1.0, 2.0, -1.0), (-0.25, 2.0, -1.0), (-1.0, 2.0, -0.25), (-1.75, 2.0, -1.75), (-1.5, 2.0, -1.5),
         (-0.25, 5.0, 7.0), (0.25, 5.0, 7.0), (-0.25, 5.0, 6.5), (0.5, 5.0, 8.0), (1.0625, 5.0, 7.0)]
    pos = np.array(c, np.float64)
    n = len(c)
    sides = np.zeros((n, 3)); sides[:, 0] = 0.4
    return Case("cellspheres", pos, _ident_quats(n), sides, np.full(n, GEOM_SPHERE, np.uint8))


def column(k, seed=3):
    """a vertical stack of k boxes in one (x,z) column (bucket capacity 8: 9 overflow the torus table, then the scrambled
    one, then the capacity doubles; 17 and 40 double it again), neighbours overlapping, and a few loose boxes around it"""
    rng = np.random.default_rng(seed + k)
    n = k + 12
    pos = np.zeros((n, 3)); sides = np.full((n, 3), 0.5)
    pos[:k, 1] = 0.45 * np.arange(k)
    pos[:k, 0] = 0.1 + 0.01 * rng.random(k); pos[:k, 2] = 0.1 + 0.01 * rng.random(k)
    pos[k:] = rng.uniform([-2.0, 0.0, -2.0], [2.0, 0.45 * k, 2.0], size=(12, 3))
    return Case(f"column{k}", pos, _unit_quats(rng, n), sides, np.full(n, GEOM_BOX, np.uint8))


def torus_clusters(n_clusters, axis, seed=5):
    """clusters of spheres (r = 0.4: cell 1.0) exactly one torus period apart -- 32 columns for n <= 512 -- along x or z: the
    clusters share their buckets, cell for cell"""
    rng = np.random.default_rng(seed)
    m = 24
    base = rng.uniform([0.0, 0.0, 0.0], [3.0, 1.0, 3.0], size=(m, 3))
    pos = np.concatenate([base + np.eye(3)[axis] * 32.0 * c for c in range(n_clusters)])
    n = len(pos)
    sides = np.zeros((n, 3)); sides[:, 0] = 0.4
    return Case(f"torus{n_clusters}{'xyz'[axis]}", pos, _ident_quats(n), sides, np.full(n, GEOM_SPHERE, np.uint8))


def one_over_many(k, big_last):
    """one large flat box over k small ones (its partners), first or last in the batch: with the lowest index it owns all k
    pairs (EXS_PARTNERS = 8 / EX_STAGE_PARTNERS = 32 staged, the rest by a second walk), with the highest none of them"""
    n = k + 1
    cols = int(np.ceil(np.sqrt(k)))
    small = np.array([[0.9 * (i % cols), 0.0, 0.9 * (i // cols)] for i in range(k)], np.float64)      # 0.9 apart: no small-small pair
    small[:, [0, 2]] -= 0.45 * (cols - 1)
    big = np.array([[0.0, 0.3, 0.0]])
    pos = np.concatenate([small, big] if big_last else [big, small])
    sides = np.full((n, 3), 0.25)
    sides[-1 if big_last else 0] = (0.9 * cols + 1.0, 0.5, 0.9 * cols + 1.0)
    return Case(f"over{k}{'last' if big_last else 'first'}", pos, _ident_quats(n), sides, np.full(n, GEOM_BOX, np.uint8))


def with_filler(case, n_total, seed=9):
    """the case's bodies first, then loose spheres on a far grid (no overlaps among them) up to n_total slots"""
    extra = n_total - case.n
    assert extra >= 0
    if extra == 0:
        return case
    side = int(np.ceil(np.sqrt(extra)))
    k = np.arange(extra)
    far = np.abs(case.pos).max() + 50.0
    pos = np.stack([far + 1.5 * (k % side), np.zeros(extra), far + 1.5 * (k // side)], 1)
    sides = np.zeros((extra, 3)); sides[:, 0] = 0.3
    return Case(f"{case.name}+{extra}", np.concatenate([case.pos, pos]), np.concatenate([case.quat, _ident_quats(extra)]),
                np.concatenate([case.sides, sides]), np.concatenate([case.gtype, np.full(extra, GEOM_SPHERE, np.uint8)]),
                case.hull, case.statics, case.n_active, case.near_origin, case.exact)


def with_ghosts(case, n_active):
    """slots [n_active, n) are ghosts (dmxBatchSetActiveCount); n_active a multiple of 4"""
    assert n_active % 4 == 0 and n_active <= case.n
    return Case(f"{case.name}/a{n_active}", case.pos, case.quat, case.sides, case.gtype, case.hull, case.statics, n_active,
                case.near_origin, case.exact)


def with_statics(case, statics, name):
    return Case(f"{case.name}+{name}", case.pos, case.quat, case.sides, case.gtype, case.hull, list(statics), case.n_active,
                case.near_origin, case.exact)


# ---- the scene lists both test modules walk ---------------------------------------------------------------------------------
FAR = [(1000.0, 0.0, 1000.0), (-1000.0, 0.0, -1000.0), (8000.0, 0.0, -8000.0), (-8000.0, 0.0, 8000.0), (-40.0, -10.0, -40.0)]


def random_pair_cases():
    """[(case, forms)]: the seeded scenes of the pair search; forms = which of the three implementations the scene's size allows
    ("one": one workgroup, "wave": a wavefront per body, n <= 8 192; "lane": a lane per body, n > 8 192)"""
    small = ("one", "wave")
    boxes = tumbling_boxes(2000, 1)
    out = [(boxes, small)] + [(boxes.moved(o), small) for o in FAR]
    big = tumbling_boxes(9000, 2)
    out += [(big, ("lane",)), (big.moved(FAR[1]), ("lane",))]
    cube = mixed(1500, 3, cube_hull(), none_share=0.05, name="cube")
    out += [(cube, small), (cube.moved(FAR[0]), small)]
    tea = mixed(600, 4, teapot_hull(), none_share=0.05, name="teapot")
    out += [(tea, small), (tea.moved(FAR[3]), small)]
    out += [(mixed(9000, 6, cube_hull(), none_share=0.02, name="cube"), ("lane",))]
    return out


def sparse_mixed(n, seed, hull, pitch=2.6, jitter=0.9, none_share=0.03):
    """spheres, boxes and hulls on a jittered grid: most bounding spheres apart (positive zones, some bound by the cap, some by a
    neighbour), a few touching or overlapping"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    pos = np.stack([pitch * (k % side), rng.uniform(0.0, 4.0, n), pitch * (k // side)], 1)
    pos[:, [0, 2]] += rng.uniform(-jitter, jitter, size=(n, 2)) - 0.5 * pitch * side
    g = rng.integers(1, 4, size=n).astype(np.uint8)
    sides = rng.uniform(0.3, 1.0, size=(n, 3))
    sides[g == GEOM_SPHERE, 0] = rng.uniform(0.2, 0.8, size=int((g == GEOM_SPHERE).sum()))
    sides[g == GEOM_CONVEX, 0] = hull_radius(hull)
    g[rng.random(n) < none_share] = GEOM_NONE
    return Case(f"sparse{n}s{seed}", pos, _unit_quats(rng, n), sides, g, hull)
