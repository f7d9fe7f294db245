"""Scenes and rays of the ray-cast tests (tests/test_gpu_raycast.py on the device; tests/test_ray_reference.py checks, with the
reference alone, that each scene leaves at most its allowed share of rays inside the band: 0.2 % near the origin, 5 % for scenes
moved 8 km out).  Everything is drawn from a seed; arrays are float64 and rounded by whoever uploads them."""
import numpy as np

from __graft_entry__ import load_package

import bp_scenes as sc
import ray_reference as rr

PLANE = (0.0, 1.0, 0.0, -1.0)          # the ground: y = -1, below every body
SEED = 35                              # of the rays: one for which every scene below keeps its band share under its cap


def cube_planes():
    return load_package().hull.planes(sc.cube_hull())


def statics_for(extent):
    """two static boxes: a platform above the bodies and a tilted wall beside them"""
    return [((2.0, 0.5, 2.0), (0.25, 3.75, -0.5), sc.IDENT_R12),
            ((0.75, 3.0, 2.0), (0.5 * extent + 1.5, 1.0, 0.25), sc.rot_y_z(0.3, 0.2))]


def mixed_case(n, seed=11):
    ext = 3.0 * np.sqrt(n)
    c = sc.mixed(n, seed, sc.cube_hull(), extent=ext)
    return sc.with_statics(c, statics_for(ext), "st")


def thin_case():
    """320 spheres of radius 0.4 (cell 1.0) one cell apart along x: ten torus periods share every bucket, the table overflows and
    goes to scrambled hashing"""
    rng = np.random.default_rng(21)
    n = 320
    pos = np.stack([np.arange(n) * 1.0 + 0.5, rng.uniform(0.0, 1.5, n), rng.uniform(0.0, 0.9, n)], 1)
    sides = np.zeros((n, 3)); sides[:, 0] = 0.4
    return sc.Case("thin320", pos, sc._ident_quats(n), sides, np.full(n, rr.GEOM_SPHERE, np.uint8))


def cases():
    """name -> (case, number of rays, near the origin?)"""
    m192 = mixed_case(192)
    return {
        "mixed1": (mixed_case(1), 2048, True),
        "mixed70": (mixed_case(70), 2048, True),
        "mixed192": (m192, 2048, True),
        "mixed192far": (m192.moved((8000.0, 0.0, 8000.0), "mixed192far"), 2048, False),
        "thin": (thin_case(), 2048, True),
        "torus": (sc.torus_clusters(2, 0), 2048, True),
        "column": (sc.column(40), 2048, True),
    }


def make_rays(case, n, seed, far=False):
    """(n, 7) float64: half uniform through the scene's box, half aimed at random geoms with jitter from a few metres away;
    directions not normalised.

    far: the ray set of a scene 8 km out.  There tol = K_RAY eps M is 3 cm in float32, a tenth of a small box's face: with the
    rays above 15 % would sit in the band (measured with the reference alone; nearly all by the margin rule: a hit point or a
    passing line within 3 cm of an edge or a silhouette), three times the 5 % such a scene may leave there.  So these rays are
    aimed at what has room for them -- sphere centres, the static boxes and the ground below them -- from one to three metres
    away, with a third of the jitter, and one ray in eight is uniform; boxes and hulls are still hit by what passes them."""
    rng = np.random.default_rng(seed)
    live = np.flatnonzero(case.gtype != rr.GEOM_NONE)
    centre = case.pos[live]
    if case.statics:          # (weighted so that about a tenth of the aimed rays go for a static box)
        centre = np.concatenate([centre, np.repeat(np.array([s[1] for s in case.statics], np.float64), max(1, len(live) // 16), 0)])
    lo, hi = centre.min(0) - 3.0, centre.max(0) + 3.0
    lo[1], hi[1] = centre[:, 1].min() - 1.5, centre[:, 1].max() + 4.0
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    L = rng.uniform(0.5, 8.0, n)
    aimed = np.arange(n) >= (n // 8 if far else n // 2)
    if far:
        sph = case.pos[case.gtype == rr.GEOM_SPHERE]
        ground = sph * np.array([1.0, 0.0, 1.0]) + np.array([0.0, -1.0, 0.0])
        stat = np.array([s[1] for s in case.statics], np.float64).reshape(-1, 3)
        pool = np.concatenate([sph, sph, ground, np.repeat(stat, max(1, len(sph) // 8), 0)])
        tgt = pool[rng.integers(0, len(pool), n)] + rng.normal(scale=0.05, size=(n, 3))
    else:
        tgt = centre[rng.integers(0, len(centre), n)] + rng.normal(scale=0.15, size=(n, 3))
    back = rng.normal(size=(n, 3))
    back /= np.linalg.norm(back, axis=1, keepdims=True)
    if far:
        back[:, 1] = np.abs(back[:, 1]) + 0.5          # from above: the ground is hit steeply
        back /= np.linalg.norm(back, axis=1, keepdims=True)
    dist = rng.uniform(1.0, 3.0 if far else 8.0, n)
    o[aimed] = (tgt + back * dist[:, None])[aimed]
    d[aimed] = -back[aimed]
    L[aimed] = (dist * rng.uniform(0.9, 1.6, n))[aimed]
    d *= rng.uniform(0.5, 2.0, n)[:, None]
    return np.concatenate([o, d, L[:, None]], 1)


def rounded_scene(case, dtype, plane=PLANE, planes=None, alive=None):
    """the reference's Scene from a Case rounded on the host the way an upload rounds it (quaternions normalised in T)"""
    T = np.dtype(dtype)
    q = case.quat.astype(T)
    q = q / np.sqrt((q * q).sum(1, dtype=T))[:, None]
    has_hull = case.hull is not None
    return rr.Scene(T, case.pos.astype(T), q, case.sides.astype(T), case.gtype, alive,
                    case.hull if has_hull else None, (cube_planes() if planes is None else planes) if has_hull else None,
                    case.statics, plane)
