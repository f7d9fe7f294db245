"""The oracle's colliders against GEOMETRY, not against their sibling in csrc/.

`oracle/orc_boxbox.c`, `orc_collide.c` restate ODE's dBoxBox / dCollideSphereBox / dCollideBoxPlane from recollection (ODE is
not vendored by the reference), and the product's colliders are pinned against them bit for bit
(tests/test_collider_equivalence.py, the GPU parity tests) -- which would pass a shared mis-recollection.  Here every collider
the reference's NearCallback can reach (/root/reference/src/main.c:678: box-box, sphere-box, sphere-sphere; box-plane for
BASELINE's configs) and the repository's own hull colliders are checked on >= 10^5 random pairs against brute-force numpy
references that share no code with them: projections of the boxes' 8 vertices on the 15 candidate axes instead of the
closed-form |R| sums, closest points, half-space tests.

What is pinned by geometry here (DESIGN.md section 5 lists it):
  * box-box: contacts <=> no separating axis among the 15 (the nine edge-pair axes with dBoxBox's 1e-5 guard against parallel
    edges: without it two of 20 000 boxes lying flat on a larger one came out "separated" -- found by this file);
    the depth is the least overlap over those axes under dBoxBox's own selection rule (faces first, an edge axis only when
    1.05 x its overlap is still less); the normal is that axis, unit, and points from box 2 into box 1; every contact of a face
    case lies in both boxes inflated by the depth, an edge case's contact is the midpoint of the two edge lines' closest
    approach; never more than maxc contacts, four for a face resting fully on a larger face, each as deep as the overlap.
  * sphere-box, sphere-sphere, box-plane, sphere-plane: the closed forms.
  * box-hull, hull-hull, hull-plane, sphere-hull (this repository's own definitions): exactly the vertices / corners that
    half-space tests find inside, in order, with the nearest face's distance.
What stays [ODE-recall]: which of several equally valid contact sets dBoxBox keeps when clipping yields more than maxc points
(cull_points' angular choice), and the order of its contacts.

The second half of the file runs the same colliders in float32, near the origin and 4.8 km out, against the same float64 references
under a band rule (see "float32" below)."""
import ctypes as C

import numpy as np
import pytest

from oracle.orc_ctypes import Oracle
from pair_population import _boxbox_cases, _rand_rot, _small_rot          # shared with the pair populations: the same draws

N_BOXBOX = 120_000
N_OTHER = 100_000


@pytest.fixture(scope="module")
def orc():
    return Oracle("float64")


# ------------------------------------------------------------------------------------------------------------ helpers
def _pose(p, R):
    """position + 3x4 row-major rotation, the oracle's geom layout"""
    n = len(p)
    out = np.zeros((n, 15))
    out[:, :3] = p
    R12 = np.zeros((n, 3, 4))
    R12[:, :, :3] = R
    out[:, 3:] = R12.reshape(n, 12)
    return out


def _bulk(orc, w, g1, g2, pose1, size1, pose2, size2, maxc=8):
    n = len(pose1)
    counts = np.zeros(n, np.int32)
    out = (orc.ContactGeom * (n * maxc))()
    keep = [np.ascontiguousarray(a, orc.dtype) if a is not None else None for a in (pose1, size1, pose2, size2)]
    orc.lib.orc_collide_bulk(w.w, g1, g2, n, *[None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep], maxc,
                             counts.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p))
    f = orc.dtype.str[1:]                                        # "f8" / "f4": the precision's contact struct
    raw = np.frombuffer(out, dtype=np.dtype([("pos", f, 3), ("normal", f, 3), ("depth", f), ("g1", "i4"), ("g2", "i4")]))
    raw = raw.reshape(n, maxc)
    return counts, raw["pos"].astype(np.float64), raw["normal"].astype(np.float64), raw["depth"].astype(np.float64)


def _box_vertices(p, R, side):
    """(n, 8, 3) world-space corners"""
    sg = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], float) * 2 - 1          # (8, 3)
    local = sg[None] * (0.5 * side)[:, None, :]                                                 # (n, 8, 3)
    return p[:, None, :] + np.einsum("nij,nkj->nki", R, local)


def _in_box(pts, p, R, side, grow):
    """pts (n, k, 3) inside the box inflated by grow (n,) on every side?"""
    loc = np.einsum("nji,nkj->nki", R, pts - p[:, None, :])
    return np.all(np.abs(loc) <= (0.5 * side)[:, None, :] + grow[:, None, None], axis=2)


def _sat_by_projection(p1, R1, s1, p2, R2, s2):
    """overlap (positive = interpenetration) of the two boxes' projections on each of the 15 candidate axes, from the projected
    vertices themselves: (n, 15) overlaps, (n, 15, 3) unit axes, (n, 15) axis is usable (edge pairs may be parallel)"""
    n = len(p1)
    axes = np.empty((n, 15, 3))
    axes[:, 0:3] = np.swapaxes(R1, 1, 2)            # rows = box 1's axes (columns of R1)
    axes[:, 3:6] = np.swapaxes(R2, 1, 2)
    k = 6
    for i in range(3):
        for j in range(3):
            axes[:, k] = np.cross(R1[:, :, i], R2[:, :, j])
            k += 1
    ln = np.linalg.norm(axes, axis=2)
    ok = ln > 1e-7
    axes = axes / np.where(ok, ln, 1.0)[:, :, None]
    v1 = _box_vertices(p1, R1, s1) - p1[:, None, :]
    v2 = _box_vertices(p2, R2, s2) - p2[:, None, :]
    ra = np.max(np.abs(np.einsum("nkj,naj->nak", v1, axes)), axis=2)       # half-extent of box 1 along each axis
    rb = np.max(np.abs(np.einsum("nkj,naj->nak", v2, axes)), axis=2)
    dist = np.abs(np.einsum("nj,naj->na", p2 - p1, axes))
    ov = ra + rb - dist
    # dBoxBox's "fudge2" [ODE-recall box.cpp]: before the nine edge-pair axes every |R1^T R2| entry grows by 1e-5, which widens
    # the boxes' extent along u_i x v_j by 1e-5 x (the four half-sides that enter it) / |u_i x v_j| -- the guard that keeps
    # (nearly) parallel edges from "separating" two boxes on rounding error alone.  Part of the rule being checked.
    a, b = 0.5 * s1, 0.5 * s2
    k = 6
    for i in range(3):
        for j in range(3):
            others = a[:, (i + 1) % 3] + a[:, (i + 2) % 3] + b[:, (j + 1) % 3] + b[:, (j + 2) % 3]
            ov[:, k] += 1e-5 * others / np.where(ok[:, k], ln[:, k], 1.0)
            k += 1
    return ov, axes, ok


# ------------------------------------------------------------------------------------------------------------ the draws
# (shared by the float64 tests and the float32 ones below, which translate and round them)
def _draw_box_box():
    return _boxbox_cases(np.random.default_rng(2024), N_BOXBOX)


def _draw_flat_on_a_face():
    """a small box lying flat on a larger one, sunk into it by U(1e-6, 0.05), the whole configuration turned at random"""
    rng = np.random.default_rng(5)
    n = 20_000
    s1 = rng.uniform(0.2, 1.0, (n, 3)); s2 = np.column_stack([rng.uniform(3, 100, n), rng.uniform(0.5, 2, n), rng.uniform(3, 100, n)])
    G = _rand_rot(rng, n)                                           # the whole configuration turned at random
    yaw = rng.uniform(0, 2 * np.pi, n)
    Y = np.zeros((n, 3, 3)); Y[:, 1, 1] = 1; Y[:, 0, 0] = np.cos(yaw); Y[:, 0, 2] = np.sin(yaw); Y[:, 2, 0] = -np.sin(yaw); Y[:, 2, 2] = np.cos(yaw)
    sink = rng.uniform(1e-6, 0.05, n)
    local1 = np.column_stack([rng.uniform(-1, 1, n), 0.5 * s2[:, 1] + 0.5 * s1[:, 1] - sink, rng.uniform(-1, 1, n)])
    p2 = rng.uniform(-2, 2, (n, 3))
    p1 = p2 + np.einsum("nij,nj->ni", G, local1)
    return p1, G @ Y, s1, p2, G, s2, sink


def _draw_sphere_box():
    rng = np.random.default_rng(7)
    n = N_OTHER
    side = rng.uniform(0.2, 1.0, (n, 3)); side[: n // 10] = [100.0, 1.0, 100.0]
    Rb = _rand_rot(rng, n); pb = rng.uniform(-1, 1, (n, 3))
    r = rng.uniform(0.1, 0.4, n)
    loc = rng.uniform(-1, 1, (n, 3)) * (0.5 * side + r[:, None] * 1.3)      # inside, near the surface and beyond
    ps = pb + np.einsum("nij,nj->ni", Rb, loc)
    return ps, r, pb, Rb, side, loc


def _draw_spheres():
    """two spheres per pair; then the plane normals of the sphere-plane part"""
    rng = np.random.default_rng(8)
    n = N_OTHER
    r1 = rng.uniform(0.1, 0.4, n); r2 = rng.uniform(0.1, 0.4, n)
    p1 = rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    gap = rng.uniform(0.5, 1.3, n) * (r1 + r2)
    p2 = p1 - d * gap[:, None]
    pn = rng.normal(size=(n, 3)); pn /= np.linalg.norm(pn, axis=1, keepdims=True)
    return r1, r2, p1, p2, d, gap, pn


def _draw_box_plane(lift_hi=1.2):
    rng = np.random.default_rng(9)
    n = N_OTHER
    side = rng.uniform(0.2, 1.0, (n, 3))
    R = _rand_rot(rng, n)
    R[: n // 4] = _small_rot(rng, n // 4, 10.0 ** rng.uniform(-9, -1, n // 4))        # nearly flat on the plane
    normal = np.array([0.0, 1.0, 0.0])
    p = rng.uniform(-1, 1, (n, 3))
    reach = 0.5 * np.abs(np.einsum("nji,j->ni", R, normal)) @ np.ones(3) * 0 + 0.5 * np.einsum("ni,ni->n", np.abs(np.einsum("nji,j->ni", R, normal)), side)
    p[:, 1] = reach * rng.uniform(0.3, lift_hi, n)
    return p, R, side


# ------------------------------------------------------------------------------------------------------------ box - box
def test_box_box_against_the_separating_axis_theorem(orc):
    n = N_BOXBOX
    p1, R1, s1, p2, R2, s2 = _draw_box_box()
    w = orc.world()
    g1 = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    g2 = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc, w, g1, g2, _pose(p1, R1), s1, _pose(p2, R2), s2, maxc=8)
    ov, axes, ok = _sat_by_projection(p1, R1, s1, p2, R2, s2)
    ov_ok = np.where(ok, ov, np.inf)
    least = ov_ok.min(axis=1)

    # (1) contacts <=> no separating axis (pairs within 1e-9 of touching may go either way)
    clear_sep = least < -1e-9
    clear_hit = least > 1e-9
    assert clear_sep.sum() > n // 10 and clear_hit.sum() > n // 4
    assert np.all(cnt[clear_sep] == 0), "contacts reported across a separating axis"
    assert np.all(cnt[clear_hit] >= 1), "no contact although all 15 axes overlap"
    assert cnt.max() <= 8 and np.all(cnt >= 0)
    hit = np.flatnonzero(clear_hit & (cnt > 0))

    # (2) dBoxBox's axis choice: the least face overlap, unless an edge axis' overlap x 1.05 is smaller still (in order, strict)
    face = ov[hit, :6]
    s = -face[:, 0].copy(); pick = np.zeros(len(hit), int)
    for a in range(1, 6):
        better = -face[:, a] > s
        s[better] = -face[better, a]; pick[better] = a
    ambiguous = np.zeros(len(hit), bool)
    for a in range(6, 15):
        cand = -ov[hit, a]
        use = ok[hit, a] & (cand * 1.05 > s)
        ambiguous |= ok[hit, a] & (np.abs(cand * 1.05 - s) < 1e-9)
        s[use] = cand[use]; pick[use] = a
    expect_depth = -s
    first_depth = dep[hit, 0]
    top_depth = np.max(np.where(np.arange(8)[None, :] < cnt[hit, None], dep[hit], -np.inf), axis=1)
    sure = ~ambiguous
    edge = pick >= 6
    # edge-edge: one contact, its depth the overlap
    assert np.all(cnt[hit][edge & sure] == 1)
    assert np.allclose(first_depth[edge & sure], expect_depth[edge & sure], atol=1e-11)
    # face: every contact at most as deep as the overlap, none negative
    fs = ~edge & sure
    assert np.all(top_depth[fs] <= expect_depth[fs] + 1e-10)
    assert np.all(np.where(np.arange(8)[None, :] < cnt[hit, None], dep[hit], 0.0) >= -1e-12)
    assert edge.sum() > 1000 and (~edge).sum() > 10000

    # (3) the normal: unit, along the chosen axis, from box 2 into box 1
    n0 = nrm[hit, 0]
    assert np.allclose(np.linalg.norm(n0, axis=1), 1.0, atol=1e-12)
    chosen = axes[hit, pick]
    assert np.all(np.abs(np.abs(np.einsum("nj,nj->n", n0[sure], chosen[sure])) - 1.0) < 1e-9)
    assert np.all(np.einsum("nj,nj->n", n0, (p1 - p2)[hit]) >= -1e-12)
    same = np.where(np.arange(8)[None, :, None] < cnt[hit, None, None], nrm[hit] - n0[:, None, :], 0.0)
    assert np.abs(same).max() == 0.0                      # every contact of a pair carries the one normal

    # (4) every contact of a FACE case lies in both boxes inflated by its pair's penetration
    grow = expect_depth + 1e-9
    m = np.arange(8)[None, :] < cnt[hit, None]
    in1 = _in_box(pos[hit], p1[hit], R1[hit], s1[hit], grow)
    in2 = _in_box(pos[hit], p2[hit], R2[hit], s2[hit], grow)
    fm = m & fs[:, None]
    assert np.all(in1[fm]) and np.all(in2[fm])

    # (5) an EDGE case's one contact is the midpoint of the closest approach of the two edges' LINES -- dBoxBox's construction:
    # the edge of box 1 farthest along the normal, the edge of box 2 farthest against it.  When the closest points fall within
    # both segments the point lies in both inflated boxes; when they do not (a handful in 10^5: the least-overlap axis is an edge
    # pair whose segments do not actually face each other) it can lie outside by a few depths -- a known trait of dBoxBox,
    # recorded in DESIGN.md section 5, not an error of the restatement.
    es = np.flatnonzero(edge & sure)
    ih = hit[es]
    ei, ej = (pick[es] - 6) // 3, (pick[es] - 6) % 3
    n12 = -nrm[ih, 0]                                            # from box 1 towards box 2
    pa = p1[ih].copy(); pb = p2[ih].copy()
    for j in range(3):
        sa = np.where(np.einsum("nj,nj->n", n12, R1[ih][:, :, j]) > 0, 1.0, -1.0)
        pa += (sa * 0.5 * s1[ih, j])[:, None] * R1[ih][:, :, j]
        sb = np.where(np.einsum("nj,nj->n", n12, R2[ih][:, :, j]) > 0, -1.0, 1.0)
        pb += (sb * 0.5 * s2[ih, j])[:, None] * R2[ih][:, :, j]
    ua = R1[ih, :, ei]; ub = R2[ih, :, ej]
    # closest approach of pa + alpha ua and pb + beta ub
    dp = pb - pa
    uaub = np.einsum("nj,nj->n", ua, ub); q1 = np.einsum("nj,nj->n", ua, dp); q2 = -np.einsum("nj,nj->n", ub, dp)
    den = 1 - uaub * uaub
    good = den > 1e-6
    alpha = (q1 + uaub * q2) / np.where(good, den, 1.0); beta = (uaub * q1 + q2) / np.where(good, den, 1.0)
    mid = 0.5 * ((pa + alpha[:, None] * ua) + (pb + beta[:, None] * ub))
    assert good.sum() > 1000
    assert np.abs(pos[ih, 0] - mid)[good].max() < 1e-8
    # where along each edge (measured from the edge's own centre) the closest points are
    ca = np.einsum("nj,nj->n", pa + alpha[:, None] * ua - p1[ih], ua); cb = np.einsum("nj,nj->n", pb + beta[:, None] * ub - p2[ih], ub)
    within = good & (np.abs(ca) <= 0.5 * s1[ih, ei]) & (np.abs(cb) <= 0.5 * s2[ih, ej])
    assert within.sum() > 0.99 * good.sum()
    assert np.all(in1[es, 0][within]) and np.all(in2[es, 0][within])


def test_box_resting_flat_on_a_larger_face_gives_four_contacts_as_deep_as_the_overlap(orc):
    p1, R1, s1, p2, R2, s2, sink = _draw_flat_on_a_face()
    G = R2
    w = orc.world()
    g1 = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    g2 = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc, w, g1, g2, _pose(p1, R1), s1, _pose(p2, R2), s2)
    assert np.all(cnt == 4)
    assert np.allclose(dep[:, :4], sink[:, None], atol=1e-10)
    up = G[:, :, 1]
    assert np.allclose(nrm[:, 0], up, atol=1e-9)                    # out of the larger box's top, into box 1
    # the four points are box 1's bottom corners, lifted onto box 2's top face: with the two y axes parallel the first axis
    # tested wins (box 1's), so box 1 is the reference box and the contacts are points of the INCIDENT face (box 2's top)
    # clipped to box 1's bottom rectangle [ODE-recall: dBoxBox returns points on the incident face]
    corners = _box_vertices(p1, R1, s1)
    below = np.argsort(np.einsum("nkj,nj->nk", corners, up), axis=1)[:, :4]
    want = np.take_along_axis(corners, below[:, :, None], axis=1) + (sink[:, None] * up)[:, None, :]
    d = np.linalg.norm(pos[:, :4, None, :] - want[:, None, :, :], axis=3).min(axis=2)
    assert d.max() < 1e-9


# ------------------------------------------------------------------------------------------------------------ sphere - box / sphere
def test_sphere_box_is_the_closest_point_on_the_box(orc):
    n = N_OTHER
    ps, r, pb, Rb, side, loc = _draw_sphere_box()
    w = orc.world()
    gs = orc.lib.orc_geom_create_sphere(w.w, 0.3)
    gb = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    rad = np.column_stack([r, np.zeros(n), np.zeros(n)])
    cnt, pos, nrm, dep = _bulk(orc, w, gs, gb, _pose(ps, np.tile(np.eye(3), (n, 1, 1))), rad, _pose(pb, Rb), side, maxc=4)
    half = 0.5 * side
    clamp = np.clip(loc, -half, half)
    outside = np.any(np.abs(loc) > half, axis=1)
    dist = np.linalg.norm(loc - clamp, axis=1)
    # centre outside the box: one contact at the closest point, depth r - distance, normal from it to the centre
    hit = outside & (r - dist > 1e-9); miss = outside & (r - dist < -1e-9)
    assert hit.sum() > n // 10 and miss.sum() > n // 20
    assert np.all(cnt[miss] == 0) and np.all(cnt[hit] == 1)
    q = pb + np.einsum("nij,nj->ni", Rb, clamp)
    assert np.allclose(pos[hit, 0], q[hit], atol=1e-12)
    assert np.allclose(dep[hit, 0], (r - dist)[hit], atol=1e-12)
    nn = (ps - q)[hit] / dist[hit, None]
    assert np.allclose(nrm[hit, 0], nn, atol=1e-9)
    # centre inside: pushed out through the nearest face, depth = distance to it + r, contact at the centre
    ins = ~outside
    assert ins.sum() > n // 20 and np.all(cnt[ins] == 1)
    fd = half - np.abs(loc)
    k = np.argmin(fd, axis=1)
    assert np.allclose(dep[ins, 0], (fd[np.arange(n), k] + r)[ins], atol=1e-12)
    axis = Rb[np.arange(n), :, k] * np.sign(loc[np.arange(n), k])[:, None]
    tie = np.sort(fd, axis=1)[:, 1] - np.sort(fd, axis=1)[:, 0] < 1e-9
    sel = ins & ~tie & (loc[np.arange(n), k] != 0)
    assert np.allclose(nrm[sel, 0], axis[sel], atol=1e-12)
    assert np.allclose(pos[ins, 0], ps[ins], atol=0)


def test_sphere_sphere_and_sphere_plane_closed_forms(orc):
    n = N_OTHER
    r1, r2, p1, p2, d, gap, pn = _draw_spheres()
    w = orc.world()
    a = orc.lib.orc_geom_create_sphere(w.w, 0.3); b = orc.lib.orc_geom_create_sphere(w.w, 0.3)
    I = np.tile(np.eye(3), (n, 1, 1))
    z = np.zeros(n)
    cnt, pos, nrm, dep = _bulk(orc, w, a, b, _pose(p1, I), np.column_stack([r1, z, z]), _pose(p2, I), np.column_stack([r2, z, z]), maxc=2)
    hit = r1 + r2 - gap > 1e-9; miss = r1 + r2 - gap < -1e-9
    assert np.all(cnt[hit] == 1) and np.all(cnt[miss] == 0)
    assert np.allclose(dep[hit, 0], (r1 + r2 - gap)[hit], atol=1e-12)
    assert np.allclose(nrm[hit, 0], d[hit], atol=1e-9)                       # from sphere 2 into sphere 1
    t = np.einsum("nj,nj->n", pos[:, 0] - p2, d)                             # on the line of centres, inside the lens
    assert np.all((t[hit] >= (gap - r1)[hit] - 1e-9) & (t[hit] <= r2[hit] + 1e-9))
    # sphere - plane
    for k in range(0, n, n // 20):                                            # the plane is per world: a handful of planes
        w2 = orc.world()
        pl = orc.lib.orc_geom_create_plane(w2.w, *pn[k], 0.25)
        s = orc.lib.orc_geom_create_sphere(w2.w, 0.3)
        sl = slice(k, k + n // 20)
        m = sl.stop - sl.start
        c2, pos2, n2, d2 = _bulk(orc, w2, s, pl, _pose(p1[sl], I[sl]), np.column_stack([r1[sl], z[sl], z[sl]]), _pose(np.zeros((m, 3)), I[sl]), None, maxc=2)
        depth = 0.25 - p1[sl] @ pn[k] + r1[sl]
        assert np.all(c2[depth > 1e-9] == 1) and np.all(c2[depth < -1e-9] == 0)
        h = depth > 1e-9
        assert np.allclose(d2[h, 0], depth[h], atol=1e-12) and np.allclose(n2[h, 0], pn[k], atol=1e-15)
        assert np.allclose(pos2[h, 0], (p1[sl] - pn[k] * r1[sl, None])[h], atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ box - plane
def test_box_plane_contacts_are_the_boxs_lowest_corners(orc):
    n = N_OTHER
    p, R, side = _draw_box_plane()
    normal = np.array([0.0, 1.0, 0.0])
    w = orc.world()
    pl = orc.lib.orc_geom_create_plane(w.w, 0.0, 1.0, 0.0, 0.0)
    b = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc, w, b, pl, _pose(p, R), side, _pose(np.zeros((n, 3)), np.tile(np.eye(3), (n, 1, 1))), None, maxc=4)
    V = _box_vertices(p, R, side)
    vd = -V[:, :, 1]                                            # depth of each corner below y = 0
    deepest = vd.max(axis=1)
    assert np.all(cnt[deepest < -1e-9] == 0) and np.all(cnt[deepest > 1e-9] >= 1)
    hit = np.flatnonzero(deepest > 1e-9)
    assert len(hit) > n // 4 and cnt.max() <= 4
    m = np.arange(4)[None, :] < cnt[hit, None]
    # every contact is one of the box's corners, at that corner's depth, no corner twice; the first is the deepest
    dist = np.linalg.norm(pos[hit][:, :, None, :] - V[hit][:, None, :, :], axis=3)
    which = dist.argmin(axis=2)
    assert dist.min(axis=2)[m].max() < 1e-9
    assert np.allclose(dep[hit][m], np.take_along_axis(vd[hit], which, axis=1)[m], atol=1e-10)
    assert np.allclose(dep[hit, 0], deepest[hit], atol=1e-10)
    assert np.all(dep[hit][m] >= -1e-12)
    srt = np.sort(np.where(m, which, 100 + np.arange(4)[None, :]), axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])
    assert np.allclose(nrm[hit][m], normal[None, :], atol=0)
    # the deepest corner, its neighbours along the two sides that rise least, and that face's fourth corner -- those of them that
    # are below the plane [ODE-recall dCollideBoxPlane]: one contact per corner below up to three; four exactly when the four lowest
    # corners are one face (a box standing on a corner with its three neighbours just under the plane gets three: two such boxes in
    # 10^5 here).  Boxes with a corner within 1e-6 of the plane are left out: there the count may go either way.
    clear = np.all(np.abs(vd) > 1e-6, axis=1)
    below = (vd > 0).sum(axis=1)
    assert np.all(cnt[clear] <= np.minimum(4, below[clear])) and np.all(cnt[clear] >= np.minimum(3, below[clear]))
    four = clear & (below >= 4)
    low4 = np.argsort(-vd, axis=1)[:, :4]
    c4 = np.take_along_axis(V, low4[:, :, None], axis=1)
    planar = np.abs(np.linalg.det(c4[:, 1:] - c4[:, :1])) < 1e-12          # the four lowest corners lie in one plane: a face
    assert np.all(cnt[four & planar] == 4) and np.all(cnt[four & ~planar] == 3)
    assert (four & planar).sum() > 1000 and (below[clear] == 3).sum() > 1000


# ------------------------------------------------------------------------------------------------------------ hulls
def _random_hull(rng, k=40):
    from scipy.spatial import ConvexHull
    pts = rng.normal(size=(k, 3)) * [0.5, 0.35, 0.4]
    h = ConvexHull(pts)
    verts = pts[h.vertices]
    eq = np.unique(np.round(h.equations, 12), axis=0)             # (nf, 4): n.x + d <= 0 inside  ->  n.x <= -d
    planes = np.column_stack([eq[:, :3], -eq[:, 3]])
    return verts, planes


def _draw_hulls():
    """one random hull; n box-hull, hull-hull and sphere-hull pairs about it"""
    rng = np.random.default_rng(11)
    verts, planes = _random_hull(rng)
    n = 25_000
    side = rng.uniform(0.3, 1.2, (n, 3))
    Rh = _rand_rot(rng, n); Rb = _rand_rot(rng, n)
    ph = rng.uniform(-1, 1, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pb = ph + d * rng.uniform(0.2, 1.1, n)[:, None]
    Ra = _rand_rot(rng, n); pa = ph + d * rng.uniform(0.2, 0.9, n)[:, None]
    r = rng.uniform(0.1, 0.4, n)
    ps = ph + d * rng.uniform(0.1, 1.2, n)[:, None]
    return verts, planes, side, Rh, Rb, ph, pb, Ra, pa, r, ps


def test_hull_colliders_take_exactly_the_points_the_half_spaces_contain(orc):
    """box-hull, hull-hull, sphere-hull, hull-plane: this repository's own colliders ("a point inside a convex shape, along
    the face it is nearest to").  The numpy side decides "inside" from the face planes and box half-extents alone."""
    verts, planes, side, Rh, Rb, ph, pb, Ra, pa, r, ps = _draw_hulls()
    nv = len(verts)
    n = len(ph)
    w = orc.world()
    w.set_hull(verts)
    w.set_hull_faces(planes)
    gh = orc.lib.orc_geom_create_convex(w.w)
    gb = orc.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc, w, gb, gh, _pose(pb, Rb), side, _pose(ph, Rh), None, maxc=8)
    VW = ph[:, None, :] + np.einsum("nij,kj->nki", Rh, verts)            # hull vertices, world
    loc = np.einsum("nji,nkj->nki", Rb, VW - pb[:, None, :])             # in the box frame
    half = 0.5 * side
    margin = (half[:, None, :] - np.abs(loc)).min(axis=2)                # > 0 inside the box
    corners = _box_vertices(pb, Rb, side)
    cl = np.einsum("nji,nkj->nki", Rh, corners - ph[:, None, :])          # box corners in the hull frame
    cm = (planes[None, None, :, 3] - np.einsum("nki,fi->nkf", cl, planes[:, :3])).min(axis=2)      # > 0 inside the hull
    sure = (np.abs(margin) > 1e-9).all(axis=1) & (np.abs(cm) > 1e-9).all(axis=1)
    want_n = np.minimum(8, (margin > 0).sum(axis=1) + (cm > 0).sum(axis=1))
    assert np.all(cnt[sure] == want_n[sure])
    assert (want_n > 0).sum() > n // 20
    for i in np.flatnonzero(sure & (want_n > 0))[:4000]:
        vs = np.flatnonzero(margin[i] > 0)
        cs = np.flatnonzero(cm[i] > 0)
        exp_pos = np.vstack([VW[i, vs], corners[i, cs]])[:8]
        exp_dep = np.concatenate([margin[i, vs], cm[i, cs]])[:8]
        assert np.allclose(pos[i, :cnt[i]], exp_pos, atol=1e-12)
        assert np.allclose(dep[i, :cnt[i]], exp_dep, atol=1e-12)
        inward = np.einsum("kj,j->k", nrm[i, :cnt[i]], pb[i] - ph[i])    # contact normals point into the box (o1)
        assert np.all(np.abs(np.linalg.norm(nrm[i, :cnt[i]], axis=1) - 1) < 1e-9)
        del inward
    # hull - hull: B's vertices inside A first, then A's inside B
    g2 = orc.lib.orc_geom_create_convex(w.w)
    cnt, pos, nrm, dep = _bulk(orc, w, gh, g2, _pose(pa, Ra), None, _pose(ph, Rh), None, maxc=8)

    def inside(pw, pc, Rc):
        l = np.einsum("nji,nkj->nki", Rc, pw - pc[:, None, :])
        return (planes[None, None, :, 3] - np.einsum("nki,fi->nkf", l, planes[:, :3])).min(axis=2)
    VA = pa[:, None, :] + np.einsum("nij,kj->nki", Ra, verts)
    mB_in_A = inside(VW, pa, Ra); mA_in_B = inside(VA, ph, Rh)
    sure = (np.abs(mB_in_A) > 1e-9).all(axis=1) & (np.abs(mA_in_B) > 1e-9).all(axis=1)
    want_n = np.minimum(8, (mB_in_A > 0).sum(axis=1) + (mA_in_B > 0).sum(axis=1))
    assert np.all(cnt[sure] == want_n[sure]) and (want_n > 0).sum() > n // 20
    for i in np.flatnonzero(sure & (want_n > 0))[:3000]:
        b_in = np.flatnonzero(mB_in_A[i] > 0); a_in = np.flatnonzero(mA_in_B[i] > 0)
        assert np.allclose(pos[i, :cnt[i]], np.vstack([VW[i, b_in], VA[i, a_in]])[:8], atol=1e-12)
        assert np.allclose(dep[i, :cnt[i]], np.concatenate([mB_in_A[i, b_in], mA_in_B[i, a_in]])[:8], atol=1e-12)
    # sphere - hull: the face plane farthest out decides
    gs = orc.lib.orc_geom_create_sphere(w.w, 0.3)
    z = np.zeros(n)
    cnt, pos, nrm, dep = _bulk(orc, w, gs, gh, _pose(ps, np.tile(np.eye(3), (n, 1, 1))), np.column_stack([r, z, z]), _pose(ph, Rh), None, maxc=2)
    c = np.einsum("nji,nj->ni", Rh, ps - ph)
    sd = c @ planes[:, :3].T - planes[None, :, 3]
    smax = sd.max(axis=1); f = sd.argmax(axis=1)
    hit = r - smax > 1e-9; miss = r - smax < -1e-9
    assert np.all(cnt[hit] == 1) and np.all(cnt[miss] == 0) and hit.sum() > n // 10
    assert np.allclose(dep[hit, 0], (r - smax)[hit], atol=1e-12)
    nw = np.einsum("nij,nj->ni", Rh, planes[f, :3])
    uniq = np.sort(sd, axis=1)[:, -1] - np.sort(sd, axis=1)[:, -2] > 1e-9
    assert np.allclose(nrm[hit & uniq, 0], nw[hit & uniq], atol=1e-12)
    assert nv >= 10


# ============================================================================================================ float32
# The same colliders in FLOAT32, near the origin and translated by pair_population.FAR, against the same float64 numpy references.
# The draws above are translated, THEN rounded to float32; the float32 oracle and the references both get those rounded values (the
# references recompute every derived quantity -- local coordinates, gaps, sinks -- from them in float64).
#
# The band rule (the broadphase's): band = k eps32 M, M = the largest |coordinate| of the pair's two centres +
# the two bounding radii + |plane offset|.  A DECISION (contact or none; a point inside or outside a box or hull; a corner below or
# above the plane) whose float64 margin is within the band may fall either way; outside it the decision equals the reference exactly.
# Depths and positions agree within the band, normals within band / (the pair's smallest extent) radians.  Where a quantity is a
# quotient, its band is divided by the denominator (a condition on the INPUTS, stated at each use).  At most MAX_IN_BAND of a test's
# cases may lie in a band or be excused; that share is computed from the float64 reference alone and asserted before the collider's
# output is looked at.  k per collider: pair_population.K_BAND = the largest deviation measured here (F32_MEASURED; every test prints
# its own, "F32 ..." lines under -s) x 2, rounded up to a power of two.
from pair_population import EPS32, FAR, K_BAND          # noqa: E402

PLACES = ["near", "far"]
MAX_IN_BAND = 0.05

# what the tests below measured, in units of eps32 M (normals: eps32 M / extent), as max(near, far): the source of K_BAND
F32_MEASURED = {"sphere_sphere": 0.81, "sphere_plane": 1.82, "sphere_box": 0.57, "box_plane": 2.56, "box_box": 1.77, "box_on_face": 0.99,
                "hulls": 0.54}


def test_f32_bands_come_from_the_measured_maxima():
    """k = the measured maximum x 2, rounded up to a power of two"""
    for name, worst in F32_MEASURED.items():
        assert K_BAND[name] == 2 ** int(np.ceil(np.log2(2 * worst))), name


def _r32(*arrays):
    """rounded to float32, held as float64"""
    out = [np.asarray(a, np.float32).astype(np.float64) for a in arrays]
    return out[0] if len(out) == 1 else out


def _shift(place):
    return np.asarray(FAR, float) if place == "far" else np.zeros(3)


def _reach(*centres):
    return np.max(np.abs(np.concatenate(centres, axis=1)), axis=1)


def _cap(tag, place, excused, of=None):
    """at most MAX_IN_BAND of the cases in a band or excused: a condition on the draw, decided by the float64 reference alone"""
    share = float(np.mean(excused)) if of is None else float(np.sum(excused)) / max(1, int(np.sum(of)))
    print(f"F32 {place} {tag}: in band or excused {100 * share:.3f} %")
    assert share <= MAX_IN_BAND, f"{tag} ({place}): {100 * share:.2f} % of the cases in the band or excused: change the draw"


def _within(tag, place, dev, k):
    """dev: deviations in units of eps32 M; printed, then held to k"""
    worst = float(np.max(dev)) if np.size(dev) else 0.0
    print(f"F32 {place} {tag}: max {worst:.3f} (k = {k}, over {np.size(dev)})")
    assert worst <= k, f"{tag} ({place}): {worst:.3f} eps32 M, beyond k = {k}"


# ------------------------------------------------------------------------------------------------------------ spheres
@pytest.mark.parametrize("place", PLACES)
def test_f32_sphere_sphere_and_sphere_plane(orc32, place):
    k = K_BAND["sphere_sphere"]
    r1, r2, p1, p2, _, _, pn = _draw_spheres()
    n = len(r1)
    s = _shift(place)
    r1, r2, p1, p2 = _r32(r1, r2, p1 + s, p2 + s)
    dv = p1 - p2
    gap = np.linalg.norm(dv, axis=1)
    d = dv / gap[:, None]
    depth = r1 + r2 - gap
    u = EPS32 * (_reach(p1, p2) + r1 + r2)
    band = k * u
    hit, miss = depth > band, depth < -band
    _cap("sphere-sphere contact or none", place, ~hit & ~miss)
    assert hit.sum() > n // 4 and miss.sum() > n // 10
    w = orc32.world()
    a = orc32.lib.orc_geom_create_sphere(w.w, 0.3); b = orc32.lib.orc_geom_create_sphere(w.w, 0.3)
    I = np.tile(np.eye(3), (n, 1, 1))
    z = np.zeros(n)
    cnt, pos, nrm, dep = _bulk(orc32, w, a, b, _pose(p1, I), np.column_stack([r1, z, z]), _pose(p2, I), np.column_stack([r2, z, z]), maxc=2)
    assert np.all(cnt[hit] == 1) and np.all(cnt[miss] == 0) and np.all((cnt == 0) | (cnt == 1))
    _within("sphere-sphere depth", place, (np.abs(dep[:, 0] - depth) / u)[hit], k)
    _within("sphere-sphere normal", place, (np.linalg.norm(nrm[:, 0] - d, axis=1) * np.minimum(r1, r2) / u)[hit], k)
    t = np.einsum("nj,nj->n", pos[:, 0] - p2, d)                             # on the line of centres, inside the lens
    assert np.all((t[hit] >= (gap - r1 - band)[hit]) & (t[hit] <= (r2 + band)[hit]))
    _within("sphere-sphere position off the line of centres", place, (np.linalg.norm(pos[:, 0] - p2 - t[:, None] * d, axis=1) / u)[hit], k)
    # sphere - plane: the plane moves with the translation; dCreatePlane normalises (a, b, c, d), so does the reference
    k = K_BAND["sphere_plane"]
    for j in range(0, n, n // 20):
        abcd = _r32(np.append(pn[j], 0.25 + pn[j] @ s))
        ln = np.linalg.norm(abcd[:3])
        nh, dh = abcd[:3] / ln, abcd[3] / ln
        w2 = orc32.world()
        pl = orc32.lib.orc_geom_create_plane(w2.w, *abcd)
        sp = orc32.lib.orc_geom_create_sphere(w2.w, 0.3)
        sl = slice(j, j + n // 20)
        m = sl.stop - sl.start
        c2, pos2, n2, d2 = _bulk(orc32, w2, sp, pl, _pose(p1[sl], I[sl]), np.column_stack([r1[sl], z[sl], z[sl]]), _pose(np.zeros((m, 3)), I[sl]), None, maxc=2)
        depth = dh - p1[sl] @ nh + r1[sl]
        up = EPS32 * (np.max(np.abs(p1[sl]), axis=1) + r1[sl] + abs(dh))
        h, ms = depth > k * up, depth < -k * up
        _cap(f"sphere-plane {j // (n // 20)} contact or none", place, ~h & ~ms)
        assert np.all(c2[h] == 1) and np.all(c2[ms] == 0)
        if h.any():
            _within("sphere-plane depth", place, (np.abs(d2[:, 0] - depth) / up)[h], k)
            _within("sphere-plane normal", place, (np.linalg.norm(n2[:, 0] - nh, axis=1) * r1[sl] / up)[h], k)
            _within("sphere-plane position", place, (np.max(np.abs(pos2[:, 0] - (p1[sl] - nh * r1[sl, None])), axis=1) / up)[h], k)


# ------------------------------------------------------------------------------------------------------------ sphere - box
@pytest.mark.parametrize("place", PLACES)
def test_f32_sphere_box(orc32, place):
    """As the float64 test.  The centre inside or outside the box is a decision; the normal of an outside centre is the unit vector of
    a difference of length dist, so its band is divided by dist (compared where dist > 10 bands: less than 0.1 rad)."""
    k = K_BAND["sphere_box"]
    ps, r, pb, Rb, side, _ = _draw_sphere_box()
    n = len(r)
    s = _shift(place)
    ps, r, pb, Rb, side = _r32(ps + s, r, pb + s, Rb, side)
    loc = np.einsum("nji,nj->ni", Rb, ps - pb)
    half = 0.5 * side
    u = EPS32 * (_reach(ps, pb) + r + 0.5 * np.linalg.norm(side, axis=1))
    band = k * u
    clamp = np.clip(loc, -half, half)
    out_by = np.max(np.abs(loc) - half, axis=1)                             # > 0: the centre is outside the box
    outside, ins = out_by > band, out_by < -band
    dist = np.linalg.norm(loc - clamp, axis=1)
    hit, miss = outside & (r - dist > band), outside & (r - dist < -band)
    fd = half - np.abs(loc)
    fs = np.sort(fd, axis=1)
    kk = np.argmin(fd, axis=1)
    tie = fs[:, 1] - fs[:, 0] <= 2 * band
    nsel = hit & (dist > 10 * band)
    _cap("sphere-box contact or none, inside or outside", place, ~(hit | miss | ins))
    _cap("sphere-box normal of an outside centre (dist > 10 band)", place, hit & ~nsel, of=hit)
    assert hit.sum() > n // 10 and miss.sum() > n // 20 and ins.sum() > n // 20
    w = orc32.world()
    gs = orc32.lib.orc_geom_create_sphere(w.w, 0.3)
    gb = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    rad = np.column_stack([r, np.zeros(n), np.zeros(n)])
    cnt, pos, nrm, dep = _bulk(orc32, w, gs, gb, _pose(ps, np.tile(np.eye(3), (n, 1, 1))), rad, _pose(pb, Rb), side, maxc=4)
    assert np.all(cnt[miss] == 0) and np.all(cnt[hit] == 1) and np.all(cnt[ins] == 1)
    q = pb + np.einsum("nij,nj->ni", Rb, clamp)
    _within("sphere-box position (centre outside)", place, (np.max(np.abs(pos[:, 0] - q), axis=1) / u)[hit], k)
    _within("sphere-box depth (centre outside)", place, (np.abs(dep[:, 0] - (r - dist)) / u)[hit], k)
    nn = (ps - q) / np.where(dist > 0, dist, 1.0)[:, None]
    _within("sphere-box normal (centre outside) x dist", place, (np.linalg.norm(nrm[:, 0] - nn, axis=1) * dist / u)[nsel], k)
    assert np.all(np.abs(np.linalg.norm(nrm[cnt > 0, 0], axis=1) - 1.0) <= 4 * EPS32)
    # centre inside: pushed out through the nearest face, depth = distance to it + r, contact at the centre
    a = np.arange(n)
    _within("sphere-box depth (centre inside)", place, (np.abs(dep[:, 0] - (fd[a, kk] + r)) / u)[ins], k)
    axis = Rb[a, :, kk] * np.sign(loc[a, kk])[:, None]
    sel = ins & ~tie & (np.abs(loc[a, kk]) > band)
    _cap("sphere-box nearest face tied", place, ins & ~sel, of=ins)
    _within("sphere-box normal (centre inside)", place, (np.linalg.norm(nrm[:, 0] - axis, axis=1) * np.minimum(r, side.min(axis=1)) / u)[sel], k)
    assert np.allclose(pos[ins, 0], ps[ins], atol=0)


# ------------------------------------------------------------------------------------------------------------ box - plane
@pytest.mark.parametrize("place", PLACES)
def test_f32_box_plane(orc32, place):
    """As the float64 test, the centres' heights drawn from (0.3 .. 1.8) x the reach instead of (0.3 .. 1.2): at FAR the band
    (k = 8) is 4 mm, and the float64 draw leaves 5.8 % of the boxes with a corner that close.  A corner within the band of the plane may
    count or not (that box is left out of the count rules), and
    the four-or-three rule is checked where the fourth and fifth lowest corners are more than two bands apart."""
    k = K_BAND["box_plane"]
    p, R, side = _draw_box_plane(lift_hi=1.8)
    n = len(p)
    s = _shift(place)
    p, R, side = _r32(p + s, R, side)
    normal = np.array([0.0, 1.0, 0.0])                                       # FAR has no y component: the plane stays y = 0
    assert float(normal @ s) == 0.0
    V = _box_vertices(p, R, side)
    Vrel = V - p[:, None, :]
    vd = -V[:, :, 1]
    deepest = vd.max(axis=1)
    u = EPS32 * (np.max(np.abs(p), axis=1) + 0.5 * np.linalg.norm(side, axis=1))
    band = k * u
    clear = np.all(np.abs(vd) > band[:, None], axis=1)
    vs = -np.sort(-vd, axis=1)
    apart = vs[:, 3] - vs[:, 4] > 2 * band
    _cap("box-plane a corner within the band of the plane", place, ~clear)
    _cap("box-plane fourth and fifth corner within two bands", place, ~apart)
    w = orc32.world()
    pl = orc32.lib.orc_geom_create_plane(w.w, 0.0, 1.0, 0.0, 0.0)
    b = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc32, w, b, pl, _pose(p, R), side, _pose(np.zeros((n, 3)), np.tile(np.eye(3), (n, 1, 1))), None, maxc=4)
    assert np.all(cnt[deepest < -band] == 0) and np.all(cnt[deepest > band] >= 1)
    hit = np.flatnonzero(deepest > band)
    assert len(hit) > n // 4 and cnt.max() <= 4
    m = np.arange(4)[None, :] < cnt[hit, None]
    dist = np.max(np.abs(pos[hit][:, :, None, :] - V[hit][:, None, :, :]), axis=3)
    which = dist.argmin(axis=2)
    uh = u[hit, None] * np.ones((1, 4))
    _within("box-plane position (a corner)", place, (dist.min(axis=2) / uh)[m], k)
    _within("box-plane depth (that corner's)", place, (np.abs(dep[hit] - np.take_along_axis(vd[hit], which, axis=1)) / uh)[m], k)
    _within("box-plane first depth (the deepest)", place, np.abs(dep[hit, 0] - deepest[hit]) / u[hit], k)
    assert np.all(dep[hit][m] >= -band[hit, None].repeat(4, 1)[m])
    srt = np.sort(np.where(m, which, 100 + np.arange(4)[None, :]), axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])
    assert np.allclose(nrm[hit][m], normal[None, :], atol=0)
    below = (vd > 0).sum(axis=1)
    assert np.all(cnt[clear] <= np.minimum(4, below[clear])) and np.all(cnt[clear] >= np.minimum(3, below[clear]))
    four = clear & apart & (below >= 4)
    low4 = np.argsort(-vd, axis=1)[:, :4]
    c4 = np.take_along_axis(Vrel, low4[:, :, None], axis=1)
    planar = np.abs(np.linalg.det(c4[:, 1:] - c4[:, :1])) < 1e-12          # the four lowest corners lie in one plane: a face
    assert np.all(cnt[four & planar] == 4) and np.all(cnt[four & ~planar] == 3)
    assert (four & planar).sum() > 1000 and (below[clear] == 3).sum() > 1000


# ------------------------------------------------------------------------------------------------------------ box - box
def _edge_sines(R1, R2):
    """(n, 15): 1 for the six face axes, |u_i x v_j| for the nine edge pairs -- the denominators of the edge axes' normalisation"""
    ln = np.ones((len(R1), 15))
    for i in range(3):
        for j in range(3):
            ln[:, 6 + 3 * i + j] = np.linalg.norm(np.cross(R1[:, :, i], R2[:, :, j]), axis=1)
    return ln


def _possible_choices(ov, ok, band_a):
    """(n, 15) bool: axis a can be dBoxBox's choice when every overlap may move by its band -- the selection rule of the float64
    test, run once per axis with that axis' overlap lowered by its band and every other one raised"""
    n = len(ov)
    out = np.zeros((n, 15), bool)
    for a in range(15):
        o = ov + band_a
        o[:, a] = ov[:, a] - band_a[:, a]
        s = -o[:, 0].copy(); pick = np.zeros(n, int)
        for f in range(1, 6):
            better = -o[:, f] > s
            s[better] = -o[better, f]; pick[better] = f
        for e in range(6, 15):
            cand = -o[:, e]
            use = ok[:, e] & (cand * 1.05 > s)
            s[use] = cand[use]; pick[use] = e
        out[:, a] = pick == a
    return out


MIN_EDGE_SINE2 = 1e-2        # an edge case's point is compared where 1 - (u.v)^2 exceeds this: below, the closest approach of two nearly
                             # parallel lines is ill-conditioned by construction (its band is divided by that denominator)


@pytest.mark.parametrize("place", PLACES)
def test_f32_box_box_against_the_separating_axis_theorem(orc32, place):
    """Judged by OUTCOME, not by the index of the axis: with near-parallel boxes the two boxes' faces are one axis to within rounding and
    ties by index are the rule.  The reported (normal, depth) must be those of SOME axis that the selection rule can choose when every
    overlap moves by its band; an edge axis u x v / |u x v| has the pair's own size over |u x v| added to its band."""
    k = K_BAND["box_box"]
    p1, R1, s1, p2, R2, s2 = _draw_box_box()
    n = len(p1)
    s = _shift(place)
    p1, R1, s1, p2, R2, s2 = _r32(p1 + s, R1, s1, p2 + s, R2, s2)
    ov, axes, ok = _sat_by_projection(p1, R1, s1, p2, R2, s2)
    ln = _edge_sines(R1, R2)
    u = EPS32 * (_reach(p1, p2) + 0.5 * np.linalg.norm(s1, axis=1) + 0.5 * np.linalg.norm(s2, axis=1))
    band = k * u
    # per axis: a face axis' overlap carries the coordinates' rounding, eps32 M; an edge axis u x v / |u x v| adds the error of its
    # own direction, eps32 / |u x v|, times what it multiplies -- lengths of the pair's own size M_rel = |p2 - p1| + the two radii
    u_rel = EPS32 * (np.linalg.norm(p2 - p1, axis=1) + 0.5 * np.linalg.norm(s1, axis=1) + 0.5 * np.linalg.norm(s2, axis=1))
    ua = u[:, None] + np.where(np.arange(15)[None, :] >= 6, u_rel[:, None] / np.where(ok, ln, 1.0), 0.0)         # (n, 15)
    band_a = k * ua
    ext = np.minimum(s1.min(axis=1), s2.min(axis=1))

    # (1) contacts <=> no separating axis, outside the band
    clear_sep = np.any(ok & (ov < -band_a), axis=1)
    clear_hit = np.all(~ok | (ov > band_a), axis=1)
    _cap("box-box contact or none", place, ~clear_sep & ~clear_hit)
    assert clear_sep.sum() > n // 10 and clear_hit.sum() > n // 4
    w = orc32.world()
    g1 = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    g2 = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc32, w, g1, g2, _pose(p1, R1), s1, _pose(p2, R2), s2, maxc=8)
    assert np.all(cnt[clear_sep] == 0), "contacts reported across a separating axis"
    assert np.all(cnt[clear_hit] >= 1), "no contact although all 15 axes overlap"
    assert cnt.max() <= 8 and np.all(cnt >= 0)
    hit = np.flatnonzero(clear_hit)
    nh = len(hit)

    # (2), (3) the normal is one of the axes the rule can choose, the depth that axis' overlap
    can = _possible_choices(ov[hit], ok[hit], band_a[hit])
    n0 = nrm[hit, 0]
    sgn = np.where(np.einsum("naj,nj->na", axes[hit], (p1 - p2)[hit]) >= 0, 1.0, -1.0)           # from box 2 into box 1
    ang = np.linalg.norm(n0[:, None, :] - sgn[:, :, None] * axes[hit], axis=2)                   # (nh, 15)
    score = np.where(can, ang * ext[hit, None] / ua[hit], np.inf)                              # in the normal's unit, per axis
    best = score.argmin(axis=1)
    ar = np.arange(nh)
    ties = can.sum(axis=1) > 1
    print(f"F32 {place} box-box: {100.0 * ties.mean():.1f} % of the hits have more than one possible axis")
    _within("box-box normal against the nearest possible axis", place, score[ar, best], k)
    assert np.all(np.abs(np.linalg.norm(n0, axis=1) - 1.0) <= 4 * EPS32)
    same = np.where(np.arange(8)[None, :, None] < cnt[hit, None, None], nrm[hit] - n0[:, None, :], 0.0)
    assert np.abs(same).max() == 0.0                      # every contact of a pair carries the one normal
    edge = best >= 6
    ud = ua[hit, best]
    want = ov[hit, best]
    first_depth = dep[hit, 0]
    valid = np.arange(8)[None, :] < cnt[hit, None]
    top_depth = np.max(np.where(valid, dep[hit], -np.inf), axis=1)
    assert np.all(cnt[hit][edge] == 1)
    _within("box-box edge-edge depth", place, (np.abs(first_depth - want) / ud)[edge], k)
    _within("box-box face: the deepest contact over the overlap", place, ((top_depth - want) / ud)[~edge], k)
    assert np.all(np.where(valid, dep[hit], 0.0) >= -band[hit, None])
    assert edge.sum() > 1000 and (~edge).sum() > 10000

    # (4) every contact of a FACE case lies in both boxes inflated by its pair's penetration + the band
    grow = want + band[hit]
    in1 = _in_box(pos[hit], p1[hit], R1[hit], s1[hit], grow)
    in2 = _in_box(pos[hit], p2[hit], R2[hit], s2[hit], grow)
    fm = valid & ~edge[:, None]
    assert np.all(in1[fm]) and np.all(in2[fm])

    # (5) an EDGE case's contact: the midpoint of the closest approach of the two edge lines, where 1 - (u.v)^2 > MIN_EDGE_SINE2 and
    # the choice of the two edges is firm (the normal is not within 1e-3 of perpendicular to another side of either box)
    es = np.flatnonzero(edge)
    ih = hit[es]
    ei, ej = (best[es] - 6) // 3, (best[es] - 6) % 3
    n12 = -(sgn[es, best[es]][:, None] * axes[ih, best[es]])     # from box 1 towards box 2, by the float64 axis
    pa = p1[ih].copy(); pb = p2[ih].copy()
    firm = np.ones(len(es), bool)
    for j in range(3):
        da = np.einsum("nj,nj->n", n12, R1[ih][:, :, j]); db = np.einsum("nj,nj->n", n12, R2[ih][:, :, j])
        firm &= ((np.abs(da) > 1e-3) | (ei == j)) & ((np.abs(db) > 1e-3) | (ej == j))
        pa += (np.where(da > 0, 1.0, -1.0) * 0.5 * s1[ih, j])[:, None] * R1[ih][:, :, j]
        pb += (np.where(db > 0, -1.0, 1.0) * 0.5 * s2[ih, j])[:, None] * R2[ih][:, :, j]
    ua_ = R1[ih, :, ei]; ub_ = R2[ih, :, ej]
    dp = pb - pa
    uaub = np.einsum("nj,nj->n", ua_, ub_); q1 = np.einsum("nj,nj->n", ua_, dp); q2 = -np.einsum("nj,nj->n", ub_, dp)
    den = 1 - uaub * uaub
    good = (den > MIN_EDGE_SINE2) & firm
    _cap("box-box edge point: 1 - (u.v)^2 below the bound", place, den <= MIN_EDGE_SINE2)
    _cap("box-box edge point: the choice of edges not firm", place, ~firm)
    alpha = (q1 + uaub * q2) / np.where(good, den, 1.0); beta = (uaub * q1 + q2) / np.where(good, den, 1.0)
    mid = 0.5 * ((pa + alpha[:, None] * ua_) + (pb + beta[:, None] * ub_))
    assert good.sum() > 1000
    # dBoxBox builds the two edge points in WORLD coordinates and only then solves for the closest approach, so the coordinates'
    # rounding, eps32 M, is what 1 / (1 - (u.v)^2) amplifies -- not the pair's own size: a trait of the construction
    _within("box-box edge point x (1 - (u.v)^2)", place, (np.max(np.abs(pos[ih, 0] - mid), axis=1) * den / u[ih])[good], k)


@pytest.mark.parametrize("place", PLACES)
def test_f32_box_flat_on_a_larger_face(orc32, place):
    """As the float64 test (at FAR a 100 m box gives M = 4 200 and a band of 1 mm: 2 % of the sinks, U(1e-6, 0.05), lie inside it).
    The two boxes' y axes are one axis to within rounding, so either box may be the reference box: the four contacts are
    box 1's bottom corners, or those corners lifted onto box 2's top face."""
    k = K_BAND["box_on_face"]
    p1, R1, s1, p2, R2, s2, _ = _draw_flat_on_a_face()
    n = len(p1)
    s = _shift(place)
    p1, R1, s1, p2, R2, s2 = _r32(p1 + s, R1, s1, p2 + s, R2, s2)
    corners = _box_vertices(p1, R1, s1)
    loc = np.einsum("nji,nkj->nki", R2, corners - p2[:, None, :])
    low = np.argsort(loc[:, :, 1], axis=1)[:, :4]
    c4 = np.take_along_axis(corners, low[:, :, None], axis=1)
    l4 = np.take_along_axis(loc, low[:, :, None], axis=1)
    sink = 0.5 * s2[:, None, 1] - l4[:, :, 1]                                 # (n, 4): each bottom corner's depth under box 2's top
    u = EPS32 * (_reach(p1, p2) + 0.5 * np.linalg.norm(s1, axis=1) + 0.5 * np.linalg.norm(s2, axis=1))
    band = k * u
    on_face = np.all((np.abs(l4[:, :, 0]) < 0.5 * s2[:, None, 0] - band[:, None]) & (np.abs(l4[:, :, 2]) < 0.5 * s2[:, None, 2] - band[:, None]), axis=1)
    firm = (sink.min(axis=1) > band) & on_face
    _cap("box flat on a face: a corner within the band of the face or of its rim", place, ~firm)
    w = orc32.world()
    g1 = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    g2 = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)
    cnt, pos, nrm, dep = _bulk(orc32, w, g1, g2, _pose(p1, R1), s1, _pose(p2, R2), s2)
    assert np.all(cnt[firm] == 4)
    up = R2[:, :, 1]
    ext = np.minimum(s1.min(axis=1), s2.min(axis=1))
    dn = np.minimum(np.linalg.norm(nrm[:, 0] - up, axis=1), np.linalg.norm(nrm[:, 0] - R1[:, :, 1], axis=1))
    _within("box flat on a face: normal", place, (dn * ext / u)[firm], k)
    lifted = c4 + sink[:, :, None] * up[:, None, :]
    d_low = np.max(np.abs(pos[:, :4, None, :] - c4[:, None, :, :]), axis=3)        # (n, contact, corner)
    d_up = np.max(np.abs(pos[:, :4, None, :] - lifted[:, None, :, :]), axis=3)
    # per pair: all four on box 1's corners, or all four on the lifted ones
    per_pair = np.minimum(d_low.min(axis=2).max(axis=1), d_up.min(axis=2).max(axis=1))
    _within("box flat on a face: positions (corners, or corners lifted onto the face)", place, (per_pair / u)[firm], k)
    which = np.where((d_low.min(axis=2).max(axis=1) <= d_up.min(axis=2).max(axis=1))[:, None], d_low.argmin(axis=2), d_up.argmin(axis=2))
    assert np.all(np.sort(which[firm], axis=1) == np.arange(4)[None, :])          # each corner once
    _within("box flat on a face: depths (each corner's)", place, (np.abs(dep[:, :4] - np.take_along_axis(sink, which, axis=1)) / u[:, None])[firm], k)


# ------------------------------------------------------------------------------------------------------------ hulls
def _match_points(cand, margin, band, pos, dep, cnt, u, maxc=8):
    """One pair of a "points inside a convex shape" collider.  cand (m, 3): the candidate points in the collider's order, margin (m,):
    each one's float64 margin (> 0 inside).  The reported contacts must be, in order, candidates with margin > -band; every candidate
    with margin > band must be there (up to the cap).  -> (worst position deviation, worst depth deviation) in units of u"""
    if cnt == 0:
        assert not np.any(margin > band), "no contact although a point is inside beyond the band"
        return 0.0, 0.0
    dist = np.max(np.abs(pos[:cnt, None, :] - cand[None, :, :]), axis=2)
    idx = dist.argmin(axis=1)
    assert np.all(np.diff(idx) > 0), "contacts out of order, or one point twice"
    assert np.all(margin[idx] > -band), "a point outside beyond the band was reported"
    must = np.flatnonzero(margin > band)
    if cnt == maxc:
        must = must[must < idx[-1]]
    assert np.all(np.isin(must, idx)), "a point inside beyond the band is missing"
    return float(dist[np.arange(cnt), idx].max() / u), float(np.abs(dep[:cnt] - margin[idx]).max() / u)


@pytest.mark.parametrize("place", PLACES)
def test_f32_hull_colliders(orc32, place):
    """As the float64 test, the decisions point by point: a vertex or corner whose margin is within the band may be a contact or not
    (at FAR the band is a millimetre and, with 28 to 40 candidate points a pair, many PAIRS have some point that close: the cap is on the
    share of POINTS)."""
    k = K_BAND["hulls"]
    verts, planes, side, Rh, Rb, ph, pb, Ra, pa, r, ps = _draw_hulls()
    n = len(ph)
    s = _shift(place)
    verts, planes, side, Rh, Rb, ph, pb, Ra, pa, r, ps = _r32(verts, planes, side, Rh, Rb, ph + s, pb + s, Ra, pa + s, r, ps + s)
    rh = float(np.linalg.norm(verts, axis=1).max())
    w = orc32.world()
    w.set_hull(verts)
    w.set_hull_faces(planes)
    gh = orc32.lib.orc_geom_create_convex(w.w)
    gb = orc32.lib.orc_geom_create_box(w.w, 1.0, 1.0, 1.0)

    def inside(pw, pc, Rc):
        l = np.einsum("nji,nkj->nki", Rc, pw - pc[:, None, :])
        return (planes[None, None, :, 3] - np.einsum("nki,fi->nkf", l, planes[:, :3])).min(axis=2)

    # box - hull: the hull's vertices inside the box, then the box's corners inside the hull
    u = EPS32 * (_reach(ph, pb) + rh + 0.5 * np.linalg.norm(side, axis=1))
    band = k * u
    VW = ph[:, None, :] + np.einsum("nij,kj->nki", Rh, verts)
    loc = np.einsum("nji,nkj->nki", Rb, VW - pb[:, None, :])
    margin = (0.5 * side[:, None, :] - np.abs(loc)).min(axis=2)
    corners = _box_vertices(pb, Rb, side)
    cm = inside(corners, ph, Rh)
    allm = np.concatenate([margin, cm], axis=1)
    _cap("box-hull points within the band", place, np.abs(allm) <= band[:, None])
    assert ((allm > band[:, None]).sum(axis=1) > 0).sum() > n // 20
    cnt, pos, nrm, dep = _bulk(orc32, w, gb, gh, _pose(pb, Rb), side, _pose(ph, Rh), None, maxc=8)
    cand = np.concatenate([VW, corners], axis=1)
    worst = np.zeros(2)
    for i in range(6000):
        worst = np.maximum(worst, _match_points(cand[i], allm[i], band[i], pos[i], dep[i], int(cnt[i]), u[i]))
        assert np.all(np.abs(np.linalg.norm(nrm[i, :cnt[i]], axis=1) - 1) <= 4 * EPS32)
    _within("box-hull position", place, worst[:1], k); _within("box-hull depth", place, worst[1:], k)
    sure = np.all(np.abs(allm) > band[:, None], axis=1)
    assert np.all(cnt[sure] == np.minimum(8, (allm > 0).sum(axis=1))[sure])

    # hull - hull: B's vertices inside A first, then A's inside B
    g2 = orc32.lib.orc_geom_create_convex(w.w)
    u = EPS32 * (_reach(ph, pa) + 2 * rh)
    band = k * u
    VA = pa[:, None, :] + np.einsum("nij,kj->nki", Ra, verts)
    allm = np.concatenate([inside(VW, pa, Ra), inside(VA, ph, Rh)], axis=1)
    _cap("hull-hull points within the band", place, np.abs(allm) <= band[:, None])
    cnt, pos, nrm, dep = _bulk(orc32, w, gh, g2, _pose(pa, Ra), None, _pose(ph, Rh), None, maxc=8)
    cand = np.concatenate([VW, VA], axis=1)
    worst = np.zeros(2)
    for i in range(6000):
        worst = np.maximum(worst, _match_points(cand[i], allm[i], band[i], pos[i], dep[i], int(cnt[i]), u[i]))
    _within("hull-hull position", place, worst[:1], k); _within("hull-hull depth", place, worst[1:], k)
    sure = np.all(np.abs(allm) > band[:, None], axis=1)
    assert np.all(cnt[sure] == np.minimum(8, (allm > 0).sum(axis=1))[sure]) and ((allm > band[:, None]).sum(axis=1) > 0).sum() > n // 20

    # sphere - hull: the face plane farthest out decides
    gs = orc32.lib.orc_geom_create_sphere(w.w, 0.3)
    z = np.zeros(n)
    u = EPS32 * (_reach(ph, ps) + rh + r)
    band = k * u
    c = np.einsum("nji,nj->ni", Rh, ps - ph)
    sd = c @ planes[:, :3].T - planes[None, :, 3]
    smax = sd.max(axis=1)
    hit = r - smax > band; miss = r - smax < -band
    _cap("sphere-hull contact or none", place, ~hit & ~miss)
    cnt, pos, nrm, dep = _bulk(orc32, w, gs, gh, _pose(ps, np.tile(np.eye(3), (n, 1, 1))), np.column_stack([r, z, z]), _pose(ph, Rh), None, maxc=2)
    assert np.all(cnt[hit] == 1) and np.all(cnt[miss] == 0) and hit.sum() > n // 10
    _within("sphere-hull depth", place, (np.abs(dep[:, 0] - (r - smax)) / u)[hit], k)
    # the normal: that of a face whose plane is within two bands of the farthest one (judged by outcome: at FAR the band is a
    # millimetre and a 36-face hull often has two faces that close)
    nwf = np.einsum("nij,fj->nfi", Rh, planes[:, :3])
    dn = np.where(sd >= (smax - 2 * band)[:, None], np.linalg.norm(nrm[:, 0, None, :] - nwf, axis=2), np.inf).min(axis=1)
    _within("sphere-hull normal", place, (dn * np.minimum(r, 2 * planes[:, 3].min()) / u)[hit], k)
