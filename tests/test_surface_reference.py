"""The extended contact surface (mu2, fdir1, motion, slip; dmxBatchStepJointsSurface): known answers on the dense float64 reference
itself (tests/surface_dense.py).  CPU only.  Contacts sit at the body's centre, so no torque arises; the world's CFM is 1e-10."""
import numpy as np
import pytest

import friction_dense as fd
import lcp_dense as ld
import surface_dense as sd

H = 1.0 / 60.0
G = 9.8
CFM = 1e-10
X = (1.0, 0.0, 0.0)


def _body(mass=2.0, lvel=(0.0, 0.0, 0.0)):
    return ld.Bodies([[0.0, 0.5, 0.0]], [[1.0, 0.0, 0.0, 0.0]], [lvel], [[0.0, 0.0, 0.0]], [mass], [[1.0, 1.0, 1.0]])


def _contact(world_first, **fields):
    """one contact at the body's centre with the world under it, given as (body, world) or as (world, body): the normal points
    into the first side"""
    if world_first:
        return ld.joints(1, pos=(0.0, 0.5, 0.0), normal=(0.0, -1.0, 0.0), body1=-1, body2=0, **fields)
    return ld.joints(1, pos=(0.0, 0.5, 0.0), normal=(0.0, 1.0, 0.0), body1=0, body2=-1, **fields)


@pytest.mark.parametrize("world_first", [False, True])
@pytest.mark.parametrize("u", [0.7, -1.3])
def test_belt_carries_the_body_at_its_speed_whichever_side_comes_first(world_first, u):
    W = ld.World(h=H, gravity=(0.0, -G, 0.0), cfm=CFM)
    jts = _contact(world_first, mode=sd.FDIR1 | sd.MOTION1, mu=np.inf)
    srf = sd.surfaces(1, fdir1=X, motion1=u)
    r = sd.step(_body(), W, jts, srf, "exact")
    v = r.bodies.lvel[0]
    # (1 / m + cfm / h) lambda = u / h: v = u / (1 + cfm m / h), 1.2e-8 below u
    assert abs(v[0] - u) <= 1e-7 * abs(u)
    assert abs(v[1]) <= 1e-7 * G * H and abs(v[2]) <= 1e-7 * G * H


@pytest.mark.parametrize("k", [0.01, 0.5])
def test_slip_slides_at_slip_times_the_friction_force(k):
    m, F = 2.0, 3.0
    W = ld.World(h=H, gravity=(F / m, -G, 0.0), cfm=CFM)          # the tangential force, as gravity's x component
    jts = _contact(False, mode=sd.FDIR1 | sd.SLIP1, mu=np.inf)
    srf = sd.surfaces(1, fdir1=X, slip1=k)
    r = sd.step(_body(mass=m), W, jts, srf, "exact")
    # v = h (F + lambda) / m and v = -k lambda (A lambda = b: (1 / m + k / h) lambda = -F / m): v = k F / (1 + k m / h)
    want = k * F / (1.0 + k * m / H)
    assert abs(r.bodies.lvel[0, 0] - want) <= 1e-9 * want
    assert abs(r.bodies.lvel[0, 2]) <= 1e-9 * G * H


@pytest.mark.parametrize("stepper", ["exact", "quick"])
def test_mu2_zero_is_the_island_with_that_row_deleted(stepper):
    W = ld.World(h=H, gravity=(1.0, -G, 2.0), cfm=CFM)
    B = _body(lvel=(0.4, -0.2, 0.6))
    jts = _contact(False, mode=sd.MU2, mu=0.5)
    srf = sd.surfaces(1, mu2=0.0)
    a = sd.step(B, W, jts, srf, stepper)
    assert a.islands[0].m == 3 and a.islands[0].lo[2] == 0.0 and a.islands[0].hi[2] == 0.0
    b = sd.step(B, W, jts, srf, stepper, drop_rows=lambda I: I.row_kind == 2)
    assert b.islands[0].m == 2
    # (the deleted row's multiplier was 0 at every visit, so the other rows' updates are the same numbers)
    tol = 1e-12 * ld.velocity_scale(b.bodies, W)
    assert np.max(np.abs(a.bodies.lvel - b.bodies.lvel)) <= tol and np.max(np.abs(a.bodies.avel - b.bodies.avel)) <= tol
    assert a.lams[0][2] == 0.0


@pytest.mark.parametrize("stepper", ["exact", "quick"])
@pytest.mark.parametrize("mode", [0, fd.APPROX1])
def test_fdir1_equal_to_plane_space_reproduces_the_friction_reference_exactly(stepper, mode):
    rng = np.random.default_rng(5)
    B = ld.Bodies([[0.0, 0.5, 0.0], [0.1, 1.5, 0.0]], [[1.0, 0.0, 0.0, 0.0]] * 2, rng.normal(size=(2, 3)), rng.normal(size=(2, 3)),
                  [1.0, 2.0], [[0.3, 0.4, 0.5]] * 2)
    W = ld.World(h=H, gravity=(0.0, -G, 0.0), cfm=CFM)
    jts = ld.joints(3, mode=mode, mu=0.5)
    jts["body1"], jts["body2"] = [0, 1, -1], [-1, 0, 1]
    for k in range(3):
        n = np.array([0.1 * k, 1.0, -0.2 * k])
        jts["normal"][k] = (n / np.linalg.norm(n)) * (-1.0 if k == 2 else 1.0)
        jts["pos"][k] = (0.1 * k, 0.0 if k == 0 else 1.0, 0.05)
    want = fd.step(B, W, jts, stepper)
    srf = sd.surfaces(3)
    canon = {k: n for k, _, _, n in ld.canonical(B, jts)}
    for k in range(3):
        srf["fdir1"][k] = ld.plane_space(canon[k])[0]
    jts2 = jts.copy()
    jts2["mode"] |= sd.FDIR1
    got = sd.step(B, W, jts2, srf, stepper)
    for name in ("pos", "quat", "lvel", "avel"):
        assert np.array_equal(getattr(got.bodies, name), getattr(want.bodies, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(got.lams, want.lams))
