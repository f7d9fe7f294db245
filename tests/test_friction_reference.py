"""Friction that scales with the normal force (DMX_CONTACT_APPROX1, ODE's dContactApprox1): known answers on the dense
float64 reference itself (tests/friction_dense.py).  CPU only."""
import numpy as np
import pytest

import friction_dense as fd
import lcp_dense as ld

H = 1.0 / 60.0
G = 9.8
MU = 0.5


def _tangential(mass, tan_theta, mu, mode, stepper="exact", **kw):
    theta = np.arctan(tan_theta)
    bodies, world, jts = fd.slope_scene(mass, theta, mu, mode, g=G, h=H, **kw)
    res = fd.step(bodies, world, jts, stepper)
    return res, theta


@pytest.mark.parametrize("mass", [1.0, 100.0])
def test_slope_below_the_friction_angle_holds(mass):
    res, _ = _tangential(mass, 0.3, MU, fd.APPROX1)
    v = res.bodies.lvel[0]
    assert abs(v[0]) <= 1e-9 * G * H and abs(v[2]) <= 1e-9 * G * H


@pytest.mark.parametrize("mass", [1.0, 100.0])
def test_slope_above_the_friction_angle_slides_at_the_coulomb_rate(mass):
    res, theta = _tangential(mass, 0.8, MU, fd.APPROX1)
    want = H * G * (np.sin(theta) - MU * np.cos(theta))
    assert abs(res.bodies.lvel[0, 0] - want) <= 1e-9 * G * H
    assert abs(res.bodies.lvel[0, 2]) <= 1e-9 * G * H


def test_slope_is_the_same_for_both_masses_with_the_bit_and_not_without():
    with_bit = [_tangential(m, 0.8, MU, fd.APPROX1)[0].bodies.lvel[0, 0] for m in (1.0, 100.0)]
    assert abs(with_bit[0] - with_bit[1]) <= 1e-9 * G * H
    without = [_tangential(m, 0.8, MU, 0)[0].bodies.lvel[0, 0] for m in (1.0, 100.0)]
    theta = np.arctan(0.8)
    # box friction: mu newtons whatever presses -- h (g sin theta - mu / m)
    for m, v in zip((1.0, 100.0), without):
        assert abs(v - H * (G * np.sin(theta) - MU / m)) <= 1e-9 * G * H
    assert abs(without[0] - without[1]) > 0.04 * G * H      # h mu (1 - 1 / 100) = 0.0505 g h


@pytest.mark.parametrize("stepper", ["exact", "quick"])
def test_unbounded_mu_with_the_bit_is_unbounded_mu_without_it(stepper):
    theta = np.arctan(0.8)
    out = []
    for mode in (fd.APPROX1, 0):
        bodies, world, jts = fd.slope_scene(3.0, theta, np.inf, mode, g=G, h=H, phi=0.4)
        res = fd.step(bodies, world, jts, stepper)
        assert not res.islands[0].pyramid.any()
        out.append((res.bodies.lvel.copy(), res.bodies.avel.copy(), res.lams[0].copy()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_zero_mu_with_the_bit_is_one_row():
    bodies, world, jts = fd.slope_scene(3.0, 0.3, 0.0, fd.APPROX1, g=G, h=H)
    res = fd.step(bodies, world, jts, "exact")
    assert res.islands[0].m == 1 and not res.islands[0].pyramid.any()
    jts["mu"] = -1.0
    assert fd.step(bodies, world, jts, "quick").islands[0].m == 1


@pytest.mark.parametrize("bit,first", [(fd.APPROX1_1, True), (fd.APPROX1_2, False)])
def test_a_bit_bounds_its_own_direction_only(bit, first):
    # downhill = (cos phi, 0, sin phi): direction 1 is -x, direction 2 is +z; both directions slide, the marked one against
    # mu N, the other against mu newtons
    mass, theta, phi = 100.0, np.arctan(2.0), 0.7
    bodies, world, jts = fd.slope_scene(mass, theta, MU, bit, g=G, h=H, phi=phi)
    res = fd.step(bodies, world, jts, "exact")
    I = res.islands[0]
    assert list(I.pyramid) == [False, first, not first]
    gx, gz = G * np.sin(theta) * np.cos(phi), G * np.sin(theta) * np.sin(phi)
    pyr, box = MU * G * np.cos(theta), MU / mass
    want_x = H * (gx - (pyr if first else box))
    want_z = H * (gz - (box if first else pyr))
    assert abs(res.bodies.lvel[0, 0] - want_x) <= 1e-9 * G * H
    assert abs(res.bodies.lvel[0, 2] - want_z) <= 1e-9 * G * H


def test_quickstep_converges_to_the_two_pass_solution_on_a_sliding_contact():
    theta = np.arctan(0.8)
    bodies, world, jts = fd.slope_scene(2.0, theta, MU, fd.APPROX1, g=G, h=H, phi=0.3)
    ex = fd.step(bodies, world, jts, "exact")
    world.iters, world.sor_w = 400, 1.0
    qs = fd.step(bodies, world, jts, "quick")
    assert np.max(np.abs(qs.bodies.lvel - ex.bodies.lvel)) <= 1e-6 * G * H
    assert np.max(np.abs(qs.lams[0] - ex.lams[0])) <= 1e-6 * np.max(np.abs(ex.lams[0]))


def test_margins_count_the_moving_bound():
    # sliding: the friction row sits ON its bound mu lambda_n, so the visited row's update overshoots it by a finite amount; holding:
    # the row is free, and the margin is its distance to mu lambda_n -- not to mu newtons
    mass = 100.0
    res, theta = _tangential(mass, 0.3, MU, fd.APPROX1, stepper="quick")
    need = mass * G * np.sin(theta)                    # the friction force that holds the box
    room = MU * mass * G * np.cos(theta) - need          # ... and how far that is from the pyramid's bound
    assert res.margins[0] <= room * (1 + 1e-6)
    assert res.margins[0] > 0.0
    ex, _ = _tangential(mass, 0.3, MU, fd.APPROX1)
    assert abs(ex.margins[0] - room) <= 1e-6 * room


def test_an_island_without_pyramid_rows_is_lcp_dense():
    rng = np.random.default_rng(5)
    bodies = ld.Bodies(rng.uniform(-1, 1, (2, 3)), [[1, 0, 0, 0]] * 2, rng.normal(size=(2, 3)), rng.normal(size=(2, 3)), [1.0, 2.0],
                       [[0.4, 0.5, 0.6]] * 2)
    world = ld.World(h=H)
    jts = ld.joints(3, normal=(0.0, 1.0, 0.0), depth=0.01, body1=0, body2=-1, mu=0.5, mode=fd.APPROX1_N)
    jts["pos"] = rng.uniform(-0.5, 0.5, (3, 3))
    jts["body2"][2] = 1
    for stepper in ("quick", "exact"):
        a, b = fd.step(bodies, world, jts, stepper), ld.step(bodies, world, jts, stepper)
        assert np.array_equal(a.bodies.lvel, b.bodies.lvel) and np.array_equal(a.bodies.avel, b.bodies.avel)
