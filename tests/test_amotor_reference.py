"""tests/amotor_dense.py -- the float64 restatement the AMotor tests compare the product with -- held to closed forms.  CPU only; it
runs no code of the product.

  the Euler angles   side 1 at Rot(a_2, th_2) Rot(a_1, th_1) Rot(a_0, th_0) from a random zero pose returns (th_0, th_1, th_2), and each
                     angle grows when side 1 turns about +a_i against side 2
  the rows           J = [ 0, a_i | 0, -a_i ] in the sides as given, both blocks negated after an exchange of sides; one row per present
                     axis, in axis order, where the set's order puts the joint
  a motor            one body on an AMotor to the world, a motor on axis i: after one dWorldStep tick a_i . omega = vel when fmax
                     suffices, and h fmax / I otherwise (isotropic inertia I, no other torque)"""
import numpy as np
import pytest

import amotor_dense as am
import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm

H = 1.0 / 60.0


@pytest.mark.parametrize("sides", ["bb", "bw", "wb"])
def test_the_composition_returns_its_angles(sides):
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(700):
        th = am.random_angles(rng, mid=1.4, outer=3.0)
        B = ld.Bodies(rng.normal(size=(2, 3)), am.random_quats(rng, 2), np.zeros((2, 3)), np.zeros((2, 3)), [1.0, 1.0], np.ones((2, 3)))
        b1, b2 = {"bb": (0, 1), "bw": (0, -1), "wb": (-1, 0)}[sides]
        a0, a2 = am.perpendicular_pair(rng)
        m = am.from_world(B, b1, b2, am.EULER, (a0, a2))
        a = am.joint(b1, b2)
        assert np.max(np.abs(am.axes_angles(B, a, m)[1])) <= 1e-15          # the zero pose
        D = am.compose(a0, a2, th)
        # a rotation common to both sides changes nothing: turn everything by G afterwards
        G = am.random_quats(rng, 1)[0]
        for s, Ds in ((b1, D), (b2, np.array([1.0, 0, 0, 0]))) if b1 >= 0 else ((b2, lm.qconj(D)),):
            if s >= 0:
                q = ld.quat_mul(Ds, B.quat[s])
                if sides == "bb":
                    q = ld.quat_mul(G, q)
                B.quat[s] = q / np.linalg.norm(q)
        got = am.axes_angles(B, a, m)[1]
        worst = max(worst, float(np.max(np.abs(got - th))))
    print(f"{sides}: worst |theta - given| {worst:.2e}")
    assert worst <= 1e-13


def test_each_angle_grows_when_side_1_turns_about_its_axis():
    rng = np.random.default_rng(2)
    for _ in range(100):
        B, a, m = am.euler_pair(rng, am.random_angles(rng, mid=1.0, outer=2.0))
        A, th = am.axes_angles(B, a, m)
        for i in range(3):
            B2 = B.copy()
            q = ld.quat_mul(am.axis_angle_quat(A[i], 1e-6), B.quat[0])
            B2.quat[0] = q / np.linalg.norm(q)
            d = am.axes_angles(B2, a, m)[1] - th
            assert d[i] > 0
            if i == 1:
                assert abs(d[1] - 1e-6) <= 1e-10                     # the middle axis: exactly the angle's rate


def test_rows_are_as_defined_and_stand_in_the_set_s_order():
    rng = np.random.default_rng(3)
    B, a, m = am.euler_pair(rng, (0.3, -0.2, 0.5))
    m["fmax"][1], m["vel"][1] = 2.0, -1.0
    W = ld.World(h=H)
    for sides in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        th = am.axes_angles(B, am.joint(*sides), m)[1]
        lo0, hi2 = th[0] + 0.2, th[2] - 0.4                     # axis 0 below its low stop, axis 2 above its high stop
        m["lo_stop"][0], m["hi_stop"][2] = lo0, hi2
        art = np.array([jd.from_world(B, jd.BALL, 0, 1, (0, 0, 0)), am.joint(*sides), jd.from_world(B, jd.BALL, 1, -1, (1, 0, 0))], jd.ART_DTYPE)
        mot = am.motors(3)
        mot[1] = m
        members = jd.canonical_arts(B, art)
        I = am.Island(B, W, [0, 1], members, np.zeros(0, ld.JOINT_DTYPE), art, mot)
        assert I.m == 9 and I.amotor_rows == [3, 4, 5] and I.n_art_rows == 9
        A, th = am.axes_angles(B, art[1], mot[1])
        k = W.erp / W.h
        for i, q in enumerate(I.amotor_rows):
            want = np.zeros(12)
            for s, sign in ((sides[0], 1.0), (sides[1], -1.0)):
                if s >= 0:
                    want[6 * s + 3:6 * s + 6] = sign * A[i]
            assert np.array_equal(I.J[q], want)
        assert I.amotor_lines == [1, 3, 2]
        assert I.c[3] == -k * (th[0] - lo0) and (I.lo[3], I.hi[3]) == (0.0, np.inf)
        assert I.c[4] == -1.0 and (I.lo[4], I.hi[4]) == (-2.0, 2.0)
        assert I.c[5] == -k * (th[2] - hi2) and (I.lo[5], I.hi[5]) == (-np.inf, 0.0)
        # the ball rows around them are joint_dense's
        ref = jd.Island(B, W, [0, 1], [members[0], members[2]], np.zeros(0, ld.JOINT_DTYPE), art)
        assert np.array_equal(np.delete(I.J, [3, 4, 5], axis=0), ref.J.reshape(6, 12))
    # user mode: rel picks the frame, the supplied angle is theta; an AMotor without a present limot has no row and links the island
    mu = am.from_world(B, 0, 1, am.USER, [rng.normal(size=3) for _ in range(3)], rel=(0, 1, 2))
    mu["angle"] = (0.1, 0.2, 0.3)
    A, th = am.axes_angles(B, am.joint(0, 1), mu)
    R1, R2 = ld.quat_to_R(B.quat[0]), ld.quat_to_R(B.quat[1])
    assert np.array_equal(A[0], mu["axis"][0]) and np.array_equal(A[1], R1 @ mu["axis"][1]) and np.array_equal(A[2], R2 @ mu["axis"][2])
    assert np.array_equal(th, (0.1, 0.2, 0.3))
    art = np.array([am.joint(0, 1)], jd.ART_DTYPE)
    r = am.step(B, W, np.zeros(0, ld.JOINT_DTYPE), art, np.array([mu], am.AMOTOR_DTYPE), "exact")
    assert len(r.islands) == 1 and r.islands[0].m == 0 and list(r.islands[0].slots) == [0, 1]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("swapped", [False, True])
def test_a_motor_reaches_its_speed_or_saturates(axis, swapped):
    rng = np.random.default_rng(4 + axis)
    inertia, vel = 0.7, 1.3
    B = ld.Bodies([[0.0, 1.0, 0.0]], am.random_quats(rng, 1), [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [1.0], [[inertia] * 3])
    sides = (-1, 0) if swapped else (0, -1)
    W = ld.World(h=H, cfm=0.0)
    for fmax, want in ((inertia * vel / H * 1.5, vel), (0.25 * inertia * vel / H, H * 0.25 * inertia * vel / H / inertia)):
        m = am.from_world(B, sides[0], sides[1], am.USER, [rng.normal(size=3) for _ in range(3)], rel=(0, 1, 2))
        m["vel"][axis], m["fmax"][axis] = vel, fmax
        art, mot = np.array([am.joint(*sides)], jd.ART_DTYPE), np.array([m], am.AMOTOR_DTYPE)
        r = am.step(B, W, np.zeros(0, ld.JOINT_DTYPE), art, mot, "exact")
        a = am.axes_angles(B, art[0], mot[0])[0][axis]
        # the rate is that of side 1 against side 2: given as (world, body) the body turns the other way
        got = a @ (np.zeros(3) - r.bodies.avel[0] if swapped else r.bodies.avel[0])
        assert abs(got - want) <= 1e-12, (got, want)
