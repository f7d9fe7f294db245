"""The per-body flags (DMX_BODY_ALIVE / KINEMATIC / NOGRAVITY / NOGYRO) as the dense float64 reference (tests/lcp_dense.py)
understands them, checked on the CPU before the device is held to that reference (tests/test_gpu_body_flags.py).

Closed forms for one tick say what each flag means without the reference's own branches: a kinematic body keeps its
velocities bit for bit and moves with them; NOGRAVITY is a world without gravity for that body; NOGYRO is GYRO_OFF for that
body; a slot that is not alive does not move, and a joint that names it treats it as static (the header's contract at
dmxBatchStepJoints: only a joint whose two ends are both static is dropped), so a chain with a dead middle link is two
islands; joints between bodies of infinite mass move nobody.

Kinematic is also checked as a limit that does not go through `if flags & KINEMATIC` at all: a dynamic body of mass and
inertia 10^k in its place.  The solution of the box LCP is a piecewise linear, hence Lipschitz, function of (A, b), and the
heavy body enters A and b only through 1 / mass = 10^-k (and its own velocity change, also O(10^-k)), so the stacks'
velocities differ from the kinematic answer by C 10^-k: the error falls monotonically over k = 4, 6, 8 and by 10^4 between
k = 4 and k = 8; the assertion asks for 10^3."""
import numpy as np
import pytest

import lcp_dense as ld

STEPPERS = ["quick", "exact"]
GYROS = [ld.GYRO_EXPLICIT, ld.GYRO_IMPLICIT]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _chain(nb, n_contacts, mu, rng, speed=0.3, mass=(0.5, 2.0)):
    """the chain of tests/test_gpu_solver_dense.py (same draws in the same order, so the same scene for the same seed): slot k
    rests on k - 1, slot 0 on static ground, n_contacts contacts round-robin over the links, anisotropic inertia"""
    pos = np.column_stack([rng.uniform(-0.05, 0.05, nb), 0.5 + np.arange(nb), rng.uniform(-0.05, 0.05, nb)])
    quat = np.array([_unit(rng.normal(size=4)) for _ in range(nb)])
    B = ld.Bodies(pos, quat, rng.normal(scale=speed, size=(nb, 3)), rng.normal(scale=speed, size=(nb, 3)),
                  rng.uniform(*mass, nb), rng.uniform(0.2, 1.0, (nb, 3)))
    links = [(0, -1)] + [(k, k - 1) for k in range(1, nb)]
    mus = np.broadcast_to(np.asarray(mu, np.float64), (n_contacts,))
    out = []
    for c in range(n_contacts):
        b1, b2 = links[c % len(links)]
        axis = B.pos[b1] - B.pos[b2] if b2 >= 0 else np.array([0.0, 1.0, 0.0])
        n = _unit(_unit(axis) + 0.4 * _unit(rng.normal(size=3)))
        p = B.pos[b1] + 0.6 * rng.uniform(0.2, 1.0) * _unit(rng.normal(size=3))
        out.append((p, n, rng.uniform(0, 0.05), b1, b2, ld.CONTACT_BOUNCE, mus[c], 0.2, 0.1, 0.0, 0.0))
    return B, np.array(out, ld.JOINT_DTYPE)


def _world(**kw):
    return ld.World(cfm=1e-5, **kw)


def _state(b):
    return np.column_stack([b.pos, b.quat, b.lvel, b.avel])


def _quat_step(q, w, h):
    """the integrator written out: q + h/2 (0, w) (x) q, normalised"""
    qw, qv = q[0], q[1:]
    d = 0.5 * h * np.concatenate([[-(w @ qv)], qw * w + np.cross(w, qv)])
    out = q + d
    return out / np.linalg.norm(out)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("gyro", GYROS)
def test_kinematic_body_keeps_its_velocity_and_moves_with_it(stepper, gyro):
    """a kinematic link in the middle of a pressed chain, gravity on, anisotropic inertia, a gyro mode on"""
    B, jts = _chain(3, 9, 0.4, np.random.default_rng(3))
    B.lvel[:, 1] -= 1.0
    B.flags[1] |= ld.KINEMATIC
    W = _world(gyro=gyro)
    r = ld.step(B, W, jts, stepper)
    (I,) = r.islands
    assert I.slots == [0, 1, 2] and np.any(I.J[:, 6:12] != 0)                 # it has rows, and they load its neighbours
    assert np.any(np.concatenate(r.lams) != 0)
    assert np.array_equal(r.bodies.lvel[1], B.lvel[1]) and np.array_equal(r.bodies.avel[1], B.avel[1])
    assert np.array_equal(r.bodies.pos[1], B.pos[1] + W.h * B.lvel[1])
    assert np.max(np.abs(r.bodies.quat[1] - _quat_step(B.quat[1], B.avel[1], W.h))) <= 4e-16
    # ... and it is there: without it the bodies around it end elsewhere
    free = B.copy(); free.flags[1] = ld.ALIVE
    assert not np.allclose(ld.step(free, W, jts, stepper).bodies.lvel[[0, 2]], r.bodies.lvel[[0, 2]], atol=1e-6)


def _one_body(seed, nc=4):
    B, jts = _chain(1, nc, 0.5, np.random.default_rng(seed), speed=1.0)
    B.lvel[0, 1] = -1.0
    return B, jts


@pytest.mark.parametrize("stepper", STEPPERS)
def test_nogravity_is_a_world_without_gravity(stepper):
    B, jts = _one_body(4)
    flagged = B.copy(); flagged.flags[0] |= ld.NOGRAVITY
    got = ld.step(flagged, _world(), jts, stepper).bodies
    assert np.array_equal(_state(got), _state(ld.step(B, _world(gravity=(0, 0, 0)), jts, stepper).bodies))
    assert not np.allclose(got.lvel, ld.step(B, _world(), jts, stepper).bodies.lvel, atol=1e-6)
    # and without contacts: the velocity does not change at all
    got = ld.step(flagged, _world(), jts[:0], stepper).bodies
    assert np.array_equal(got.lvel, B.lvel) and np.array_equal(got.avel, B.avel)


@pytest.mark.parametrize("stepper", STEPPERS)
@pytest.mark.parametrize("gyro", GYROS)
def test_nogyro_is_gyro_off(stepper, gyro):
    B, jts = _one_body(5)
    B.avel[0] = (3.0, -2.0, 1.0)
    flagged = B.copy(); flagged.flags[0] |= ld.NOGYRO
    got = ld.step(flagged, _world(gyro=gyro), jts, stepper).bodies
    assert np.array_equal(_state(got), _state(ld.step(B, _world(gyro=ld.GYRO_OFF), jts, stepper).bodies))
    assert not np.allclose(got.avel, ld.step(B, _world(gyro=gyro), jts, stepper).bodies.avel, atol=1e-6)


@pytest.mark.parametrize("stepper", STEPPERS)
def test_dead_middle_link_makes_two_islands(stepper):
    """slot 2 of a five-link chain is dead: it does not move, the links below and above it are islands of their own, and the
    joints that named it act as joints to static ground (the same scene with -1 in its place)"""
    B, jts = _chain(5, 20, 0.4, np.random.default_rng(6))
    B.lvel[:, 1] -= 1.0
    B.flags[2] = 0
    extra = jts[:2].copy()
    extra["body1"], extra["body2"] = (2, -1), (-1, 2)                         # dead - static, static - dead: dropped
    jj = np.concatenate([jts, extra])
    r = ld.step(B, _world(), jj, stepper)
    assert [I.slots for I in r.islands] == [[0, 1], [3, 4]]
    assert np.array_equal(_state(r.bodies)[2], _state(B)[2])
    assert not set(np.concatenate([I.row_joint for I in r.islands])) & {20, 21}
    static = jts.copy()
    static["body1"] = np.where(jts["body1"] == 2, -1, jts["body1"])
    static["body2"] = np.where(jts["body2"] == 2, -1, jts["body2"])
    r2 = ld.step(B, _world(), static, stepper)
    assert np.array_equal(_state(r2.bodies), _state(r.bodies))
    assert sum(I.m for I in r.islands) == sum(I.m for I in r2.islands) == 60
    # ... which is not what the chain does with the link alive
    alive = B.copy(); alive.flags[2] = ld.ALIVE
    assert [I.slots for I in ld.step(alive, _world(), jj, stepper).islands] == [[0, 1, 2, 3, 4]]


@pytest.mark.parametrize("stepper", STEPPERS)
def test_joints_between_immovable_bodies_move_nobody(stepper):
    """contacts between two kinematic bodies, and between a kinematic body and static ground (either way round), added to a
    scene: every body ends where it ends without them, and the kinematic ones keep their velocities"""
    B, jts = _chain(4, 12, 0.4, np.random.default_rng(7))
    B.lvel[:, 1] -= 1.0
    B.flags[0] |= ld.KINEMATIC
    B.flags[1] |= ld.KINEMATIC
    keep = ~((jts["body1"] == 1) & (jts["body2"] == 0)) & ~((jts["body1"] == 0) & (jts["body2"] == -1))
    assert 0 < keep.sum() < len(jts)
    with_them, without = ld.step(B, _world(), jts, stepper), ld.step(B, _world(), jts[keep], stepper)
    # (their rows have zero off-diagonal entries in A: only the length of the reference's dense dot products changes, rounding)
    assert np.max(np.abs(_state(with_them.bodies) - _state(without.bodies))) <= 1e-13
    for s in (0, 1):
        assert np.array_equal(with_them.bodies.lvel[s], B.lvel[s]) and np.array_equal(with_them.bodies.avel[s], B.avel[s])
    # two kinematic bodies and nothing else: nobody's velocity changes
    two = ld.Bodies(B.pos[:2], B.quat[:2], B.lvel[:2], B.avel[:2], B.mass[:2], B.inertia[:2], B.flags[:2])
    r = ld.step(two, _world(), jts[~keep], stepper)
    assert np.array_equal(r.bodies.lvel, two.lvel) and np.array_equal(r.bodies.avel, two.avel)


# ---------------------------------------------------------------------------------------------------------------------
def two_stacks(slab_flags):
    """the scene of test_kinematic_body_shared_by_two_stacks (tests/test_gpu_solver_dense.py): slot 0 a slab that carries two
    stacks of three bodies, the stacks' lowest contacts remapped from static ground to the slab"""
    rng = np.random.default_rng(21)
    B1, j1 = _chain(3, 9, 0.4, rng)
    B2, j2 = _chain(3, 9, 0.4, rng)
    pos = np.vstack([[[0, -0.5, 0]], B1.pos + (-2, 0, 0), B2.pos + (2, 0, 0)])
    quat = np.vstack([[[1, 0, 0, 0]], B1.quat, B2.quat])
    lv = np.vstack([[[0.1, 0.2, 0]], B1.lvel, B2.lvel]); av = np.vstack([[[0, 0.3, 0]], B1.avel, B2.avel])
    flags = np.full(7, ld.ALIVE, np.uint8); flags[0] |= slab_flags
    B = ld.Bodies(pos, quat, lv, av, np.concatenate([[5.0], B1.mass, B2.mass]), np.vstack([[[1, 1, 1]], B1.inertia, B2.inertia]), flags)
    jj = np.concatenate([j1, j2])
    jj["body1"][:9] += 1; jj["body2"][:9] = np.where(j1["body2"] >= 0, j1["body2"] + 1, 0)
    jj["body1"][9:] += 4; jj["body2"][9:] = np.where(j2["body2"] >= 0, j2["body2"] + 4, 0)
    jj["pos"][:9] += (-2, 0, 0); jj["pos"][9:] += (2, 0, 0)
    return B, jj


@pytest.mark.parametrize("stepper", STEPPERS)
def test_kinematic_is_the_limit_of_a_heavy_body(stepper):
    Bk, jj = two_stacks(ld.KINEMATIC | ld.NOGRAVITY)
    W = _world()
    ref = ld.step(Bk, W, jj, stepper).bodies
    errs = []
    for k in (4, 6, 8):
        B, _ = two_stacks(ld.NOGRAVITY)
        B.mass[0] = 10.0 ** k
        B.inertia[0] = 10.0 ** k
        got = ld.step(B, W, jj, stepper).bodies
        errs.append(max(np.max(np.abs(got.lvel[1:] - ref.lvel[1:])), np.max(np.abs(got.avel[1:] - ref.avel[1:]))))
    print("heavy-body error at k = 4, 6, 8:", errs)
    assert errs[0] > errs[1] > errs[2]
    assert errs[2] <= 1e-3 * errs[0]
    assert errs[0] <= 1e-2                                                    # C 1e-4 with C the size of the contact forces
