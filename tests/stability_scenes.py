"""The scenes of the damping / angular speed cap / contact correction tests, shared by tests/test_stability_reference.py (the
float64 reference alone, on the CPU) and tests/test_gpu_stability.py (the device against that reference).  Test infrastructure,
not a test file.

One scene per place the knobs live in the device code.  Every scene carries
  * contact depths on both sides of the surface layer, push-outs erp (d - layer) / h on both sides of the maximum correcting
    velocity, and at least one contact whose bounce ends above that maximum;
  * spins on both sides of the maximum angular speed after the tick's velocity update;
  * per-slot tables that differ from slot to slot (some slots without damping, some without a cap);
  * four extra slots at the end: two free spinners on either side of the cap, a KINEMATIC body faster than every
    threshold and the cap, and a slow body below both damping thresholds with NOGRAVITY and a unit inertia -- both must keep their velocity bits.
The CPU test asserts all of that on the reference, and that the reference keeps stability_reference.margin_ok on every tick."""
import numpy as np

import autodisable_reference as ar
import joint_dense as jd
import lcp_dense as ld
import stability_reference as sr

H = 1.0 / 60.0
LAYER, VMAX = 0.02, 0.15            # erp / h = 12: depths up to 0.05 give push-outs up to 0.36 past the layer
MAX_SPIN = 0.5
# contact c's depth is DEPTHS[c % 4] +- 10 %: under the layer with a bounce of 0.3 (contact 0 meets the ground at ~1 m/s: past VMAX),
# a push-out of 0.06 under VMAX, one of 0.30 over it, and under the layer without a bounce (c = 0 exactly)
DEPTHS = (0.005, 0.025, 0.045, 0.01)
KIN_LVEL, KIN_AVEL = (0.7, 0.2, -0.4), (1.5, -0.8, 0.3)
SLOW_LVEL, SLOW_AVEL = (0.03, -0.02, 0.01), (0.02, 0.01, -0.03)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


class Scene:
    def __init__(self, B, jts, knobs, steppers, ticks=1, art=None, gravity=(0.0, -9.8, 0.0), grid=False):
        self.B, self.jts, self.knobs, self.steppers, self.ticks, self.art, self.grid = B, jts, knobs, steppers, ticks, art, grid
        self.W = ld.World(h=H, gravity=gravity, cfm=1e-5)
        self.kinematic, self.slow = B.n - 2, B.n - 1


def with_extras(B):
    """B with four free bodies appended, far from everything: a fast spinner (damped, ends on the cap), a gentle one (undamped,
    stays below the cap), the kinematic and the slow body"""
    flags = np.concatenate([B.flags, [ld.ALIVE, ld.ALIVE, ld.ALIVE | ld.KINEMATIC, ld.ALIVE | ld.NOGRAVITY]]).astype(np.uint8)
    ident = [[1, 0, 0, 0]] * 4
    return ld.Bodies(np.vstack([B.pos, [30.0, 5.0, 0.0], [40.0, 5.0, 0.0], [50.0, 5.0, 0.0], [60.0, 5.0, 0.0]]), np.vstack([B.quat, ident]),
                     np.vstack([B.lvel, (0.5, 0.1, 0.2), (0.1, 0.4, 0.3), KIN_LVEL, SLOW_LVEL]),
                     np.vstack([B.avel, (0.9, -0.7, 0.4), (0.1, 0.2, -0.2), KIN_AVEL, SLOW_AVEL]),
                     np.concatenate([B.mass, [1.0, 1.5, 1.0, 1.0]]), np.vstack([B.inertia, [0.5, 0.7, 0.9], [0.4, 0.4, 0.4], [1, 1, 1], [1, 1, 1]]), flags)


def knobs_for(n, rng):
    """damping 5 % / 10 % above 0.2 m/s and 0.2 rad/s and a cap of MAX_SPIN, varied per slot: every fourth slot undamped, every
    fifth uncapped, thresholds spread by +-20 %; of the four extra slots only the gentle spinner is undamped"""
    t = np.tile([0.05, 0.10, 0.2, 0.2, MAX_SPIN], (n, 1))
    t[:, 2:4] *= rng.uniform(0.8, 1.2, (n, 2))
    t[:, 4] *= rng.uniform(0.9, 1.1, n)
    t[0:n - 4:4, 0:2] = 0.0
    t[1:n - 4:5, 4] = np.inf
    t[n - 3, 0:2] = 0.0                 # the gentle spinner: undamped
    return sr.Knobs(n, t, LAYER, VMAX)


def chain(nb, n_contacts, mu, rng, speed=0.3):
    """nb bodies along y (slot k on k - 1, slot 0 on static ground), the contacts spread round-robin over the links: points within
    0.6 of body1's centre, normals within ~25 degrees of the link's axis, depths from DEPTHS, bounce 0.3 above 0.1 m/s on every
    fourth contact; every body moves down faster than the one below it"""
    pos = np.column_stack([rng.uniform(-0.05, 0.05, nb), 0.5 + np.arange(nb), rng.uniform(-0.05, 0.05, nb)])
    quat = np.array([_unit(rng.normal(size=4)) for _ in range(nb)])
    lvel = rng.normal(scale=speed, size=(nb, 3))
    lvel[:, 1] -= 1.0 + 0.1 * np.arange(nb)
    B = ld.Bodies(pos, quat, lvel, rng.normal(scale=speed, size=(nb, 3)), rng.uniform(0.5, 2.0, nb), rng.uniform(0.2, 1.0, (nb, 3)))
    links = [(0, -1)] + [(k, k - 1) for k in range(1, nb)]
    mus = np.broadcast_to(np.asarray(mu, np.float64), (n_contacts,))
    out = []
    for c in range(n_contacts):
        b1, b2 = links[c % len(links)]
        axis = B.pos[b1] - B.pos[b2] if b2 >= 0 else np.array([0.0, 1.0, 0.0])
        n = _unit(_unit(axis) + 0.4 * _unit(rng.normal(size=3)))
        p = B.pos[b1] + 0.6 * rng.uniform(0.2, 1.0) * _unit(rng.normal(size=3))
        out.append((p, n, DEPTHS[c % 4] * rng.uniform(0.9, 1.1), b1, b2, ld.CONTACT_BOUNCE if c % 4 == 0 else 0, mus[c], 0.3, 0.1, 0.0, 0.0))
    return B, np.array(out, ld.JOINT_DTYPE)


def press_chain(m, rng):
    """m rows of frictionless contacts, three per link of a chain of ceil(m / 3) bodies along y, each normal tilted 34 degrees from
    the chain's axis, the three of a link 120 degrees apart; every body moves down faster than the one below it and spins"""
    nb = -(-m // 3)
    pos = np.column_stack([np.zeros(nb), 0.5 + np.arange(nb), np.zeros(nb)])
    lv = np.zeros((nb, 3))
    lv[:, 1] = -(1.0 + 0.1 * np.arange(nb))
    B = ld.Bodies(pos, np.tile([1.0, 0, 0, 0], (nb, 1)), lv, rng.normal(scale=0.3, size=(nb, 3)), rng.uniform(0.8, 1.2, nb),
                  rng.uniform(0.3, 0.5, (nb, 3)))
    out = []
    for c in range(m):
        k = c // 3
        a = 2 * np.pi * (c % 3) / 3 + 0.3 * k
        d = np.array([np.cos(a), 0.0, np.sin(a)])
        n = np.array([0.0, np.cos(0.6), 0.0]) + d * np.sin(0.6)
        out.append((np.array([0.0, float(k), 0.0]) + 0.3 * d, n, DEPTHS[c % 4] * rng.uniform(0.9, 1.1), k, k - 1 if k else -1,
                    ld.CONTACT_BOUNCE if c % 4 == 0 else 0, 0.0, 0.3, 0.1, 0, 0))
    return B, np.array(out, ld.JOINT_DTYPE)


def _finish(B, jts, seed, steppers, **kw):
    B = with_extras(B)
    return Scene(B, jts, knobs_for(B.n, np.random.default_rng(seed + 7)), steppers, **kw)


def free():
    """six free bodies, islands without rows: speeds 0.25 .. 1.5 of MAX_SPIN, under gravity"""
    rng = np.random.default_rng(11)
    n = 6
    pos = np.column_stack([3.0 * np.arange(n), np.full(n, 4.0), np.zeros(n)])
    avel = np.array([_unit(rng.normal(size=3)) * MAX_SPIN * f for f in (0.25, 0.6, 1.3, 1.5, 0.8, 1.2)])
    B = ld.Bodies(pos, np.array([_unit(rng.normal(size=4)) for _ in range(n)]), rng.normal(scale=0.5, size=(n, 3)), avel, rng.uniform(0.5, 2.0, n),
                  rng.uniform(0.2, 1.0, (n, 3)))
    return _finish(B, np.zeros(0, ld.JOINT_DTYPE), 11, ("quick", "exact"), ticks=3)


def single(nc):
    """one body on static ground with nc contacts: the one-body forms (1..4 contacts in registers, 5..8 in LDS)"""
    B, jts = chain(1, nc, np.inf, np.random.default_rng(100 + nc))
    return _finish(B, jts, 100 + nc, ("quick", "exact"), ticks=2)


def stack2():
    """two boxes on the ground: the lane-per-island form"""
    B, jts = chain(2, 6, np.array([np.inf, 0.4, 0.0, np.inf, 0.4, 0.0]), np.random.default_rng(21))
    return _finish(B, jts, 21, ("quick", "exact"), ticks=2)


def quick_rows(m):
    """one QuickStep island of exactly m rows (README's row-form boundaries)"""
    B, jts = press_chain(m, np.random.default_rng(m))
    return _finish(B, jts, m, ("quick",))


def exact_rows(m, grid):
    """one dWorldStep island of m rows, mu = 0 / 0.4 / inf in turn"""
    rng = np.random.default_rng(m)
    mus, rows, k = [], 0, 0
    while rows < m:
        mu = (0.4, np.inf, 0.0)[k % 3]
        if rows + (3 if mu > 0 else 1) > m:
            mu = 0.0
        mus.append(mu)
        rows += 3 if mu > 0 else 1
        k += 1
    B, jts = chain(max(2, len(mus) // 3), len(mus), np.array(mus), rng)
    return _finish(B, jts, m, ("exact",), grid=grid)


def hinge_chain():
    """six links on hinges from the world, a ball in the middle, with errors to correct, swinging and spinning; no contacts"""
    B, art = jd.chain([jd.HINGE, jd.HINGE, jd.BALL, jd.HINGE, jd.HINGE, jd.HINGE], seed=5)
    jd.disturb(B, 5)
    B.avel *= 2.0
    return _finish(B, np.zeros(0, ld.JOINT_DTYPE), 5, ("quick", "exact"), ticks=2, art=art)


def sleepy_scene():
    """three stacks of two and six free bodies under auto-disable: stack 1 and two free bodies start asleep, every body may fall
    asleep; damping 30 % above 0.005 takes the slow free bodies from 0.018 to 0.0126 and 0.0088, past ODE's sleep thresholds of 0.01
    with more than 10 % to spare on either side, and they sleep three ticks later"""
    rng = np.random.default_rng(3)
    parts, jts = [], []
    for k in range(3):
        B, j = chain(2, 6, np.array([np.inf, 0.4, 0.0, np.inf, 0.4, 0.0]), np.random.default_rng(40 + k))
        B.pos[:, 0] += 5.0 * k
        j["pos"][:, 0] += 5.0 * k
        j["body1"] += 2 * k
        j["body2"] = np.where(j["body2"] >= 0, j["body2"] + 2 * k, -1)
        parts.append(B); jts.append(j)
    n_free = 6
    free = ld.Bodies(np.column_stack([20.0 + 3 * np.arange(n_free), np.full(n_free, 3.0), np.zeros(n_free)]), np.tile([1.0, 0, 0, 0], (n_free, 1)),
                     np.array([_unit(rng.normal(size=3)) * v for v in (0.018, 0.5, 0.018, 0.3, 0.018, 0.9)]),
                     np.array([_unit(rng.normal(size=3)) * v for v in (0.018, 0.4, 0.018, 0.1, 0.018, 0.7)]), np.ones(n_free), np.ones((n_free, 3)))
    parts.append(free)
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])
    flags = np.full(6 + n_free, ld.ALIVE | ar.AUTODISABLE, np.uint8)
    flags[6:] |= ld.NOGRAVITY
    flags[[2, 3, 7, 9]] |= ar.DISABLED
    B = ld.Bodies(cat("pos"), cat("quat"), cat("lvel"), cat("avel"), cat("mass"), cat("inertia"), flags)
    B = with_extras(B)
    k = sr.Knobs(B.n, None, LAYER, VMAX).set_damping(0.3, 0.3, 0.005, 0.005).set_max_angular_speed(0.5)
    s = Scene(B, np.concatenate(jts), k, ("quick", "exact"), ticks=6)
    return s, ar.Params(0.01, 0.01, 3, 0.0)


SCENES = {
    "free": free,
    "single-4": lambda: single(4),
    "single-8": lambda: single(8),
    "stack-2": stack2,
    "quick-256": lambda: quick_rows(256),
    "quick-260": lambda: quick_rows(260),
    "quick-1028": lambda: quick_rows(1028),
    "quick-3076": lambda: quick_rows(3076),
    "exact-lds-30": lambda: exact_rows(30, False),
    "exact-grid-300": lambda: exact_rows(300, True),
    "hinge-chain": hinge_chain,
}
SMALL_SCENES = ["free", "single-4", "single-8", "stack-2", "quick-256", "exact-lds-30", "hinge-chain"]      # the single-launch tick's
