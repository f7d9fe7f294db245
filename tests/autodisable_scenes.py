"""The scenes of the auto-disable tests, shared by tests/test_autodisable_reference.py (the float64 reference alone, on the CPU)
and tests/test_gpu_autodisable.py (the device against that reference).  Test infrastructure, not a test file.

Every scene is built so that the reference keeps two conditions on every tick (autodisable_reference.margin_ok): no speed the
rule looks at within 10 % of its threshold, and no time_left within 0.25 h of zero without being zero (idle_time is an odd
multiple of h / 2).  The CPU test asserts them for every scene; the GPU test asserts them again on the ticks it compares."""
import numpy as np

import autodisable_reference as ar
import lcp_dense as ld

H = 1.0 / 60.0
A, K, AD, DIS = ld.ALIVE, ld.KINEMATIC, ar.AUTODISABLE, ar.DISABLED
IDENT = (1.0, 0.0, 0.0, 0.0)


class Scene:
    def __init__(self, B, W, params, ticks, joints=None, links=(), uploads=None, counters=None):
        self.B, self.W, self.params, self.ticks = B, W, params, ticks
        self.joints = joints or (lambda t: np.zeros(0, ld.JOINT_DTYPE))
        self.links = links                  # (b1, b2) of articulation joints (hinges at the bodies' midpoint, axis z)
        self.uploads = uploads or {}        # tick -> flags (whole array) uploaded before that tick
        self.counters = counters


def bodies(pos, lvel=None, avel=None, flags=None, mass=None):
    n = len(pos)
    z = np.zeros((n, 3))
    return ld.Bodies(pos, np.tile(IDENT, (n, 1)), z if lvel is None else lvel, z if avel is None else avel,
                     np.ones(n) if mass is None else mass, np.ones((n, 3)), flags)


def world(**kw):
    kw.setdefault("cfm", 1e-5)
    return ld.World(h=H, **kw)


# ---------------------------------------------------------------------------------------------------------------------
def free_bodies(n):
    """n slots without gravity or joints: constant velocities at 0.5 x and 2 x a threshold, linear and angular in turn; a
    kinematic body, a dead slot and a slot without the bit among them (when there is room)"""
    p = ar.Params(lin=0.04, ang=0.06, idle_steps=3, idle_time=4.5 * H)       # sleeps after max(3, ceil(4.5)) = 5 idle ticks
    rng = np.random.default_rng(n)
    lvel, avel = np.zeros((n, 3)), np.zeros((n, 3))
    flags = np.full(n, A | AD, np.uint8)
    for s in range(n):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        e = rng.normal(size=3); e /= np.linalg.norm(e)
        kind = s % 4                                            # 0: slow in both, 1: fast linear, 2: fast angular, 3: at rest
        lvel[s] = d * p.lin * (2.0 if kind == 1 else 0.5 if kind in (0, 2) else 0.0)
        avel[s] = e * p.ang * (2.0 if kind == 2 else 0.5 if kind in (0, 1) else 0.0)
    if n >= 8:
        flags[4] |= K            # slow, with the bit: never sleeps
        flags[5] = 0             # dead
        flags[6] = A             # slow, without the bit
        lvel[6], avel[6] = lvel[0], avel[0]
        lvel[4], avel[4] = lvel[0], avel[0]
    pos = np.column_stack([np.arange(n) * 3.0, np.zeros(n), np.zeros(n)])
    return Scene(bodies(pos, lvel, avel, flags), world(gravity=(0, 0, 0)), p, 7)


def apex(idle_steps):
    """a body thrown straight up at 0.9 m/s: its speed is under 0.5 m/s for six ticks around the apex (2 thr / (g h) = 6.1).
    idle_steps = 3: asleep in mid-air at the third of them; idle_steps = 10: never, the counters reset on leaving"""
    p = ar.Params(lin=0.5, ang=0.5, idle_steps=idle_steps, idle_time=0.0)
    return Scene(bodies([[0.0, 5.0, 0.0]], [[0.0, 0.9, 0.0]], flags=[A | AD]), world(), p, 12)


def stack_contacts(k, below, y):
    """four depth-0 contacts at the corners of unit box k's lower face (at height y), normal up into k"""
    out = []
    for dx, dz in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        out.append(((dx, y, dz), (0.0, 1.0, 0.0), 0.0, k, below, 0, 0.5, 0.0, 0.0, 0.0, 0.0))
    return out


def stack(height, x=0.0, first=0, speed=0.3, mu=0.5):
    """-> (pos, lvel, joints) of `height` unit boxes on static ground, arriving at `speed`, slots from `first`"""
    pos = [[x, 0.5 + k, 0.0] for k in range(height)]
    lvel = [[0.0, -speed, 0.0]] * height
    j = []
    for k in range(height):
        j += stack_contacts(first + k, first + k - 1 if k else -1, float(k))
    j = np.array(j, ld.JOINT_DTYPE)
    j["pos"][:, 0] += x
    j["mu"] = mu
    return np.array(pos), np.array(lvel), j


def settling(heights, stepper, params=None):
    """stacks of unit boxes with four depth-0 contacts per layer arriving at 0.3 m/s (mu = 0.5, cfm = 1e-5).  Under dWorldStep
    every stack is 7 times or more under the default thresholds from the first tick on (the reference's speeds: 1.5e-3 at the
    most) and asleep at the tenth.  Under QuickStep the single box is too (3.6e-5), while the three-stack's sweeps never
    converge: its boxes keep turning at 6e-3 to 1.1e-2 rad/s and moving at 4e-3 to 2.6e-2 m/s.  That straddles the default
    angular threshold, so the scene's is 0.004 there (every box of the stack 55 % or more above it: the stack stays awake)
    with the linear one at the default (7.8e-3 at the most for the lowest box, 1.2e-2 at the least for the others)"""
    pos, lvel, js, first = [], [], [], 0
    for i, hgt in enumerate(heights):
        p, v, j = stack(hgt, 4.0 * i, first)
        pos.append(p); lvel.append(v); js.append(j); first += hgt
    B = bodies(np.vstack(pos), np.vstack(lvel), flags=np.full(first, A | AD, np.uint8))
    j = np.concatenate(js)
    if params is None:
        params = ar.Params() if stepper == "exact" else ar.Params(ang=0.004)
    return Scene(B, world(), params, 13, joints=lambda t: j)


def waking(stepper):
    """slots 0..2: a three-stack; 3: a fast body that touches the top of it in tick 3 only; 4: a box on the ground next to it, no
    link; 5, 6: two sleeping bodies in mid-air joined by a hinge.  Ticks 0, 1: the stack and the box rest awake (under dWorldStep
    they are idle and count down; idle_steps is large, nothing sleeps by itself).  Before tick 2 an upload sets DISABLED on them
    by hand, which leaves the counters alone.  Tick 2: everything but 3 is left out.  Tick 3: the contact joint 3 - 2 wakes the
    whole stack, whose counters must stand where they stood; 4, 5 and 6 stay asleep.  Tick 4: the stack goes on awake"""
    p3, _, j3 = stack(3, 0.0, 0)
    p1, _, j1 = stack(1, 4.0, 4)
    pos = np.vstack([p3, [[0.0, 3.5, 0.0]], p1, [[8.0, 3.0, 0.0], [9.0, 3.0, 0.0]]])
    lvel = np.zeros((7, 3)); lvel[3] = (0.0, -1.0, 0.0)
    flags = np.full(7, A | AD, np.uint8); flags[5:] |= DIS
    hand = flags.copy(); hand[[0, 1, 2, 4]] |= DIS
    hit = np.array(stack_contacts(3, 2, 3.0), ld.JOINT_DTYPE)
    rest = np.concatenate([j3, j1])
    # thresholds of 0.002, placed by the reference's speeds: under dWorldStep the resting and the woken stack move at 1.2e-3 m/s or
    # less and do not turn; under QuickStep every box turns at 5e-3 rad/s or more, and the one linear speed under the threshold is
    # 1.65e-3 m/s (17 % below it)
    p = ar.Params(lin=0.002, ang=0.002, idle_steps=50, idle_time=0.0)
    return Scene(bodies(pos, lvel, flags=flags), world(), p, 5, joints=lambda t: np.concatenate([rest, hit]) if t == 3 else rest,
                 links=((5, 6),), uploads={2: hand})


SCENES = {
    "free-1": lambda st: free_bodies(1), "free-63": lambda st: free_bodies(63), "free-64": lambda st: free_bodies(64),
    "free-65": lambda st: free_bodies(65), "free-130": lambda st: free_bodies(130),
    "apex-sleeps": lambda st: apex(3), "apex-stays-awake": lambda st: apex(10),
    "settling": lambda st: settling((1, 3, 6) if st == "exact" else (1, 3), st),
    # a multi-body island that falls asleep under QuickStep too: thresholds of 0.2, far above the sweeps' residual motion
    "settling-loose": lambda st: settling((1, 3), st, ar.Params(lin=0.2, ang=0.2)),
    "waking": waking,
}


def run_reference(scene, stepper, on_tick=None):
    """the scene through the reference alone -> list of Ticks; asserts the margin conditions on every tick"""
    B, cnt = scene.B.copy(), scene.counters.copy() if scene.counters else ar.Counters(scene.B.n, scene.params)
    out = []
    for t in range(scene.ticks):
        if t in scene.uploads:
            B, cnt = apply_upload(B, cnt, scene.uploads[t], scene.params)
        tk = ar.step(B, scene.W, scene.joints(t), stepper, scene.params, cnt, scene.links)
        assert ar.margin_ok(tk, scene.params, scene.W.h), f"tick {t}: the scene does not keep the margin conditions"
        B, cnt = tk.bodies, tk.counters
        out.append(tk)
    return out


def apply_upload(B, cnt, flags, params):
    """dmxBatchUploadBodyFlags' counter rule: DISABLED set -> clear or AUTODISABLE clear -> set resets the slot's counters"""
    B, cnt = B.copy(), cnt.copy()
    new = np.asarray(flags, np.uint8)
    reset = (((B.flags & DIS) != 0) & ((new & DIS) == 0)) | (((B.flags & AD) == 0) & ((new & AD) != 0))
    cnt.steps[reset], cnt.time[reset] = params.idle_steps, params.idle_time
    B.flags = new.copy()
    return B, cnt
