"""Auto-disable restated in float64 on top of tests/lcp_dense.py, from the definition in include/dmx_batch.h ("auto-disable").

Test infrastructure, not a test file, and no code of the product: islands are lcp_dense's, an asleep island is left out by
stepping a copy in which its slots are not alive and its joints are gone, the awake rest is lcp_dense.step's, and the
end-of-tick rule is the four lines of the definition.

    idle = (lvel.lvel <= lin^2) && (avel.avel <= ang^2)
    if idle:  steps_left = max(steps_left - 1, 0);  time_left = max(time_left - h, 0)
    else:     steps_left = idle_steps;              time_left = idle_time
    if steps_left == 0 && time_left == 0:  set DISABLED;  lvel = avel = 0
"""
import numpy as np

import lcp_dense as ld

AUTODISABLE, DISABLED = 16, 32


class Params:
    """the batch's four values (defaults: ODE's)"""

    def __init__(self, lin=0.01, ang=0.01, idle_steps=10, idle_time=0.0):
        self.lin, self.ang, self.idle_steps, self.idle_time = float(lin), float(ang), int(idle_steps), float(idle_time)


class Counters:
    """per slot: steps_left (int32), time_left (float64)"""

    def __init__(self, n, params, steps=None, time=None):
        self.steps = np.full(n, params.idle_steps, np.int32) if steps is None else np.array(steps, np.int32)
        self.time = np.full(n, params.idle_time, np.float64) if time is None else np.array(time, np.float64)

    def copy(self):
        c = Counters.__new__(Counters)
        c.steps, c.time = self.steps.copy(), self.time.copy()
        return c


def idle_rule(lvel, avel, flags, steps, time, params, h):
    """the end-of-tick rule for one stepped slot -> (lvel, avel, flags, steps_left, time_left)"""
    if (flags & (ld.ALIVE | AUTODISABLE | ld.KINEMATIC | DISABLED)) != (ld.ALIVE | AUTODISABLE):
        return lvel, avel, flags, steps, time
    idle = (lvel @ lvel <= params.lin ** 2) and (avel @ avel <= params.ang ** 2)
    if idle:
        steps, time = max(int(steps) - 1, 0), max(float(time) - h, 0.0)
    else:
        steps, time = params.idle_steps, params.idle_time
    if steps == 0 and time == 0.0:
        return np.zeros(3), np.zeros(3), flags | DISABLED, steps, time
    return lvel, avel, flags, steps, time


def split_islands(bodies, jts, links=()):
    """-> (awake islands, asleep islands), each a list of (slots ascending, indices of jts).  `links`: (b1, b2) pairs of
    articulation joints that connect bodies beside the contact joints (b < 0: the world)"""
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    extra = ld.joints(len(links), body1=[l[0] for l in links], body2=[l[1] for l in links], normal=(0.0, 1.0, 0.0)) if len(links) else jts[:0]
    all_j = np.concatenate([jts, extra])
    awake, asleep = [], []
    for slots, cjs in ld.islands(bodies, ld.canonical(bodies, all_j)):
        idx = [k for k, *_ in cjs if k < len(jts)]
        (awake if any(not (bodies.flags[s] & DISABLED) for s in slots) else asleep).append((slots, idx))
    return awake, asleep


class Tick:
    """one tick's outcome: bodies (state and flags), counters, what was woken / skipped / put to sleep, the joints that made
    rows (mask over the input), and lcp_dense's Result of the awake part"""


def step(bodies, world, jts, stepper, params, counters, links=(), h_idle=None):
    """one dmxBatchStepJoints tick with auto-disable.  `bodies.flags` carries the AUTODISABLE / DISABLED bits; nothing passed
    in is changed.  An awake island with an articulation link cannot be stepped here (lcp_dense knows contacts only)."""
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    awake, asleep = split_islands(bodies, jts, links)
    awake_slots = sorted(s for slots, _ in awake for s in slots)
    asleep_slots = sorted(s for slots, _ in asleep for s in slots)
    for b1, b2 in links:
        live = [b for b in (b1, b2) if 0 <= b < bodies.n and bodies.flags[b] & ld.ALIVE]
        assert all(b in asleep_slots for b in live), "the reference steps no articulation joints"
    t = Tick()
    t.woken = [s for s in awake_slots if bodies.flags[s] & DISABLED]
    t.skipped_islands = len(asleep)
    t.asleep_before = asleep_slots
    t.stepped = awake_slots
    keep = np.zeros(len(jts), bool)
    for _, idx in awake:
        keep[idx] = True
    t.rows_from = keep
    work = bodies.copy()
    work.flags[t.woken] &= np.uint8(~DISABLED & 0xff)
    flags = work.flags.copy()
    work.flags[asleep_slots] &= np.uint8(~ld.ALIVE & 0xff)
    t.result = ld.step(work, world, jts[keep], stepper)
    out = t.result.bodies
    out.flags = flags
    t.pre_lvel, t.pre_avel = out.lvel.copy(), out.avel.copy()      # what the rule looks at
    cnt = counters.copy()
    h = world.h if h_idle is None else float(h_idle)
    t.slept = []
    for s in awake_slots:
        lv, av, f, st, tl = idle_rule(out.lvel[s], out.avel[s], int(flags[s]), cnt.steps[s], cnt.time[s], params, h)
        if (f & DISABLED) and not (flags[s] & DISABLED):
            t.slept.append(s)
        out.lvel[s], out.avel[s], out.flags[s], cnt.steps[s], cnt.time[s] = lv, av, f, st, tl
    t.bodies, t.counters = out, cnt
    t.contacts = int(keep.sum())
    return t


def margin_ok(tick, params, h):
    """the conditions that keep a comparison honest (never a tolerance): no stepped body that the rule looks at has a speed
    within 10 % of its threshold -- an exact zero is the same zero in every precision and is exempt -- and no time_left ends
    the tick within 0.25 h of zero without being zero.  Speeds are the rule's inputs: the post-step ones, before the zeroing."""
    for s in tick.stepped:
        f = int(tick.bodies.flags[s])
        if (f & (ld.ALIVE | AUTODISABLE)) != (ld.ALIVE | AUTODISABLE) or (f & ld.KINEMATIC):
            continue
        for v, thr in ((tick.pre_lvel[s], params.lin), (tick.pre_avel[s], params.ang)):
            sp = float(np.sqrt(v @ v))
            if sp != 0.0 and abs(sp - thr) <= 0.1 * thr:
                return False
        tl = float(tick.counters.time[s])
        if tl != 0.0 and tl <= 0.25 * h:
            return False
    return True
